#!/usr/bin/env python3
"""Generate golden input/output vectors by importing the UNMODIFIED reference.

Runs only in the build container (where /root/reference is mounted read-only).
The reference never travels: only the arrays written here (inputs + expected
outputs) are committed under tests/golden/.  Weights are NOT stored -- both
sides regenerate them from influentialrs_amd.synth (the build's own
deterministic generator) and the reference receives them via load_state_dict.

Harness-side shims for API drift between the reference's pinned torch 1.12 /
numpy 1.23 and this image's torch 2.10 / numpy 2.2; no
reference file is touched:
  1. ReduceLROnPlateau(verbose=True) is rejected by torch 2.10 -> subclass
     that swallows `verbose`.
  2. `import wandb` (absent here) -> empty stub module (only needed when the
     data_provider/pipeline modules are imported).
  3. np.Inf alias.
  4. np.save of a ragged list (pipeline.py:244 `histories`) is rejected by numpy >= 1.24 -> retried as an
     object array (harness case only).

The published IRN only runs at batch size 1, so every IRN
golden is produced by looping the reference at B=1.

Usage:  python tests/golden/make_golden.py [case ...]   (default: all cases)
"""
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
os.chdir("/tmp")

import numpy as np
import torch
from torch.optim import lr_scheduler

if not hasattr(np, "Inf"):
    np.Inf = np.inf
sys.modules.setdefault("wandb", types.ModuleType("wandb"))

_RLROP = lr_scheduler.ReduceLROnPlateau


class _RLROPCompat(_RLROP):
    def __init__(self, *a, verbose=None, **k):
        super().__init__(*a, **k)


lr_scheduler.ReduceLROnPlateau = _RLROPCompat

from model.influentialRS import InfluentialNet, IRSNN  # noqa: E402  (reference)
from model.uRS import SampleNet  # noqa: E402
from model.evaluator import Evaluator  # noqa: E402

from influentialrs_amd import synth  # noqa: E402


def _load(net, sd_np):
    sd = {k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}
    missing, unexpected = net.load_state_dict(sd, strict=True), None
    return net


def _pad_ragged(lst, fill=0):
    n = max(len(a) for a in lst)
    out = np.full((len(lst), n), fill, dtype=np.int64)
    lens = np.zeros(len(lst), dtype=np.int64)
    for i, a in enumerate(lst):
        out[i, :len(a)] = a
        lens[i] = len(a)
    return out, lens


def _filtered_rank_list(row, raw):
    """ids (1-based) in the reference's ranking order with the raw history removed
    (model/influentialRS.py:375-379: sort desc, +1, drop history)."""
    order = np.lexsort((np.arange(row.shape[0]), -row.astype(np.float64))) + 1
    return order[~np.isin(order, raw)]


def irn_case(name, cfg_name, n_users, seed=1234, max_path_len=20, full_logits=False, hist_users=None,
             save_x_full=False, tune=True):
    """One IRN golden.  Every output comes from the unmodified reference looped at B = 1.

    `tune` shapes the INPUTS (never the outputs) so that the Hit@k branch (:383-385) and the early-success
    trim (:459-467) are exercised with non-zero counts (round-1 goldens had hit_count = n_early_success = 0):
      user i % 4 == 1: label := the item the reference itself ranks (i // 4) % 20 + 1 among the
                        non-history items  -> a hit;
      user i % 4 == 3: label := an item ranked 21..70  -> no hit, large reciprocal rank;
      user i % 4 == 2: target := an item of the reference's own greedy path (fixed-point search over a few
                        candidates)  -> early success, tail of the path zeroed;
      user i % 4 == 0: the natural row (label = last event, random target)."""
    cfg = synth.make_config(cfg_name)
    sd = synth.irn_state_dict(cfg, seed)
    torch.manual_seed(0)
    net = _load(InfluentialNet(cfg), sd)
    net.eval()
    irn = IRSNN(cfg, net, "cpu")
    irn.eval()
    hist_n = hist_users or max(n_users, 8)
    hists = synth.user_histories(hist_n, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:n_users]
    raws, seqs, users, targets, labels = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    L = cfg.max_len
    hep = L - 2
    K = min(128, cfg.n_item - 1)
    g = {}
    r_us, x_rows, x_full, logits_hep, top_ids, top_vals, gaps_all, probes, probe_ids = [], [], [], [], [], [], [], [], []
    logits_full = []
    hit_total, rr_all, paths_all, early_total, early_users, hit_users = 0, [], [], 0, [], []
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for i in range(n_users):
            u = torch.from_numpy(users[i:i + 1])
            if tune and i % 4 == 2:  # early-success target: an item of the reference's own path for that target
                s = torch.from_numpy(seqs[i:i + 1].copy())
                cand_pos = 3
                for it in range(6):
                    t = torch.from_numpy(targets[i:i + 1])
                    p, _, _, early = irn.get_seq_in_batch(s, u, t, max_path_len, 0, False, 3)
                    if early:
                        break
                    c = int(p[0][min(cand_pos, max_path_len - 1)])
                    targets[i] = c
                    seqs[i, -1] = c
                    s = torch.from_numpy(seqs[i:i + 1].copy())
                    cand_pos = 2 if cand_pos == 3 else 3
            s = torch.from_numpy(seqs[i:i + 1])
            t = torch.from_numpy(targets[i:i + 1])
            r_us.append(irn.get_pif_in_batch(s, u)[0])
            x = net.decoding(s.clone(), u)[0].numpy()
            x_rows.append(x[hep])
            if save_x_full:
                x_full.append(x)
            lg = net.forward(s.clone(), u)[0].numpy()
            if full_logits:
                logits_full.append(lg)
            row = lg[hep].copy()
            del lg
            if cfg.n_item <= 4096:
                logits_hep.append(row)
            if tune and i % 4 in (1, 3):
                fl = _filtered_rank_list(row, raws[i])
                pos = (i // 4) % 20 if i % 4 == 1 else 20 + (7 * i) % 50
                labels[i] = int(fl[pos])
            lab = torch.from_numpy(labels[i:i + 1])
            order = np.lexsort((np.arange(row.shape[0]), -row.astype(np.float64)))
            top = order[:K + 1]
            top_ids.append(top[:K])
            top_vals.append(row[top[:K]])
            gaps_all.append(row[top[:-1]].astype(np.float64) - row[top[1:]].astype(np.float64))
            pid = rng.choice(cfg.n_item, size=64, replace=False)
            probe_ids.append(pid)
            probes.append(row[pid])
            hit, rr = irn.get_accuracy_metrics_in_batch([torch.from_numpy(raws[i])], s, u, t, lab, 20, 0, True)
            hit_total += hit
            if hit:
                hit_users.append(i)
            rr_all.append(rr[0] if len(rr) else 0.0)
            p, tt, hh, early = irn.get_seq_in_batch(s, u, t, max_path_len, 0, False, 3)
            paths_all.append(p[0])
            early_total += early
            if early:
                early_users.append(i)
    g["seqs"], g["users"], g["targets"], g["labels"] = seqs, users, targets, labels
    g["raw"], g["raw_len"] = _pad_ragged(raws)
    g["r_u"] = np.array(r_us, dtype=np.float32).reshape(-1)
    g["x_hep"] = np.stack(x_rows)
    if save_x_full:
        g["x_full"] = np.stack(x_full)
    if logits_hep:
        g["logits_hep"] = np.stack(logits_hep)
    if full_logits:
        g["logits_full"] = np.stack(logits_full)
    # the reference's ranking of row `hep`: the first K ids / values in (score desc, id asc) order and the K
    # adjacent score gaps gap[j] = s(rank j) - s(rank j+1), j = 0..K-1 (float64 differences of float32 logits)
    g["top_ids0"] = np.stack(top_ids).astype(np.int64)
    g["top_vals"] = np.stack(top_vals)
    g["top_gaps"] = np.stack(gaps_all)
    g["probe_ids0"] = np.stack(probe_ids).astype(np.int64)
    g["probe_vals"] = np.stack(probes)
    g["hit_count"] = np.array(hit_total)
    g["hit_users"] = np.array(hit_users, dtype=np.int64)
    g["rr"] = np.array(rr_all)
    g["paths"] = np.stack(paths_all)
    g["n_early_success"] = np.array(early_total)
    g["early_users"] = np.array(early_users, dtype=np.int64)
    g["meta"] = np.array([cfg_name, str(seed), str(max_path_len), torch.__version__, str(hist_n)])
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
    mg = g["top_gaps"][:, :100].min(axis=1)
    print(f"[golden] {name}: users={n_users} min gap(top-101)={mg.min():.3e} users with a gap<2e-5: "
          f"{int((mg < 2e-5).sum())} hit={hit_total} early={early_total} {early_users}", flush=True)


def _eval_inputs(cfg, n_rows, seed, irn_cfg_name):
    """Evaluator inputs in the DatasetEvalNN1 layout (data_provider.py:711-760)
    built by the REFERENCE's own class from synthetic histories/paths/targets."""
    sys.modules.setdefault("sklearn", __import__("sklearn"))
    from data_provider import DatasetEvalNN1, DataLoaderEvalNN1  # reference
    rng = np.random.default_rng(seed)
    hists = synth.user_histories(max(n_rows, 8), cfg.n_item, seed=7)
    histories, paths, targets = [], [], []
    for i in range(n_rows):
        h = hists[i][:-1]
        keep = [3, cfg.max_len - 10, cfg.max_len + 7, cfg.max_len - 1][i % 4]
        h = h[-max(keep, 1):]
        hs = set(int(v) for v in h)
        t = int(rng.integers(1, cfg.n_item + 1))
        while t in hs:
            t = int(rng.integers(1, cfg.n_item + 1))
        plen = int(rng.integers(3, min(20, cfg.max_len // 2) + 1))
        p = np.zeros(20, dtype=np.float32)
        items = rng.choice(cfg.n_item, size=plen, replace=False) + 1
        p[:plen] = items
        if i % 3 == 0 and plen > 2:  # early success: target inside the path, tail zeroed
            pos = int(rng.integers(1, plen))
            p[pos] = t
            p[pos + 1:] = 0
        histories.append(h)
        paths.append(p)
        targets.append(t)
    ds = DatasetEvalNN1(histories, np.stack(paths), np.array(targets, dtype=np.int64), seq_len=cfg.max_len)
    dl = DataLoaderEvalNN1(ds, batch_size=n_rows, shuffle=False, num_workers=0)
    h, d, t, sp, lp = next(iter(dl))
    hp, hl = _pad_ragged(histories)
    return (h, d, t, sp, lp), dict(in_histories=hp, in_histories_len=hl, in_paths=np.stack(paths),
                                   in_targets=np.array(targets, dtype=np.int64))


def eval_case(name, cfg_name, n_rows, seed=17):
    cfg = synth.make_config(cfg_name)
    sd = synth.irn_state_dict(cfg, seed, evaluator=True)
    torch.manual_seed(0)
    net = _load(SampleNet(cfg), sd)
    net.eval()
    ev = Evaluator(cfg, net, "cpu")
    ev.eval()
    (h, d, t, sp, lp), extra = _eval_inputs(cfg, n_rows, seed, cfg_name)
    g = dict(extra)
    g["histories"], g["new_seqs"], g["targets"] = h.numpy().copy(), d.numpy().copy(), t.numpy().copy()
    g["start_pos"], g["l_paths"] = sp.numpy().copy(), lp.numpy().copy()
    with torch.no_grad():
        g["pp"] = np.array(ev.get_pp_in_batch(d, sp, lp))
        irr, ir = ev.get_rr_increase_in_batch(h, d, t)
        g["irr"], g["ir"] = irr, ir
        tp, pp_, avg, ioi = ev.get_grad_in_batch(h.clone(), d, t, sp, lp)
        g["t_probs"], g["p_probs"], g["avg_ps"], g["iois"] = tp, pp_, np.array(avg), np.array(ioi)
        lg = net.forward(d[:, :-1])[0].numpy()
        g["logits_row0_full"] = lg if cfg.n_item <= 512 else lg[:4]
    g["meta"] = np.array([cfg_name, str(seed), torch.__version__])
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
    print(f"[golden] {name}: rows={n_rows} pp[0]={g['pp'][0]:.5f} ir={ir[:4]}")
    eval_accuracy_case(name.replace("eval_", "eval_accuracy_"), cfg_name, seed, ev=ev)


ACC_TOP_K, ACC_USE_H = (1, 20), (True, False)


def accuracy_batch(cfg, sd, seed):
    """The 8 post-padded rows [8, max_len + 1] of the accuracy golden.  The logits a row is ranked on sit at the position in
    front of its label and the mask is causal, so a label can be chosen AFTER the rest of the row, from the CPU oracle's ranking
    of that position:
      0: a full window (no zero: end = max_len, the label is the column seq[:-1] cuts off)
      1: the label also occurs in its history (skipped under use_h, counted without)
      2 / 3: the label's rank with the history removed is exactly 20 / exactly 1
      4 / 5: the label's rank over the whole catalog is exactly 20 / exactly 1
      6: the label's filtered rank is 21 (one behind a hit at top_k = 20)
      7: the shortest row, one history item and the label."""
    from oracle import oracle_np as O
    L, N = cfg.max_len, cfg.n_item
    rng = np.random.default_rng(seed + 1)
    lens = [L + 1, L // 2, L - 3, 5, L // 3, 7, L - 1, 2]
    seqs = np.zeros((8, L + 1), dtype=np.int64)
    for i, n in enumerate(lens):
        seqs[i, :n] = rng.choice(N, size=n, replace=False) + 1
    seqs[1, lens[1] - 1] = seqs[1, 2]
    W, b = sd["project.weight"], sd["project.bias"]
    for i, (filtered, place) in {2: (True, 20), 3: (True, 1), 4: (False, 20), 5: (False, 1), 6: (True, 21)}.items():
        end = lens[i] - 1
        x, _ = O.decode(sd, cfg, seqs[i, :-1], None, evaluator=True)
        order = O.topk(O.score_chain(x[end - 1], W, b), N)[1] + 1  # 1-based ids, (score desc, id asc)
        if filtered:
            order = order[~np.isin(order, seqs[i, :end])]
        seqs[i, end] = order[place - 1]
    return seqs


def eval_accuracy_case(name, cfg_name, seed=17, ev=None):
    """Evaluator.get_accuracy_metrics_in_batch of the unmodified reference on accuracy_batch(), at every (top_k, use_h) of
    ACC_TOP_K x ACC_USE_H: arrays only (the rows as int16, hit counts, reciprocal ranks)."""
    cfg = synth.make_config(cfg_name)
    sd = synth.irn_state_dict(cfg, seed, evaluator=True)
    if ev is None:
        torch.manual_seed(0)
        net = _load(SampleNet(cfg), sd)
        net.eval()
        ev = Evaluator(cfg, net, "cpu")
        ev.eval()
    seqs = accuracy_batch(cfg, sd, seed)
    assert seqs.max() < 2 ** 15
    g = {"seqs": seqs.astype(np.int16)}
    with torch.no_grad():
        for k in ACC_TOP_K:
            for h in ACC_USE_H:
                hit, rr = ev.get_accuracy_metrics_in_batch(torch.from_numpy(seqs), k, h)
                g[f"hit_k{k}_h{int(h)}"] = np.array(hit, dtype=np.int64)
                g[f"rr_k{k}_h{int(h)}"] = np.asarray(rr, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **g)
    print(f"[golden] {name}: " + " ".join(f"{k}={v.tolist() if v.ndim == 0 else np.round(1 / v).astype(int).tolist()}"
                                           for k, v in g.items() if k != "seqs"))


def contract_case():
    """Input contract and checkpoint key set (section 5) from the
    reference's own classes: DataLoaderEvalIRS._collate_fn (data_provider.py:591-617),
    DatasetEvalNN1 (data_provider.py:711-760), InfluentialNet / SampleNet state_dict."""
    from data_provider import DataLoaderEvalIRS, DatasetNN  # reference
    g = {}
    cfg = synth.make_config("default")
    hists = synth.user_histories(12, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)
    for gap in (0, 5):
        dl = DataLoaderEvalIRS(dataset=DatasetNN([list(r) for r in rows]), batch_size=len(rows), shuffle=False,
                               num_workers=0, gap_len=gap, seq_len=cfg.max_len)
        raw, seq, u, t, l = next(iter(dl))
        g[f"collate_gap{gap}_seq"] = seq.numpy()
        g[f"collate_gap{gap}_users"] = u.numpy()
        g[f"collate_gap{gap}_targets"] = t.numpy()
        g[f"collate_gap{gap}_labels"] = l.numpy()
        g[f"collate_gap{gap}_raw"], g[f"collate_gap{gap}_raw_len"] = _pad_ragged([r.numpy() for r in raw])
    tiny = synth.make_config("tiny")
    net = InfluentialNet(tiny)
    g["irn_keys"] = np.array(list(net.state_dict().keys()))
    g["irn_shapes"] = np.array([",".join(map(str, v.shape)) for v in net.state_dict().values()])
    et = synth.make_config("eval_tiny")
    snet = SampleNet(et)
    g["eval_keys"] = np.array(list(snet.state_dict().keys()))
    g["eval_shapes"] = np.array([",".join(map(str, v.shape)) for v in snet.state_dict().values()])
    np.savez_compressed(os.path.join(OUT, "contract.npz"), **g)
    print("[golden] contract:", len(g["irn_keys"]), "irn keys,", len(g["eval_keys"]), "eval keys")


def harness_case():
    """the reference's UNMODIFIED pipeline.test_model (pipeline.py:151-247) and
    pipeline.evaluate_prob (:250-331) run end to end on CPU, at the only batch size the published IRN
    supports (1), from checkpoints written in the reference's own format.  `dp` is a stub whose
    get_random_evaluate_data returns synthetic rows in the reference's row layout
    [new_seq, user_id, random_target, label] (data_provider.py:398-449).  Stored: the inputs, the printed
    aggregates and the six result arrays."""
    import contextlib
    import io
    import re
    import tempfile
    import pipeline  # reference, unmodified
    tmp = tempfile.mkdtemp(dir="/tmp")
    os.chdir(tmp)
    cfg = synth.make_config("tiny")
    ecfg = synth.make_config("eval_tiny")
    n_users, max_path_len = 10, 6
    for k, v in dict(model_store_path=tmp + "/", dataset="syn", method="IRN", use_train=False, gap_len=0, batch_size=1,
                     top_k=20, use_h=True, max_path_len=max_path_len, sample=False, sample_k=3, use_wandb=False).items():
        setattr(cfg, k, v)
    ecfg.batch_size = 4
    os.makedirs(os.path.join(tmp, "syn"))
    torch.manual_seed(0)
    net = _load(InfluentialNet(cfg), synth.irn_state_dict(cfg, 1234))
    irn = IRSNN(cfg, net, "cpu")
    torch.save({"epoch": 3, "state_dict": net.state_dict(), "optimizer": irn.optimizer.state_dict()},
               os.path.join(tmp, "syn", "irn_params.pth.tar"))
    snet = _load(SampleNet(ecfg), synth.irn_state_dict(ecfg, 17, evaluator=True))
    ev = Evaluator(ecfg, snet, "cpu")
    torch.save({"epoch": 3, "state_dict": snet.state_dict(), "optimizer": ev.optimizer.state_dict()},
               os.path.join(tmp, "syn", "eval_params.pth.tar"))
    hists = synth.user_histories(n_users, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)

    class _DP:
        def get_random_evaluate_data(self, **kw):
            return [list(r) for r in rows]

    orig_save = np.save

    def save_ragged(file, arr, *a, **k):
        try:
            return orig_save(file, arr, *a, **k)
        except ValueError:
            o = np.empty(len(arr), dtype=object)
            for i, x in enumerate(arr):
                o[i] = x
            return orig_save(file, o, *a, **k)

    pipeline.np.save = save_ragged
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            pipeline.test_model(cfg, _DP(), device="cpu")
            pipeline.evaluate_prob(cfg, dict(vars(ecfg)), _DP(), device="cpu")
    finally:
        pipeline.np.save = orig_save
    out = buf.getvalue()

    def grab(label):
        return float(re.search(re.escape(label) + r": (-?[0-9.eE+-]+|nan|inf)", out).group(1))

    g = {}
    g["in_raw"], g["in_raw_len"] = _pad_ragged([r[0] for r in rows])
    g["in_users"] = np.array([r[1] for r in rows], dtype=np.int64)
    g["in_targets"] = np.array([r[2] for r in rows], dtype=np.int64)
    g["in_labels"] = np.array([r[3] for r in rows], dtype=np.int64)
    g["max_path_len"] = np.array(max_path_len)
    g["printed"] = np.array([grab("Hit rate"), grab("MRR"), grab("Early Success"), grab("Early Success Rate"),
                             grab("The perplexity"), grab("The increase of interest"),
                             grab("The increase of reverse ranking"), grab("The increase of ranking"),
                             grab("The average acceptance probability")])
    rd = os.path.join(tmp, "results", "syn", "IRN")
    g["paths"] = np.load(os.path.join(rd, "paths_d_%d.npy" % max_path_len))
    g["targets"] = np.load(os.path.join(rd, "targets_d_%d.npy" % max_path_len))
    g["r_u"] = np.load(os.path.join(rd, "r_u.npy"))
    h = np.load(os.path.join(rd, "histories.npy"), allow_pickle=True)
    g["histories"], g["histories_len"] = _pad_ragged([np.asarray(x) for x in h])
    g["p_probs"] = np.load(os.path.join(rd, "p_probs.npy"))
    g["t_probs"] = np.load(os.path.join(rd, "t_probs.npy"))
    g["dtypes"] = np.array([str(g[k].dtype) for k in ("paths", "targets", "r_u", "p_probs", "t_probs")])
    g["meta"] = np.array(["tiny", "eval_tiny", torch.__version__])
    np.savez_compressed(os.path.join(OUT, "harness_tiny.npz"), **g)
    print("[golden] harness_tiny: printed =", g["printed"], "paths", g["paths"].shape, g["paths"].dtype)


def train_case():
    """The training side as the unmodified reference runs it, dropout 0 (the only source of randomness):
    IRSNN.train_batch looped at B = 1 over four users (sequential Adam steps, influentialRS.py:278-310) with
    get_loss_on_eval_data before and after; Evaluator.train_batch at B = 4 (evaluator.py:53-68), three steps."""
    g = {}
    cfg = synth.make_config("tiny", dropout=0.0)
    torch.manual_seed(0)
    net = _load(InfluentialNet(cfg), synth.irn_state_dict(cfg, 1234))
    irn = IRSNN(cfg, net, "cpu")
    hists = synth.user_histories(8, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:4]
    raws, seqs, users, targets, labels = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    g["irn_seqs"], g["irn_users"] = seqs, users
    ev0 = [irn.get_loss_on_eval_data(torch.from_numpy(seqs[i:i + 1]), torch.from_numpy(users[i:i + 1])) for i in range(4)]
    tr = [irn.train_batch(torch.from_numpy(seqs[i:i + 1]), torch.from_numpy(users[i:i + 1])) for i in range(4)]
    ev1 = [irn.get_loss_on_eval_data(torch.from_numpy(seqs[i:i + 1]), torch.from_numpy(users[i:i + 1])) for i in range(4)]
    g["irn_eval_before"], g["irn_train"], g["irn_eval_after"] = np.array(ev0), np.array(tr), np.array(ev1)
    g["irn_bias_after"] = net.project.bias.detach().numpy().copy()

    ecfg = synth.make_config("eval_tiny", dropout=0.0)
    torch.manual_seed(0)
    snet = _load(SampleNet(ecfg), synth.irn_state_dict(ecfg, 17, evaluator=True))
    ev = Evaluator(ecfg, snet, "cpu")
    rng = np.random.default_rng(3)
    B, L = 4, ecfg.max_len
    tgt = np.zeros((B, L), dtype=np.int64)
    for i in range(B):  # post-padded sequences, as the evaluator's loader emits them
        n = int(rng.integers(5, L + 1))
        tgt[i, :n] = rng.integers(1, ecfg.n_item + 1, size=n)
    g["ev_target"] = tgt
    t = torch.from_numpy(tgt)
    g["ev_eval_before"] = np.array([ev.get_loss_on_eval_data(t)])
    g["ev_train"] = np.array([ev.train_batch(t) for _ in range(3)])
    g["ev_eval_after"] = np.array([ev.get_loss_on_eval_data(t)])
    g["meta"] = np.array([torch.__version__])
    np.savez_compressed(os.path.join(OUT, "train_tiny.npz"), **g)
    print(f"[golden] train_tiny: irn train {g['irn_train']} eval {ev0[0]:.5f} -> {ev1[0]:.5f}; evaluator {g['ev_train']}")


CASES = {
    "irn_tiny": lambda: irn_case("irn_tiny", "tiny", 12, full_logits=True, save_x_full=True),
    "irn_default": lambda: irn_case("irn_default", "default", 32),
    "irn_c1": lambda: irn_case("irn_c1", "c1", 32),
    "irn_c2": lambda: irn_case("irn_c2", "c2", 32),
    "irn_c3": lambda: irn_case("irn_c3", "c3", 8, max_path_len=4),
    "irn_c4d": lambda: irn_case("irn_c4d", "c4d", 32),
    "eval_tiny": lambda: eval_case("eval_tiny", "eval_tiny", 8),
    "eval_default": lambda: eval_case("eval_default", "eval_default", 6),
    "eval_accuracy_tiny": lambda: eval_accuracy_case("eval_accuracy_tiny", "eval_tiny"),
    "eval_accuracy_default": lambda: eval_accuracy_case("eval_accuracy_default", "eval_default"),
    "contract": contract_case,
    "harness_tiny": harness_case,
    "train_tiny": train_case,
}

if __name__ == "__main__":
    which = sys.argv[1:] or list(CASES)
    for c in which:
        CASES[c]()
