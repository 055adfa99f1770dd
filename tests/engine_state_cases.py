"""State between calls of one engine, as a table of probes and schedules (test infrastructure, shared by
tests/test_engine_state_cases.py on the CPU and tests/test_gpu_engine_state.py on the GPU).

All calls of a context share one caller-owned workspace (workspace_walk in influentialrs_amd/csrc/capi.hip) and the context keeps
state in it and on the host between calls: the HOLDERS below.  A PROBE is one public Engine call, or a fixed short group of calls,
on seeded inputs of a fixed shape; it names the holders it writes and the ones it relies on, so that the CPU test can show that
every holder is written by one probe and relied on by another.  A SCHEDULE orders probes on ONE engine: all_pairs() makes every
ordered pair of probes adjacent, shuffled() is the order of the variants (another stream, a re-bound workspace, two engines).
The GPU module compares every occurrence of every probe with the same call on a fresh engine that has made no other call.

Nothing here needs a GPU: the probe callables only touch torch when they run."""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import decoder_route_cases as RC
from influentialrs_amd import synth
from influentialrs_amd._lib import (IRS_REPLAY_SLOT, IRS_SWEEP_BF16, IRS_SWEEP_EXHAUSTIVE, IRS_SWEEP_F32)

# ---------------------------------------------------------------------------------------------------------------- state holders
HOLDERS = {
    "arrive": "step_ctr[8..40): arrival counters of k_topk_direct; zeroed by irs_bind_workspace, then by the last workgroup",
    "fb_count": "rows recorded for the cooperative exhaustive fallback (with fb_list / exh_keys); zeroed by a swept top-k kernel",
    "cand_cnt": "per-row candidate bucket counters of the swept top-k",
    "m_dev": "number of packed rows of the decode plan",
    "n_wg_dev": "workgroups in use of the sequence-resident plan",
    "un_count": "live users of the stop-at-target loops (with the un_* ping-pong)",
    "step_pair": "step_ctr[0..1] / step_pair: the step counter the merged small-batch loop hands over inside the plan kernel",
    "thr": "carried emission thresholds: thr_valid / thr_M / thr_k / thr_age on the host, the thr buffer on the device",
    "proj_stale": "a training entry point ran since irs_finalize_weights",
    "surv_rows": "rows of the running search call, the layout of the bound survivor scratch",
    "seq_last": "the last decode took the sequence-resident launch (and the route it reported)",
    "g_greedy": "captured step of the greedy / sampled loop",
    "g_beam": "captured step of the beam loop",
    "plan_tables": "tok_row / seq_cnt / seq_off / seq_qrow / seq_padq and the tile tables a decode of one shape leaves behind",
    "activations": "act_* buffers and the fragment-major / plane copies a decode leaves behind",
    "beam_pingpong": "bm[2] / bm_side[2]: the two sides of the beam state",
    "until_pingpong": "un_seq / un_user / un_hep / un_map [2]: the compacted live users",
}
# holders of the context that no probe of this table can reach, with the reason
UNPROBED_HOLDERS = {
    "g_sharded": "the captured step of the item-sharded loops: no sharded probe runs on one GPU (tests/test_gpu_comm.py and "
                 "tests/test_gpu_multirank.py hold it, irs_sharded_graph_state reports it)",
}

P_GREEDY, P_G70, P_UNTIL, P_BEAM, BEAM_W = 4, 3, 6, 4, 4
K = 100
D = 128
L_ITEMS = 600_017  # engine L: the smallest project shape with the threshold carry (>= 524288) and the cooperative fallback (>= 262144)
S_ROWS = 192       # engine S: max_rows = max_seqs
L_ROWS = 288       # engine L: max_rows


@dataclass(frozen=True)
class Probe:
    id: str
    engine: str                       # "S" (the model engine) or "L" (the big-catalog scoring engine)
    run: Callable                     # run(env) -> tuple of tensors / ints; env.eng the Engine, env.inp the device inputs, env.held
    writes: Tuple[str, ...]           # HOLDERS it leaves changed
    relies: Tuple[str, ...]           # HOLDERS whose value from BEFORE the call can reach its result if a reset or a drop is lost
    abi: Tuple[str, ...]              # the include/irs_hip.h functions taking `void *stream` that it reaches
    route: Optional[str] = None       # decode probes: the decoder_route_cases id whose route the call must report
    case: Optional[RC.Case] = None    # decode probes: the case (for the sample and the bar of tests/test_gpu_decoder_routes.py)
    mask_fallback: Tuple[int, ...] = ()  # outputs (status words) whose bit 0, IRS_ROW_FALLBACK, may depend on the previous call
    kind: str = ""                    # how the GPU module checks the expected value against a reference


def s_config():
    return synth.make_config("c2", n_layers=2)


# ------------------------------------------------------------------------------------------------------------- engine S: inputs
def _windows(B: int, cfg, seed: int):
    """Seeded IRN windows (pre-padded, the target last) with the edge contents of the route tests on the first sequences."""
    L, N = cfg.max_len, cfg.n_item
    g = np.random.default_rng(seed)
    seqs = np.zeros((B, L), dtype=np.int64)
    pos = np.full(B, L - 2, dtype=np.int32)
    for b in range(B):
        n = int(np.clip(g.lognormal(np.log(0.4 * L), 0.8), 2, L))
        seqs[b, L - n:] = g.integers(1, N + 1, size=n)
    edges = []
    if B > 2:
        seqs[1] = 0
        seqs[1, L - 1] = int(g.integers(1, N + 1))      # the target alone
        pos[1] = L - 1
        seqs[2] = g.integers(1, N + 1, size=L)          # a full window
        pos[2] = L - 1
        edges = [1, 2]
    if B > 4:
        seqs[3] = np.array([1, N] * (L // 2))           # item ids 1 and n_item, consumed at 0
        pos[3] = 0
        edges.append(3)
    users = g.integers(0, cfg.n_user, size=B).astype(np.int64)
    users[0], users[-1] = 0, cfg.n_user - 1
    return seqs, users, pos, edges


def _search_windows(B: int, cfg, seed: int, first: int = 0):
    """Evaluation rows as the harness builds them: distinct history items, a target absent from the history."""
    hists = synth.user_histories(first + B, cfg.n_item, seed=seed)
    rows = synth.eval_rows(hists, cfg.n_item, seed=seed + 4)[first:first + B]
    _, seqs, users, targets, _ = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    return seqs, users, targets


def until_windows(oracle, sd, cfg, seed: int = 0):
    """The windows of the stop-at-target probe: 8 users.  User b is offered as target the item its own greedy path takes at step
    1 + b % 4; the target sits in the window, so the path depends on it, and the offer is kept only where the path under the new
    target still reaches it before the last step (found on the CPU with oracle.get_seq), for five users at the most.  Returns
    (seqs, users, targets, arrive) with arrive[b] = the step at which user b chooses its target, or -1."""
    seqs, users, targets = _search_windows(8, cfg, 31 + seed)
    seqs, targets = seqs.copy(), targets.copy()
    natural = oracle.get_seq(sd, cfg, seqs, users, targets, max_path_len=P_UNTIL)[0]
    kept = 0
    for b in range(8):
        t = int(natural[b][1 + b % 4])
        if kept == 5 or t in seqs[b, :-1]:
            continue
        row = seqs[b:b + 1].copy()
        row[0, -1] = t
        p = oracle.get_seq(sd, cfg, row, users[b:b + 1], np.array([t]), max_path_len=P_UNTIL)[0][0]
        if t in p[:P_UNTIL - 1]:
            seqs[b, -1] = targets[b] = t
            kept += 1
    paths = oracle.get_seq(sd, cfg, seqs, users, targets, max_path_len=P_UNTIL)[0]
    arrive = np.array([int(np.where(paths[b] == targets[b])[0][0]) if (paths[b] == targets[b]).any() else -1 for b in range(8)])
    return seqs, users, targets, arrive


def s_inputs(seed: int = 0, until=None) -> Dict[str, np.ndarray]:
    """Every input of engine S's probes, as numpy arrays (the GPU module uploads them once).  `until`: until_windows()'s result."""
    cfg = s_config()
    L, N = cfg.max_len, cfg.n_item
    inp: Dict[str, np.ndarray] = {}
    for B in (1, 8, 70, 165, 176):
        seqs, users, pos, edges = _windows(B, cfg, 1000 + B + seed)
        inp[f"win{B}_seq"], inp[f"win{B}_usr"], inp[f"win{B}_pos"] = seqs, users, pos
        inp[f"win{B}_edges"] = np.array(edges, dtype=np.int64)
    g = np.random.default_rng(50 + seed)
    for M in (8, 70):
        inp[f"rows{M}"] = g.standard_normal((M, D)).astype(np.float32)
    inp["rows8b"] = g.standard_normal((8, D)).astype(np.float32)  # (the LSE probe's own rows)
    ids = g.integers(0, N, size=(8, 17)).astype(np.int64)
    ids[0, 0] = -1
    inp["gather_ids"] = ids
    inp["labels8"] = g.integers(0, N, size=8).astype(np.int64)
    hist = g.integers(0, N, size=(8, 23)).astype(np.int64)
    hist[:, 3], hist[:, 5] = hist[:, 4], -1
    inp["hist8"] = hist
    ce = g.integers(0, N, size=8).astype(np.int64)
    ce[3] = -1
    inp["ce_labels"] = ce
    for name, B, s, first in (("s8", 8, 7, 0), ("s70", 70, 9, 0), ("beam", 2, 7, 8)):
        seqs, users, targets = _search_windows(B, cfg, s + seed, first)
        inp[f"{name}_seq"], inp[f"{name}_usr"] = seqs, users
        inp[f"{name}_hep"] = np.full(B, L - 2, dtype=np.int32)
    if until is not None:
        inp["until_seq"], inp["until_usr"] = until[0], until[1]
        inp["until_hep"] = np.full(8, L - 2, dtype=np.int32)
    excl = g.integers(0, N, size=(8, 12)).astype(np.int64)
    excl[:, 7] = -1
    inp["excl8"] = excl  # (the GPU module puts step 0's chosen item of the plain probe into column 0)
    seqs, users, _, _ = _windows(4, cfg, 2000 + seed)
    inp["train_seq"], inp["train_usr"] = seqs, users
    inp["train_dx"] = (g.standard_normal((4, L, D)) * 0.1).astype(np.float32)
    return inp


# ------------------------------------------------------------------------------------------------------------- engine S: probes
def _decode(B: int, want_x: bool = False, seq_mode=None):
    def run(env):
        e, i = env.eng, env.inp
        if seq_mode is not None:
            e.decoder_seq = seq_mode
        try:
            x, xr, ru = e.decode(i[f"win{B}_seq"], i[f"win{B}_usr"], want_x=want_x, pos=i[f"win{B}_pos"], want_r_u=True)
            env.route = e.decoder_route_last
        finally:
            if seq_mode is not None:
                e.decoder_seq = None  # back to auto: the second setter call of the probe (both drop the captured steps)
        return (x, xr, ru) if want_x else (xr, ru)
    return run


def _topk(rows: str, k: int = K, sweep: int = IRS_SWEEP_BF16, carry: bool = False):
    def run(env):
        return env.eng.score_topk(env.inp[rows], k, sweep, carry=carry)
    return run


def _topk_lse(rows: str, k: int = K):
    def run(env):
        return env.eng.score_topk_lse(env.inp[rows], k, IRS_SWEEP_BF16)
    return run


def _gather_count(rows: str, ids: str, labels: str, hist: str):
    def run(env):
        e, i = env.eng, env.inp
        got = e.score_gather(i[rows], i[ids])
        ref = e.score_gather(i[rows], i[labels].view(-1, 1))[:, 0].contiguous()
        return got, ref, e.score_count_before(i[rows], ref, i[labels], i[hist])
    return run


def _greedy(name: str, P: int, **kw):
    def run(env):
        i = env.inp
        seq, hep = i[f"{name}_seq"].clone(), i[f"{name}_hep"].clone()
        out = env.eng.generate_paths(seq, i[f"{name}_usr"], hep, P, k=K, **{k: (i[v] if isinstance(v, str) else v) for k, v in kw.items()})
        if len(out) == 3:
            return out[0], out[1], seq, hep, out[2][0], out[2][1], out[2][2]
        return out[0], out[1], seq, hep
    return run


def _greedy_held(name: str, P: int):
    """use_graph=True on caller-held seqs / hep / paths / status: their addresses stay in the key of the captured step, so a later
    occurrence is a genuine cache hit, or a capture after a drop."""
    def run(env):
        import torch
        i = env.inp
        if "greedy" not in env.held:
            env.held["greedy"] = (torch.empty_like(i[f"{name}_seq"]), torch.empty_like(i[f"{name}_hep"]),
                                  torch.empty((i[f"{name}_seq"].shape[0], P), dtype=torch.float32, device=i[f"{name}_seq"].device),
                                  torch.empty_like(i[f"{name}_hep"]))
        seq, hep, paths, status = env.held["greedy"]
        seq.copy_(i[f"{name}_seq"])
        hep.copy_(i[f"{name}_hep"])
        paths.zero_()
        status.zero_()
        env.eng.generate_paths(seq, i[f"{name}_usr"], hep, P, k=K, use_graph=True, paths=paths, status=status)
        return paths.clone(), status.clone(), seq.clone(), hep.clone()
    return run


def _until(name: str, P: int):
    def run(env):
        i = env.inp
        paths, status, steps, row_steps = env.eng.generate_paths_until(i[f"{name}_seq"].clone(), i[f"{name}_usr"], i[f"{name}_hep"].clone(),
                                                                      P, k=K, check_every=1)
        return paths, status, steps, row_steps
    return run


def _beam(name: str, until: bool):
    def run(env):
        e, i = env.eng, env.inp
        if until:
            paths, scores, status, fin, steps, wsteps, win = e.beam_search_until(i[f"{name}_seq"], i[f"{name}_usr"], i[f"{name}_hep"], P_BEAM,
                                                                                BEAM_W, k=K, want_windows=True)
            return paths, scores, status, fin, win, steps, wsteps
        return e.beam_search(i[f"{name}_seq"], i[f"{name}_usr"], i[f"{name}_hep"], P_BEAM, BEAM_W, k=K, use_graph=True, want_windows=True)
    return run


def replay_rows(B: int = 8, P: int = P_GREEDY):
    ru = np.repeat(np.arange(B), P).astype(np.int32)
    rs = np.tile(np.arange(P), B).astype(np.int32)
    return ru, rs


def _replay(name: str):
    """replay_paths on the paths of the plain probe `name` (env.inp["replay_paths"], int64: the GPU module takes them from that
    probe's expected value)."""
    def run(env):
        i = env.inp
        return env.eng.replay_paths(IRS_REPLAY_SLOT, i[f"{name}_seq"], i["replay_paths"], i["replay_ru"], i["replay_rs"],
                                    hep0=i[f"{name}_hep"], users=i[f"{name}_usr"])
    return run


def _ce(rows: str, labels: str):
    def run(env):
        out = env.eng.ce_forward(env.inp[rows], env.inp[labels])
        env.eng.finalize()  # irs_ce_forward marks the derived catalog stale: the filtered entry points refuse until this
        return out
    return run


def _train(seed: int = 77, p: float = 0.05):
    def run(env):
        e, i = env.eng, env.inp
        x, saved = e.train_forward(i["train_seq"], i["train_usr"], p, seed)
        grads = e.train_backward(i["train_seq"], i["train_usr"], p, seed, saved, i["train_dx"])
        return x, grads
    return run


def _case(route_id: str, B: int, **kw) -> RC.Case:
    return RC.Case(f"state_{route_id}_b{B}", "c2", B, RC.BY_ID[route_id].route, over=dict(n_layers=2), full_check=False, **kw)


_DEC_W = ("m_dev", "plan_tables", "activations", "seq_last")
_DEC_R = ("m_dev", "plan_tables", "activations")
_LOOP_ABI = ("irs_decode", "irs_score_topk", "irs_score_topk_carry", "irs_path_step")

S_PROBES: List[Probe] = [
    # ---- decodes: one per plan kernel and per layer family of the shape (thresholds: decoder_route_cases.py)
    Probe("dec_b1", "S", _decode(1), _DEC_W, _DEC_R, ("irs_decode",), route="c2_b1_att_fused", case=_case("c2_b1_att_fused", 1), kind="decode"),
    Probe("dec_b8", "S", _decode(8), _DEC_W, _DEC_R, ("irs_decode",), route="c2_b2", case=_case("c2_b2", 8), kind="decode"),
    Probe("dec_b70", "S", _decode(70), _DEC_W, _DEC_R, ("irs_decode",), route="c2_b65", case=_case("c2_b65", 70), kind="decode"),
    Probe("dec_b176_seq1", "S", _decode(176, seq_mode=1), _DEC_W + ("n_wg_dev", "g_greedy", "g_beam"), _DEC_R + ("n_wg_dev",),
          ("irs_decode",), route="c2_b164_seq1", case=_case("c2_b164_seq1", 176, seq=1), kind="decode"),
    Probe("dec_b165_seq1", "S", _decode(165, seq_mode=1), _DEC_W + ("n_wg_dev", "g_greedy", "g_beam"), _DEC_R + ("n_wg_dev",),
          ("irs_decode",), route="c2_b164_seq1", case=_case("c2_b164_seq1", 165, seq=1), kind="decode"),
    Probe("dec_b176_seq0", "S", _decode(176, seq_mode=0), _DEC_W + ("g_greedy", "g_beam"), _DEC_R, ("irs_decode",), route="c2_b164",
          case=_case("c2_b164", 176, seq=0), kind="decode"),
    Probe("dec_full_b8", "S", _decode(8, want_x=True), ("activations", "seq_last"), ("activations",), ("irs_decode",), route="c2_full_b8",
          case=_case("c2_full_b8", 8, rows_only=False), kind="decode"),
    # ---- scoring on the small catalog: the direct top-k
    Probe("topk_m8", "S", _topk("rows8"), ("arrive",), ("arrive", "proj_stale"), ("irs_score_topk",), kind="fresh"),
    Probe("topk_m70", "S", _topk("rows70"), ("arrive",), ("arrive", "proj_stale"), ("irs_score_topk",), kind="fresh"),
    Probe("topk_lse_m8", "S", _topk_lse("rows8b"), ("arrive",), ("arrive",), ("irs_score_topk_lse",), kind="fresh"),
    Probe("gather_count_m8", "S", _gather_count("rows8", "gather_ids", "labels8", "hist8"), (), (),
          ("irs_score_gather", "irs_score_count_before"), kind="fresh"),
    # ---- search loops
    Probe("greedy_b8", "S", _greedy("s8", P_GREEDY), _DEC_W + ("arrive", "step_pair", "thr"), _DEC_R + ("arrive", "step_pair", "surv_rows", "proj_stale"), ("irs_generate_paths",), kind="greedy"),
    Probe("greedy_b8_graph", "S", _greedy_held("s8", P_GREEDY), _DEC_W + ("arrive", "step_pair", "g_greedy"),
          _DEC_R + ("arrive", "step_pair", "g_greedy", "seq_last"), ("irs_generate_paths",), kind="fresh"),
    # (use_graph with buffers of its own: the capture replaces the step greedy_b8_graph left in the cache)
    Probe("greedy_b70", "S", _greedy("s70", P_G70, use_graph=True), _DEC_W + ("arrive", "step_pair", "g_greedy"),
          _DEC_R + ("arrive", "step_pair", "g_greedy"), ("irs_generate_paths",), kind="greedy"),
    Probe("until_b8", "S", _until("until", P_UNTIL), _DEC_W + ("arrive", "un_count", "until_pingpong"),
          _DEC_R + ("arrive", "un_count", "until_pingpong"), ("irs_generate_paths_until",), kind="fresh"),
    Probe("beam_graph", "S", _beam("beam", False), _DEC_W + ("arrive", "g_beam", "beam_pingpong"),
          _DEC_R + ("arrive", "g_beam", "beam_pingpong", "seq_last"), ("irs_beam_search",), kind="fresh"),
    Probe("beam_until", "S", _beam("beam", True), _DEC_W + ("arrive", "un_count", "beam_pingpong", "until_pingpong"),
          _DEC_R + ("arrive", "un_count", "beam_pingpong", "until_pingpong"), ("irs_beam_search_until",), kind="fresh"),
    Probe("greedy_b8_bound", "S", _greedy("s8", P_GREEDY, exclude="excl8", no_repeat=True, exact_candidates=True, trace=True, arrive_rank=3),
          _DEC_W + ("arrive", "step_pair", "surv_rows", "g_greedy", "g_beam"), _DEC_R + ("arrive", "step_pair"),
          ("irs_generate_paths", "irs_bind_exclusions"), kind="fresh"),
    Probe("replay_b8", "S", _replay("s8"), _DEC_W, _DEC_R, ("irs_replay_paths",), kind="fresh"),
    # ---- training side
    Probe("ce_m8_finalize", "S", _ce("rows8", "ce_labels"), ("proj_stale", "thr", "g_greedy", "g_beam"), (),
          ("irs_ce_forward", "irs_finalize_weights"), kind="fresh"),
    Probe("train_b4", "S", _train(), (), (), ("irs_train_forward", "irs_train_backward"), kind="fresh"),
]


# ------------------------------------------------------------------------------------------------------------- engine L
def l_inputs(rows_fn, seed: int = 0) -> Dict[str, np.ndarray]:
    """rows_fn = tests/test_gpu_scoring.py:_rows (M, d, seed) -> float32 [M, d]."""
    inp: Dict[str, np.ndarray] = {}
    for name, M, s in (("m5", 5, 1), ("m288", 288, 2), ("m33", 33, 3), ("m9", 9, 4), ("m70l", 70, 6), ("m32", 32, 7), ("m70", 70, 5),
                       ("m5x", 5, 8), ("m10", 10, 9), ("m3", 3, 10)):
        inp[name] = rows_fn(M, D, s + 1000 * seed)
    g = np.random.default_rng(70 + D + seed)
    inp["m70_later"] = (inp["m70"] + 0.02 * g.standard_normal(inp["m70"].shape)).astype(np.float32)
    inp["m70_x4"] = (4.0 * rows_fn(70, D, 97 + 1000 * seed)).astype(np.float32)  # fb_high of test_carried_emission_thresholds_stay_exact
    inp["l_ids"] = g.integers(0, L_ITEMS, size=(10, 5)).astype(np.int64)
    inp["l_labels"] = g.integers(0, L_ITEMS, size=10).astype(np.int64)
    hist = g.integers(0, L_ITEMS, size=(10, 23)).astype(np.int64)
    hist[:, 3], hist[:, 5] = hist[:, 4], -1
    inp["l_hist"] = hist
    return inp


def _lse(rows: str):
    def run(env):
        return env.eng.score_lse(env.inp[rows])
    return run


def _dense(rows: str):
    def run(env):
        return (env.eng.score_dense(env.inp[rows]),)
    return run


_SW_W, _SW_R = ("cand_cnt", "fb_count"), ("cand_cnt", "fb_count")

L_PROBES: List[Probe] = [
    Probe("l_topk_bf16_m5", "L", _topk("m5"), _SW_W + ("thr",), _SW_R, ("irs_score_topk",), kind="topk"),           # streaming form
    Probe("l_topk_bf16_m288", "L", _topk("m288"), _SW_W + ("thr",), _SW_R, ("irs_score_topk",), kind="topk"),       # ring form
    Probe("l_topk_f32_m33", "L", _topk("m33", sweep=IRS_SWEEP_F32), _SW_W, _SW_R, ("irs_score_topk",), kind="topk"),
    Probe("l_topk_lse_m9", "L", _topk_lse("m9"), _SW_W, _SW_R, ("irs_score_topk_lse",), kind="topk_lse"),           # per-wave ring LSE
    Probe("l_topk_lse_m70", "L", _topk_lse("m70l"), _SW_W, _SW_R, ("irs_score_topk_lse",), kind="topk_lse"),        # register form
    Probe("l_lse_m32", "L", _lse("m32"), (), (), ("irs_score_lse",), kind="lse"),
    Probe("l_topk_plain_m70", "L", _topk("m70"), _SW_W + ("thr",), _SW_R, ("irs_score_topk",), kind="topk"),        # sets the thresholds
    Probe("l_carry_reuse_m70", "L", _topk("m70_later", carry=True), _SW_W + ("thr",), _SW_R + ("thr",), ("irs_score_topk_carry",),
          mask_fallback=(2,), kind="topk"),
    Probe("l_carry_x4_m70", "L", _topk("m70_x4", carry=True), _SW_W + ("thr",), _SW_R + ("thr",), ("irs_score_topk_carry",),
          mask_fallback=(2,), kind="topk"),
    Probe("l_exhaustive_m5", "L", _topk("m5x", sweep=IRS_SWEEP_EXHAUSTIVE), (), (), ("irs_score_topk",), kind="topk"),
    Probe("l_gather_count_m10", "L", _gather_count("m10", "l_ids", "l_labels", "l_hist"), (), (),
          ("irs_score_gather", "irs_score_count_before"), kind="count"),
    Probe("l_dense_m3", "L", _dense("m3"), (), (), ("irs_score_dense",), kind="dense"),
]

PROBES = {"S": S_PROBES, "L": L_PROBES}
BY_ID = {p.id: p for p in S_PROBES + L_PROBES}
assert len(BY_ID) == len(S_PROBES) + len(L_PROBES), "duplicate probe ids"

# Exported functions that take `void *stream` and that no probe reaches, with the reason.
_STATELESS = "reads and writes caller buffers only (no workspace, no context state); its own module holds it against a reference: "
NOT_PROBED = {
    "irs_pif": _STATELESS + "tests/test_gpu_decoder_path.py (every decode probe computes the same factor through want_r_u)",
    "irs_ce_grad_logits": "the chunked training route; marks the catalog stale exactly as irs_ce_forward, which is probed "
                          "(tests/test_gpu_training.py)",
    "irs_ce_backward": "works in a caller scratch, no workspace (tests/test_gpu_ce_backward.py); irs_ce_forward is the probe of proj_stale",
    "irs_merge_topk": _STATELESS + "tests/test_gpu_scoring.py, tests/test_gpu_path_kernels.py",
    "irs_pack_topk": _STATELESS + "tests/test_gpu_path_kernels.py",
    "irs_merge_topk_keys": _STATELESS + "tests/test_gpu_path_kernels.py",
    "irs_build_eval_batch": _STATELESS + "tests/test_gpu_frontend.py, tests/test_gpu_path_kernels.py",
    "irs_path_step": "one step on caller buffers; the GPU module calls it on a fresh engine for the composition the greedy probes must "
                     "equal (tests/test_gpu_path_kernels.py)",
    "irs_beam_step": _STATELESS + "tests/test_gpu_path_kernels.py; the beam probes run it inside their loops",
    "irs_beam_step_until": _STATELESS + "tests/test_gpu_beam_until.py; the beam_until probe runs it inside its loop",
    "irs_topk_ensure_survivors": "works in a caller scratch (tests/test_gpu_survivors.py); greedy_b8_bound runs the pass inside its loop",
    "irs_score_target_trace": "works in a caller scratch (tests/test_gpu_path_trace.py); greedy_b8_bound runs the sweep inside its loop",
    "irs_bind_guide": "the held-binding test of the GPU module binds and unbinds it around the plain probe (tests/test_gpu_guided.py)",
    "irs_arrival_offer": _STATELESS + "tests/test_gpu_arrival.py; greedy_b8_bound runs the rule inside its loop",
    "irs_replay_windows": _STATELESS + "tests/test_gpu_replay.py; replay_b8 builds the same windows inside irs_replay_paths",
    "irs_allgather_rows": "sharded / RCCL: one GPU here (tests/test_gpu_comm.py, tests/test_gpu_multirank.py)",
    "irs_exchange_topk": "sharded / RCCL: one GPU here (tests/test_gpu_comm.py, tests/test_gpu_multirank.py)",
    "irs_generate_paths_sharded": "sharded / RCCL: one GPU here (tests/test_gpu_comm.py, tests/test_gpu_multirank.py)",
    "irs_beam_search_sharded": "sharded / RCCL: one GPU here (tests/test_gpu_comm.py, tests/test_gpu_multirank.py)",
    "irs_ce_forward_sharded": "sharded / RCCL: one GPU here (tests/test_gpu_ce_sharded.py)",
    "irs_ce_backward_sharded": "sharded / RCCL: one GPU here (tests/test_gpu_ce_sharded.py)",
}


def stream_functions(header_text: str) -> List[str]:
    """The exported functions of include/irs_hip.h whose declaration takes `void *stream`."""
    txt = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(irs_[a-z_0-9]+)\s*\(([^;{}]*?)\)\s*;", txt, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return sorted(set(out))


# ---------------------------------------------------------------------------------------------------------------- schedules
def all_pairs(probes: Sequence[Probe], seed: int = 0) -> List[Probe]:
    """A closed walk over the complete directed graph with loops on `probes`: every ordered pair (A, then B), A -> A included,
    is adjacent exactly once, n * n + 1 entries (an Euler circuit, Hierholzer's algorithm; the seed orders each node's edges)."""
    n = len(probes)
    g = np.random.default_rng(seed)
    out_edges = [list(g.permutation(n)) for _ in range(n)]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(int(out_edges[v].pop()))
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1]
    return [probes[v] for v in walk]


def shuffled(probes: Sequence[Probe], seed: int, times: int = 3) -> List[Probe]:
    """`times` seeded permutations of the probes, one after the other."""
    g = np.random.default_rng(seed)
    return [probes[int(v)] for _ in range(times) for v in g.permutation(len(probes))]
