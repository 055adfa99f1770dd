"""-m gpu: the stop-at-target search (irs_generate_paths_until, Engine.generate_paths_until,
IRSNN.get_seq_in_batch(stop_at_target=True)) against the reference's goldens and against the plain loop.

The reference runs every step for every user and zeroes the tail behind the target on the host
(model/influentialRS.py:459-467); the goldens' `paths` are that result.  The loop under test stops a user after the step
that chose its target, compacts the live users on the device and returns when nobody is left: the paths must be the same
id for id, zeros included, and the counters it returns must show that the work really stopped.

Everything here is integer-exact (ids stored as float32, status words, step counts): there are no tolerances."""
import numpy as np
import pytest
import torch

from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_NO_CANDIDATE, IRS_SWEEP_BF16
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from gpu_util import make_engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENG = {}


def _engine(cfgname, B=32):
    key = (cfgname, B)
    if key not in _ENG:
        _ENG.clear()  # one catalog resident at a time
        cfg = synth.make_config(cfgname)
        _ENG[key] = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=B, max_seqs=B)
    return _ENG[key]


def _inputs(g, src):
    src = np.asarray(src)
    seq = torch.from_numpy(g["seqs"][src]).to(DEV)
    usr = torch.from_numpy(g["users"][src]).to(DEV)
    hep = torch.full((len(src),), g["seqs"].shape[1] - 2, dtype=torch.int32, device=DEV)  # the goldens' gap_len is 0
    return seq, usr, hep


def _until(eng, g, src, check_every, P=None, **kw):
    seq, usr, hep = _inputs(g, src)
    P = int(g["meta"][2]) if P is None else P
    paths, status, steps, row_steps = eng.generate_paths_until(seq, usr, hep, P, k=100, sweep=IRS_SWEEP_BF16,
                                                               check_every=check_every, **kw)
    torch.cuda.synchronize()
    return paths.cpu().numpy(), status.cpu().numpy(), steps, row_steps


def _finish_step(g, u):
    """s_b: the target's position in the golden path, None for a user that never arrives."""
    pos = np.where(g["paths"][u] == g["targets"][u])[0]
    return int(pos[0]) if len(pos) else None


# ---------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("name,cfgname", [("irn_tiny", "tiny"), ("irn_c1", "c1")])
def test_paths_equal_the_reference_goldens(golden, name, cfgname):
    g = golden(name)
    B = g["seqs"].shape[0]
    paths, status, steps, row_steps = _until(_engine(cfgname), g, np.arange(B), 1)
    assert paths.dtype == np.float32 and np.array_equal(paths, g["paths"])
    assert not (status & IRS_ROW_NO_CANDIDATE).any()
    assert sorted(g["early_users"].tolist()) == [u for u in range(B) if _finish_step(g, u) is not None]
    assert steps == int(g["meta"][2]) and row_steps < B * steps  # somebody never arrives, somebody does


@pytest.mark.parametrize("name,cfgname", [("irn_tiny", "tiny"), ("irn_c1", "c1")])
def test_front_end_returns_the_reference_tuple(golden, name, cfgname):
    g = golden(name)
    cfg = synth.make_config(cfgname)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    irn.eval()
    seq, usr, _ = _inputs(g, np.arange(g["seqs"].shape[0]))
    tgt = torch.from_numpy(g["targets"]).to(DEV)
    before = seq.clone()
    P = int(g["meta"][2])
    with torch.no_grad():
        plain = irn.get_seq_in_batch(seq, usr, tgt, P, 0, False, 3)
        paths, tt, hh, early = irn.get_seq_in_batch(seq, usr, tgt, P, 0, False, 3, stop_at_target=True)
    assert np.array_equal(paths, g["paths"]) and paths.dtype == np.float32
    assert early == int(g["n_early_success"]) and early > 0
    assert np.array_equal(tt, g["targets"]) and tt.dtype == np.int64
    assert np.array_equal(paths, plain[0]) and early == plain[3]
    assert all(np.array_equal(a, b) for a, b in zip(hh, plain[2]))
    assert torch.equal(seq, before), "the search works on a clone"


# ---------------------------------------------------------------- 2. the plain search plus the host's zeroing
@pytest.mark.parametrize("name,cfgname", [("irn_tiny", "tiny"), ("irn_c1", "c1")])
def test_same_rows_as_the_plain_search_then_zeroing(golden, name, cfgname):
    g = golden(name)
    B = g["seqs"].shape[0]
    P = int(g["meta"][2])
    eng = _engine(cfgname)
    seq, usr, hep = _inputs(g, np.arange(B))
    ref_t, ref_st = eng.generate_paths(seq, usr, hep, P, k=100, sweep=IRS_SWEEP_BF16)
    torch.cuda.synchronize()
    ref, ref_st = ref_t.cpu().numpy().copy(), ref_st.cpu().numpy()
    never = []
    for b in range(B):  # the reference's zeroing (influentialRS.py:459-467)
        pos = np.where(ref[b] == g["targets"][b])[0]
        if len(pos):
            ref[b, pos[0] + 1:] = 0
        else:
            never.append(b)
    assert never and len(never) < B
    assert not ref_st.any()  # no golden user runs out of candidates in any step, so a finished row's live steps set no bit either
    for check_every in (1, 3, P + 1):
        paths, status, steps, row_steps = _until(eng, g, np.arange(B), check_every)
        assert np.array_equal(paths.view(np.uint32), ref.view(np.uint32)), check_every
        assert np.array_equal(status[never], ref_st[never]), check_every
        assert np.array_equal(status, ref_st), check_every
        if check_every == P + 1:  # never checked: every row in every step
            assert (steps, row_steps) == (P, B * P)


# ---------------------------------------------------------------- 3. the work really stops
def test_steps_and_decoded_rows_stop_with_the_users(golden):
    g = golden("irn_tiny")
    P = int(g["meta"][2])
    eng = _engine("tiny")
    early = [int(u) for u in g["early_users"]]
    s = {u: _finish_step(g, u) for u in early}
    never = [u for u in range(g["seqs"].shape[0]) if _finish_step(g, u) is None][:4]
    # only users that arrive, repeated to 8 rows
    src = (early * 8)[:8]
    paths, _, steps, row_steps = _until(eng, g, src, 1)
    assert np.array_equal(paths, g["paths"][src])
    assert steps == max(s[u] for u in src) + 1 and steps < P
    assert row_steps == sum(s[u] + 1 for u in src)
    # mixed with users that never arrive
    src = early + never
    paths, _, steps, row_steps = _until(eng, g, src, 1)
    assert np.array_equal(paths, g["paths"][src])
    assert steps == P and row_steps == sum(s[u] + 1 for u in early) + P * len(never)
    # one user
    u = early[0]
    paths, _, steps, row_steps = _until(eng, g, [u], 1)
    assert np.array_equal(paths, g["paths"][[u]])
    assert steps == s[u] + 1 and row_steps == s[u] + 1


# ---------------------------------------------------------------- 4. compaction across a decoder route switch
def test_compaction_crosses_the_sequence_resident_threshold(golden):
    """c2 users x 13 = 416 sequences start on the sequence-resident decoder (384 sequences and up); 8 of the 32 golden users
    arrive within four steps, which leaves 312 live sequences: the later steps run on the two-kernel route."""
    g = golden("irn_c2")
    B0 = g["seqs"].shape[0]
    reps = 13
    B = B0 * reps
    P = int(g["meta"][2])
    src = np.random.default_rng(20261018).permutation(np.tile(np.arange(B0), reps))
    eng = _engine("c2", B)
    assert B >= 400 and eng.decoder_seq == 2  # auto: sequence-resident from 384 sequences per call up
    fin = np.array([P if _finish_step(g, u) is None else _finish_step(g, u) for u in src])
    live = [int((fin >= i).sum()) for i in range(P)]  # rows of step i with check_every = 1
    assert live[0] >= 384 > live[-1] > 0, "the golden inputs let the batch fall through the switch"
    _until(eng, g, src, 1, P=1)
    assert eng.decoder_seq_last, "the first step runs the sequence-resident kernel"
    paths, status, steps, row_steps = _until(eng, g, src, 1)
    assert not eng.decoder_seq_last, "the last step runs below the switch"
    assert (steps, row_steps) == (P, sum(live))
    assert not (status & IRS_ROW_NO_CANDIDATE).any()
    assert np.array_equal(paths, g["paths"][src])


# ---------------------------------------------------------------- 5. order of compaction
@pytest.mark.parametrize("check_every", [1, 3])
def test_every_original_row_keeps_its_own_user(golden, check_every):
    g = golden("irn_tiny")
    eng = _engine("tiny")
    e = [int(u) for u in g["early_users"]]
    n = [u for u in range(g["seqs"].shape[0]) if _finish_step(g, u) is None]
    assert len(e) >= 4 and len(n) >= 5
    # arriving users in the first and the last row, alternating in between, then runs of each kind
    src = [e[0], n[0], e[1], n[1], e[2], n[2], e[3], n[3], n[4], e[0], e[1], n[0], n[1], e[3]]
    paths, status, steps, _ = _until(eng, g, src, check_every)
    assert np.array_equal(paths, g["paths"][src])
    assert not status.any() and steps == int(g["meta"][2])
    # ... and with nobody left after a few steps: arriving users only, permuted
    src = [e[3], e[0], e[2], e[1], e[0], e[3]]
    paths, _, steps, _ = _until(eng, g, src, check_every)
    assert np.array_equal(paths, g["paths"][src])
    s_max = max(_finish_step(g, u) for u in src) + 1
    assert steps == min(-(-s_max // check_every) * check_every, int(g["meta"][2]))


# ---------------------------------------------------------------- 6. argument checks
def test_bad_arguments_are_refused_before_any_launch(golden):
    g = golden("irn_tiny")
    B = 4
    cfg = synth.make_config("tiny")
    seq, usr, hep = _inputs(g, np.arange(B))
    seq0, hep0 = seq.clone(), hep.clone()
    paths = torch.full((B, 5), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((B,), 1 << 20, dtype=torch.int32, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return (bool((paths == -7.0).all()) and bool((status == (1 << 20)).all()) and torch.equal(seq, seq0)
                and torch.equal(hep, hep0))

    eng = _engine("tiny")
    with pytest.raises(IrsError, match=r"error -1\b.*check_every"):  # IRS_E_INVALID
        eng.generate_paths_until(seq, usr, hep, 5, check_every=0, paths=paths, status=status)
    assert untouched()
    shard = make_engine(cfg, synth.irn_state_dict(cfg, 1234), max_rows=32, max_seqs=8, rank=0, world=2)
    with pytest.raises(IrsError, match=r"error -4\b.*whole catalog"):  # IRS_E_UNSUPPORTED
        shard.generate_paths_until(seq, usr, hep, 5, check_every=1, paths=paths, status=status)
    assert untouched()


def test_front_end_names_what_is_not_built(golden):
    g = golden("irn_tiny")
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    seq, usr, _ = _inputs(g, np.arange(4))
    tgt = torch.from_numpy(g["targets"][:4]).to(DEV)
    with pytest.raises(ValueError, match="beam"):
        irn.get_seq_in_batch(seq, usr, tgt, 5, 0, beam_width=2, stop_at_target=True)


# ---------------------------------------------------------------- 7. sampled mode
@pytest.mark.parametrize("check_every", [1, 3])
def test_sampled_search_is_deterministic_and_zero_behind_the_target(golden, check_every):
    g = golden("irn_tiny")
    B = g["seqs"].shape[0]
    eng = _engine("tiny")
    runs = [_until(eng, g, np.arange(B), check_every, sample=True, sample_k=3, seed=20261018) for _ in range(2)]
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert np.array_equal(runs[0][1], runs[1][1]) and runs[0][2:] == runs[1][2:]
    other = _until(eng, g, np.arange(B), check_every, sample=True, sample_k=3, seed=7)
    assert not np.array_equal(other[0], runs[0][0]), "12 users x 20 draws among 3 survivors: another seed, other paths"
    paths, _, steps, row_steps = runs[0]
    P = paths.shape[1]
    live_steps = []
    for b in range(B):
        pos = np.where(paths[b] == g["targets"][b])[0]
        if len(pos):
            live_steps.append(int(pos[0]) + 1)
            assert (paths[b, pos[0] + 1:] == 0).all()
            assert (paths[b, :pos[0] + 1] > 0).all()
        else:
            live_steps.append(P)
            assert (paths[b] > 0).all()
    # the counters agree with the paths: a row is decoded until the first check at or behind its last live step
    to_check = [min(-(-n // check_every) * check_every, P) for n in live_steps]
    assert steps == max(to_check) and row_steps == sum(to_check)


# ---------------------------------------------------------------- 8. a pad target, a list that runs out
def test_pad_target_and_exhausted_candidates_match_the_plain_search(golden):
    """Windows whose last slot is the pad id 0, searched with k = 1: the only candidate is often in the window already, so rows
    run out of candidates (IRS_ROW_NO_CANDIDATE, path entry 0).  The host's comparison `path == target` then holds at that
    step, as it does in the reference's zeroing; such a row keeps its window in the plain loop and writes 0 for the rest of
    the search, so stopping it there must give the same row and the same status word."""
    g = golden("irn_tiny")
    B = g["seqs"].shape[0]
    P = int(g["meta"][2])
    eng = _engine("tiny")

    def inputs():
        seq, usr, hep = _inputs(g, np.arange(B))
        seq[:, -1] = 0
        return seq, usr, hep

    seq, usr, hep = inputs()
    ref, ref_st = eng.generate_paths(seq, usr, hep, P, k=1, sweep=IRS_SWEEP_BF16)
    torch.cuda.synchronize()
    ref, ref_st = ref.cpu().numpy().copy(), ref_st.cpu().numpy()
    for b in range(B):
        pos = np.where(ref[b] == 0)[0]
        if len(pos):
            ref[b, pos[0] + 1:] = 0
    out_of_candidates = (ref_st & IRS_ROW_NO_CANDIDATE) != 0
    assert out_of_candidates.any() and not out_of_candidates.all(), "the fixed inputs hold both kinds of row"
    for check_every in (1, 3):
        seq, usr, hep = inputs()
        paths, status, steps, row_steps = eng.generate_paths_until(seq, usr, hep, P, k=1, sweep=IRS_SWEEP_BF16,
                                                                   check_every=check_every)
        torch.cuda.synchronize()
        assert np.array_equal(paths.cpu().numpy().view(np.uint32), ref.view(np.uint32)), check_every
        assert np.array_equal(status.cpu().numpy(), ref_st), check_every
        assert steps == P and row_steps < B * P


def test_harness_passes_stop_at_target_through(golden, tmp_path):
    """harness.test_model with config.stop_at_target = True: the reference pipeline's aggregates and files, unchanged."""
    from influentialrs_amd import harness
    g = golden("harness_tiny")
    n = g["in_users"].shape[0]
    rows = [(g["in_raw"][i, :g["in_raw_len"][i]].copy(), int(g["in_users"][i]), int(g["in_targets"][i]), int(g["in_labels"][i]))
            for i in range(n)]
    cfg = synth.make_config("tiny")
    for k, v in dict(gap_len=0, batch_size=4, top_k=20, use_h=True, max_path_len=int(g["max_path_len"]), sample=False,
                     sample_k=3, stop_at_target=True).items():
        setattr(cfg, k, v)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    irn = IRSNN(cfg, net, DEV)
    seen = []
    inner = irn.get_seq_in_batch
    irn.get_seq_in_batch = lambda *a, **kw: (seen.append(kw), inner(*a, **kw))[1]
    res = harness.test_model(cfg, rows, irn, DEV, result_dir=str(tmp_path), verbose=False)
    assert seen and all(kw == {"stop_at_target": True} for kw in seen)
    assert res["n_early_success"] == int(g["printed"][2])
    assert res["paths"].dtype == np.float32 and np.array_equal(res["paths"], g["paths"])
    assert np.array_equal(res["targets"], g["targets"])
