"""-m gpu: one engine, any call order, any stream -- results equal a fresh engine's (tests/engine_state_cases.py).

Every entry point has its own module against a reference; this module's subject is the state a context keeps between calls: the
self-resetting device counters, the host fields that describe device buffers, the three captured-step caches, the plan tables and
activations one shape leaves behind for the next.  The expected value of a probe is the same call on a FRESH engine that has made
no other call; it is computed once per module, checked against the references of the entry point's own module (the CPU oracle, the
exhaustive kernel, float64 decodes, the composition of public calls), and shown to be reproducible bit for bit on a second fresh
engine, which is what makes bit equality a fair demand.

Bars.  Integers (ids, ranks, paths, status words, counts) equal; floats bit-equal to the fresh engine's.  The one exception is bit
0, IRS_ROW_FALLBACK, of the two carry=True probes: include/irs_hip.h says it may depend on the previous call.  Against the
references: the bars of tests/test_gpu_scoring.py (ids and value bits exact, 4e-6 on max + log sum) and of
tests/test_gpu_decoder_routes.py (_max_bar over X_TOL / X_TOL_X6), imported, not restated.

Wall times of one MI355X run are in the pull request that added the module; nothing here asserts a time."""
import numpy as np
import pytest
import torch

import decoder_route_cases as RC
import engine_state_cases as E
from gpu_util import make_engine, scoring_only_engines, upload_state_dict
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_ROW_FALLBACK, IRS_ROW_OFFERED, IRS_ROW_RESCUED, IRS_SWEEP_BF16, IRS_SWEEP_EXHAUSTIVE
from influentialrs_amd.engine import _ptr
from test_gpu_decoder_path import X_TOL, X_TOL_X6
from test_gpu_decoder_routes import _max_bar, _sample
from test_gpu_scoring import _rows, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED_S, SEED_TWIN = 2027, 2028
LSE_TOL = 4e-6  # tests/test_gpu_scoring.py: max + log(sum) against the oracle


class Env:
    """One engine with the inputs its probes read (shared, never written) and the buffers a probe holds across calls."""

    def __init__(self, eng, inp):
        self.eng, self.inp, self.held, self.route = eng, inp, {}, None


# ---------------------------------------------------------------------------------------------------------------- engines, inputs
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_module_s_device_memory():
    """The shared weights, inputs and expected values (about 1 GB with engine L's catalog) live for this module only."""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sd_np(seed):
    return _cached(("sd", seed), lambda: synth.irn_state_dict(E.s_config(), seed))


def _fresh(kind, seed=SEED_S):
    """A new engine: context, workspace and derived weights of its own; the bound weights are shared device tensors."""
    if kind == "S":
        sd = _cached(("sd_dev", seed), lambda: upload_state_dict(_sd_np(seed), DEV))
        return make_engine(E.s_config(), sd, max_rows=E.S_ROWS, max_seqs=E.S_ROWS, max_k=E.K, device=DEV)
    W, b = _l_weights()
    return _cached("l_factory", lambda: scoring_only_engines(E.L_ITEMS, E.D, W, b, max_rows=E.L_ROWS, max_k=E.K, device=DEV))()


def _l_weights():
    return _cached("l_weights", lambda: _weights(E.L_ITEMS, E.D, E.L_ITEMS + E.D))


def _up(inp_np):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in inp_np.items()}


def _inputs_np(kind, oracle):
    if kind == "L":
        return _cached("inp_np_L", lambda: E.l_inputs(_rows))
    return _cached("inp_np_S", lambda: E.s_inputs(0, until=E.until_windows(oracle, _sd_np(SEED_S), E.s_config())))


# ---------------------------------------------------------------------------------------------------------------- comparison
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _diff(p, got, want):
    """None, or where the outputs of probe p differ from the expected ones (device comparisons; the first differing row)."""
    if len(got) != len(want):
        return f"{len(got)} outputs, expected {len(want)}"
    for j, (g, w) in enumerate(zip(got, want)):
        if not torch.is_tensor(w):
            if g != w:
                return f"output {j}: {g} != {w}"
            continue
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"output {j}: {tuple(g.shape)} {g.dtype}, expected {tuple(w.shape)} {w.dtype}"
        if j in p.mask_fallback:
            g, w = g & ~IRS_ROW_FALLBACK, w & ~IRS_ROW_FALLBACK
        g, w = _bits(g), _bits(w)
        if not torch.equal(g, w):
            ne = (g != w).reshape(g.shape[0], -1)
            row = int(ne.any(1).nonzero()[0])
            return f"output {j} differs first at row {row} ({int(ne.sum())} of {ne.numel()} words, {int(ne.any(1).sum())} rows)"
    return None


def _call(env, p):
    env.route = None
    got = p.run(env)
    if p.route is not None:
        want = RC.BY_ID[p.route].route
        assert env.route == want, (p.id, {k: (env.route[k], want[k]) for k in want if env.route[k] != want[k]})
    return got


def _run(env, schedule, want, before=None, defer=False):
    """Runs the schedule on env.  defer: returns the outputs for _settle() instead of comparing after every call."""
    outs, trail = [], []
    for n, p in enumerate(schedule):
        if before is not None:
            before()
        got = _call(env, p)
        if defer:
            outs.append((n, p, tuple(trail), got))
        else:
            _settle([(n, p, tuple(trail), got)], want)
        trail = (trail + [p.id])[-TRAIL:]
    return outs


TRAIL = 6  # calls named in a failure: the predecessor first, then the ones before it (the state may be older than one call)


def _settle(outs, want):
    for n, p, trail, got in outs:
        d = _diff(p, got, want[p.id])
        if d is not None:
            after = f"{trail[-1]} (before that, latest first: {', '.join(reversed(trail[:-1])) or 'nothing'})" if trail else \
                "nothing (a fresh engine)"
            raise AssertionError(f"call {n}: probe {p.id} after {after}: {d}")


# ---------------------------------------------------------------------------------------------------------------- expected values
def _baseline(kind, seed, inp, p):
    """Probe p on a fresh engine that makes no other call."""
    env = Env(_fresh(kind, seed), inp)
    got = _call(env, p)
    torch.cuda.synchronize()
    del env
    return got


def _expected(kind, oracle, seed=SEED_S, twice=False):
    """(inputs on the device, {probe id: outputs of a fresh engine}); twice: every baseline on a second fresh engine too, and the
    list of probes whose two runs differ."""
    key = ("exp", kind, seed)
    if key not in _CACHE:
        inp = _up(_inputs_np(kind, oracle))
        want = {}
        if kind == "S":  # the plain probe first: two other probes take their inputs from its result
            plain = E.BY_ID["greedy_b8"]
            want[plain.id] = _baseline(kind, seed, inp, plain)
            paths = want[plain.id][0]
            inp["excl8"] = inp["excl8"].clone()
            inp["excl8"][:, 0] = paths[:, 0].long() - 1  # step 0's chosen item, 0-based
            inp["replay_paths"] = paths.long().contiguous()
            ru, rs = E.replay_rows()
            inp["replay_ru"], inp["replay_rs"] = torch.from_numpy(ru).to(DEV), torch.from_numpy(rs).to(DEV)
        for p in E.PROBES[kind]:
            if p.id not in want:
                want[p.id] = _baseline(kind, seed, inp, p)
        _CACHE[key] = (inp, want, None)
    inp, want, unequal = _CACHE[key]
    if twice and unequal is None:
        unequal = []
        for p in E.PROBES[kind]:
            d = _diff(p, _baseline(kind, seed, inp, p), want[p.id])
            if d is not None:
                unequal.append((p.id, d))
        _CACHE[key] = (inp, want, unequal)
    return inp, want, unequal


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else t


def _rows3(M):
    return sorted({0, M // 2, M - 1})


def _check_topk(oracle, x, W, b, val, ids, rows, k=E.K):
    out = {}
    for m in rows:
        s = out[m] = oracle.score_chain(x[m], W, b)
        ov, oi = oracle.topk(s, k)
        assert np.array_equal(ids[m], oi), f"row {m}: ids differ from the oracle"
        assert np.array_equal(val[m].view(np.uint32), ov.view(np.uint32)), f"row {m}: value bits differ from the oracle"
    return out


def _check_lse(oracle, scores, mx, sm):
    for m, s in scores.items():
        om, osum = oracle.max_sumexp(s)
        assert abs(mx[m] - om) <= LSE_TOL * max(1.0, abs(om)), m
        assert abs((mx[m] + np.log(sm[m])) - (om + np.log(osum))) <= LSE_TOL * max(1.0, abs(om)), m


def _composition(eng, inp, name, P):
    """The greedy loop out of public calls: decode, score_topk (carried after step 0), path_step."""
    seq, hep, usr = inp[f"{name}_seq"].clone(), inp[f"{name}_hep"].clone(), inp[f"{name}_usr"]
    paths = torch.zeros((seq.shape[0], P), dtype=torch.float32, device=DEV)
    status = torch.zeros(seq.shape[0], dtype=torch.int32, device=DEV)
    for i in range(P):
        _, xr, _ = eng.decode(seq, usr, want_x=False, pos=hep)
        val, ids, _ = eng.score_topk(xr, E.K, IRS_SWEEP_BF16, carry=i > 0)
        eng.path_step(seq, hep, val, ids, i, paths, status)
    return paths, status, seq, hep


def _check_decode(oracle, p, inp_np, want, memo):
    cfg, sd, c = E.s_config(), _sd_np(SEED_S), p.case
    B = c.B
    seqs, users, pos = (inp_np[f"win{B}_{k}"] for k in ("seq", "usr", "pos"))
    out = [_host(t) for t in want]
    x, xr, ru = (out if len(out) == 3 else [None] + out)
    U = sd["user_embedder.weight"].astype(np.float64)[users]
    ref_ru = U @ sd["user_mask_layer.weight"][0].astype(np.float64) + np.float64(sd["user_mask_layer.bias"][0])
    assert np.abs(ru - ref_ru).max() < 1e-6, p.id
    bar = _max_bar(c, cfg)
    assert bar in (X_TOL, X_TOL_X6), (p.id, bar)  # (d = 128: the two bars of tests/test_gpu_decoder_path.py, unscaled)
    worst = 0.0
    for b in _sample(B, [int(e) for e in inp_np[f"win{B}_edges"]], seed=1000 + B):
        key = (B, b)
        if key not in memo:
            memo[key] = oracle.decode(sd, cfg, seqs[b], int(users[b]), dtype=np.float64)[0]
        o64 = memo[key]
        got, ref = (x[b], o64) if x is not None else (xr[b], o64[pos[b]])
        if x is not None:
            assert np.array_equal(xr[b].view(np.uint32), x[b, pos[b]].view(np.uint32)), (p.id, b)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (p.id, b)
        fin = np.isfinite(ref)
        if fin.any():
            worst = max(worst, float(np.abs(got - ref)[fin].max()))
    assert 0.0 < worst < bar, (p.id, worst, bar)


@pytest.mark.parametrize("kind", ["S", "L"])
def test_expected_values_are_reproducible_and_match_their_references(oracle, kind):
    """The fresh-engine values every other test compares with: each probe on two fresh engines gives the same bits, and the values
    are right by the reference of the entry point's own module."""
    inp, want, unequal = _expected(kind, oracle, twice=True)
    assert not unequal, f"not reproducible on a second fresh engine: {unequal}"
    inp_np = _inputs_np(kind, oracle)
    if kind == "L":
        W, b = _l_weights()
        exh = _fresh("L")  # a second engine: the exhaustive kernel over every row of every top-k probe
        for p in E.L_PROBES:
            out = [_host(t) for t in want[p.id]]
            if p.kind in ("topk", "topk_lse"):
                rows = {"l_topk_bf16_m5": "m5", "l_topk_bf16_m288": "m288", "l_topk_f32_m33": "m33", "l_topk_lse_m9": "m9",
                        "l_topk_lse_m70": "m70l", "l_topk_plain_m70": "m70", "l_carry_reuse_m70": "m70_later", "l_carry_x4_m70": "m70_x4",
                        "l_exhaustive_m5": "m5x"}[p.id]
                ev, ei, _ = exh.score_topk(inp[rows], E.K, IRS_SWEEP_EXHAUSTIVE)
                assert torch.equal(want[p.id][1], ei) and torch.equal(_bits(want[p.id][0]), _bits(ev)), p.id
                x = inp_np[rows]
                scores = _check_topk(oracle, x, W, b, out[0], out[1], _rows3(x.shape[0]))
                if p.kind == "topk_lse":
                    _check_lse(oracle, scores, out[3], out[4])
                if not p.mask_fallback and p.id != "l_exhaustive_m5":
                    assert not (out[2] & IRS_ROW_FALLBACK).any(), p.id  # benign rows on a fresh engine
            elif p.kind == "lse":
                x = inp_np["m32"]
                _check_lse(oracle, {m: oracle.score_chain(x[m], W, b) for m in _rows3(32)}, out[0], out[1])
            elif p.kind == "dense":
                x = inp_np["m3"]
                for m in range(3):
                    assert np.array_equal(out[0][m].view(np.uint32), oracle.score_chain(x[m], W, b).view(np.uint32)), m
            elif p.kind == "count":
                x, ids, labels, hist = (inp_np[k] for k in ("m10", "l_ids", "l_labels", "l_hist"))
                for m in _rows3(10):
                    s = oracle.score_chain(x[m], W, b)
                    assert np.array_equal(out[0][m].view(np.uint32), s[ids[m]].view(np.uint32)) and out[1][m] == s[labels[m]]
                    assert out[2][m] + 1 == oracle.rank_of(s, int(labels[m]), hist[m][hist[m] >= 0]), m
            else:
                raise AssertionError(p.kind)
        # the big catalog makes the carried thresholds and the cooperative fallback exist: the x4 rows overflow their buckets
        # once thresholds are carried (the second call of a pair; a fresh engine has none to carry)
        env = Env(exh, inp)
        _call(env, E.BY_ID["l_topk_plain_m70"])
        st = _call(env, E.BY_ID["l_carry_x4_m70"])[2]
        assert int((st & IRS_ROW_FALLBACK).sum()) > 0, "the x4 rows should push rows onto the exhaustive path behind carried thresholds"
        return
    cfg, sd = E.s_config(), _sd_np(SEED_S)
    W, b = sd["project.weight"], sd["project.bias"]
    memo = {}
    for p in E.S_PROBES:
        if p.kind == "decode":
            _check_decode(oracle, p, inp_np, want[p.id], memo)
        elif p.kind == "greedy":
            name, P = ("s8", E.P_GREEDY) if p.id == "greedy_b8" else ("s70", E.P_G70)
            comp = _composition(_fresh("S"), inp, name, P)
            d = _diff(p, comp, want[p.id])
            assert d is None, f"{p.id} against the composition of decode, score_topk and path_step: {d}"
    for pid, rows in (("topk_m8", "rows8"), ("topk_m70", "rows70"), ("topk_lse_m8", "rows8b")):
        out = [_host(t) for t in want[pid]]
        x = inp_np[rows]
        scores = _check_topk(oracle, x, W, b, out[0], out[1], _rows3(x.shape[0]))
        assert not out[2].any(), pid
        if pid == "topk_lse_m8":
            _check_lse(oracle, scores, out[3], out[4])
    # the graph form of the plain probe is the plain probe
    assert _diff(E.BY_ID["greedy_b8"], want["greedy_b8_graph"], want["greedy_b8"]) is None
    # the stop-at-target probe: at least two and not all users arrive before the last step, so the compaction runs
    paths, _, steps, _ = (_host(t) for t in want["until_b8"])
    tg = inp_np["until_seq"][:, -1]
    early = [(paths[u, :E.P_UNTIL - 1] == tg[u]).any() for u in range(8)]
    assert 2 <= sum(early) < 8 and steps == E.P_UNTIL, (early, steps)
    # every binding of the bound probe left its mark: the excluded step-0 item is gone, a trace was written
    bound, plain = [_host(t) for t in want["greedy_b8_bound"]], [_host(t) for t in want["greedy_b8"]]
    assert (bound[0][:, 0] != plain[0][:, 0]).all() and (bound[4] < 0).all() and (bound[6] >= 1).all()
    # the training probe: finite, non-zero gradients (its reference tests are tests/test_gpu_train_trunk.py)
    x, grads = (_host(t) for t in want["train_b4"])
    assert np.isfinite(grads).all() and np.abs(grads).max() > 0


# ---------------------------------------------------------------------------------------------------------------- 1. every pair
@pytest.mark.parametrize("kind", ["S", "L"])
def test_every_ordered_pair_on_one_engine(oracle, kind):
    """all_pairs on ONE engine: every probe after every probe, itself included, equals the fresh engine's value."""
    inp, want, _ = _expected(kind, oracle)
    env = Env(_fresh(kind), inp)
    _run(env, E.all_pairs(E.PROBES[kind], seed=0), want)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2. a side stream
def _busy_default_stream():
    """A matmul on the default stream, sized once to a millisecond or two (not asserted): work the library wrongly put on the
    null stream, or on a stream of its own that it does not join back, queues behind it and shows as a wrong value."""
    n = 2048
    while True:
        a = torch.randn((n, n), device=DEV)
        c = torch.empty_like(a)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(a, a, out=c)
        t0.record()
        torch.mm(a, a, out=c)
        t1.record()
        t1.synchronize()
        if t0.elapsed_time(t1) >= 1.0 or n >= 8192:
            break
        n *= 2
    default = torch.cuda.default_stream(torch.device(DEV))

    def enqueue():
        with torch.cuda.stream(default):
            torch.mm(a, a, out=c)
    return enqueue


@pytest.mark.parametrize("kind", ["S", "L"])
def test_side_stream_with_a_busy_default_stream(oracle, kind):
    """Three shuffled rounds on a stream that is not the default one, the default stream kept busy before every probe; results
    are read only after the side stream has drained."""
    inp, want, _ = _expected(kind, oracle)
    env = Env(_fresh(kind), inp)
    busy = _busy_default_stream()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.default_stream(torch.device(DEV)))
    with torch.cuda.stream(side):
        outs = _run(env, E.shuffled(E.PROBES[kind], seed=11, times=3), want, before=busy, defer=True)
    side.synchronize()
    _settle(outs, want)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 3. re-binding
@pytest.mark.parametrize("kind", ["S", "L"])
def test_rebinding_a_used_or_filled_workspace(oracle, kind):
    """irs_bind_workspace on memory that is not fresh: the same workspace after use, filled (a) with zero bytes and (b) with the
    32-bit word 1 -- a wrong counter and a wrong but in-range index, so that a read of a never-written word gives a wrong result,
    never an address out of range."""
    inp, want, _ = _expected(kind, oracle)
    env = Env(_fresh(kind), inp)
    eng = env.eng
    _run(env, E.shuffled(E.PROBES[kind], seed=3, times=1), want)
    for word in (0, 1):
        torch.cuda.synchronize()
        ws = eng._ws
        ws.zero_()
        if word:
            ws[:ws.numel() // 4 * 4].view(torch.int32).fill_(word)
        torch.cuda.synchronize()
        eng._check(eng.lib.irs_bind_workspace(eng.h, _ptr(ws), ws.numel()))
        _run(env, E.shuffled(E.PROBES[kind], seed=20 + word, times=2), want)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 4. two engines
def test_two_engines_alternate_and_overlap(oracle):
    """Engine S and a twin on other weights (seed 2028): call by call on one stream, then each on a stream of its own with no
    synchronisation between the two inside the schedule.  Each engine's results equal its own fresh-engine values."""
    inp_a, want_a, _ = _expected("S", oracle)
    inp_b, want_b, _ = _expected("S", oracle, seed=SEED_TWIN)
    assert not torch.equal(want_a["greedy_b8"][0], want_b["greedy_b8"][0])  # (other weights: other paths)
    a, b = Env(_fresh("S"), inp_a), Env(_fresh("S", SEED_TWIN), inp_b)
    sched_a, sched_b = E.shuffled(E.S_PROBES, seed=31, times=2), E.shuffled(E.S_PROBES, seed=32, times=2)
    trail_a, trail_b = [], []
    for n, (pa, pb) in enumerate(zip(sched_a[:len(E.S_PROBES)], sched_b[:len(E.S_PROBES)])):
        _settle([(n, pa, tuple(trail_a), _call(a, pa))], want_a)
        _settle([(n, pb, tuple(trail_b), _call(b, pb))], want_b)
        trail_a, trail_b = (trail_a + [pa.id])[-TRAIL:], (trail_b + [pb.id])[-TRAIL:]
    default = torch.cuda.default_stream(torch.device(DEV))
    sa, sb = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    sa.wait_stream(default)
    sb.wait_stream(default)
    outs_a, outs_b = [], []
    for n, (pa, pb) in enumerate(zip(sched_a[len(E.S_PROBES):], sched_b[len(E.S_PROBES):])):
        with torch.cuda.stream(sa):
            outs_a.append((n, pa, tuple(trail_a), _call(a, pa)))
        with torch.cuda.stream(sb):
            outs_b.append((n, pb, tuple(trail_b), _call(b, pb)))
        trail_a, trail_b = (trail_a + [pa.id])[-TRAIL:], (trail_b + [pb.id])[-TRAIL:]
    sa.synchronize()
    sb.synchronize()
    _settle(outs_a, want_a)
    _settle(outs_b, want_b)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 5. held bindings
def _g8(env, graph, k=E.K, **kw):
    """The plain B = 8 search (the greedy_b8 probe's inputs) on plain stream launches, or as a captured step on held buffers."""
    i = env.inp
    if not graph:
        seq, hep = i["s8_seq"].clone(), i["s8_hep"].clone()
        out = env.eng.generate_paths(seq, i["s8_usr"], hep, E.P_GREEDY, k=k, **kw)
        return out[0], out[1], seq, hep
    if "g8" not in env.held:
        env.held["g8"] = (torch.empty_like(i["s8_seq"]), torch.empty_like(i["s8_hep"]),
                          torch.empty((8, E.P_GREEDY), dtype=torch.float32, device=DEV), torch.empty_like(i["s8_hep"]))
    seq, hep, paths, status = env.held["g8"]
    seq.copy_(i["s8_seq"])
    hep.copy_(i["s8_hep"])
    paths.zero_()
    status.zero_()
    env.eng.generate_paths(seq, i["s8_usr"], hep, E.P_GREEDY, k=k, use_graph=True, paths=paths, status=status, **kw)
    return paths.clone(), status.clone(), seq.clone(), hep.clone()


def test_a_held_binding_changes_the_plain_probe_and_unbinding_restores_it(oracle):
    """Sensitivity, through the public API: a binding that is held changes the plain B = 8 search -- graph and no graph, the
    captured form following every time -- to what the same binding gives on a fresh engine, and unbinding restores the plain
    value.  A trace bound a second time, to other arrays, is followed too: no option is part of the captured step's key, every
    bind and unbind drops the captured steps.  (No getter reports the single-device caches: the results are the evidence.)"""
    inp, want, _ = _expected("S", oracle)
    plain_p = E.BY_ID["greedy_b8"]
    plain = want["greedy_b8"]
    cfg = E.s_config()
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    table = torch.randint(0, 2, (cfg.n_item + 1, 24), generator=g, device=DEV, dtype=torch.uint8)
    RANK = 1500  # an arrival rule that fires for random targets (the bound probe of the schedules uses rank 3)

    def fresh(k=E.K, **kw):
        out = _g8(Env(_fresh("S"), inp), False, k=k, **kw)
        torch.cuda.synchronize()
        return out

    exp_excl = fresh(exclude=inp["excl8"])
    exp_guide = fresh(guide=table, guide_k=5)
    f = Env(_fresh("S"), inp)
    seq, hep = inp["s8_seq"].clone(), inp["s8_hep"].clone()
    tr = f.eng.generate_paths(seq, inp["s8_usr"], hep, E.P_GREEDY, k=E.K, trace=True, arrive_rank=RANK)
    exp_trace = (tr[0], tr[1], seq, hep)
    exp_trace_arrays = tuple(t.clone() for t in tr[2])
    torch.cuda.synchronize()
    exp_k1_plain, exp_k1_exact = fresh(k=1), fresh(k=1, exact_candidates=True)
    KC = 5
    f = Env(_fresh("S"), inp)
    seq, hep = inp["s8_seq"].clone(), inp["s8_hep"].clone()
    lk = f.eng.generate_paths(seq, inp["s8_usr"], hep, E.P_GREEDY, k=E.K, lookahead=KC, lookahead_record=True)
    exp_look = (lk[0], lk[1], seq, hep)
    exp_look_record = tuple(t.clone() for t in lk[2])
    torch.cuda.synchronize()
    # each binding matters on these inputs
    assert (exp_excl[0][:, 0] != plain[0][:, 0]).all()                       # the lists hold step 0's chosen item
    assert not torch.equal(exp_guide[0], plain[0])
    assert int((exp_trace[1] & IRS_ROW_OFFERED).ne(0).sum()) > 0 and not torch.equal(exp_trace[0], plain[0])
    assert int((exp_k1_exact[1] & IRS_ROW_RESCUED).ne(0).sum()) > 0 and not torch.equal(exp_k1_exact[0], exp_k1_plain[0])
    assert not torch.equal(exp_look[0], plain[0])

    env = Env(_fresh("S"), inp)
    eng = env.eng

    def rounds(expect, k=E.K, extra=None):
        for graph in (True, False, True):
            d = _diff(plain_p, _g8(env, graph, k=k), expect)
            assert d is None, f"graph={graph}: {d}"
            if extra is not None:
                extra()

    rounds(plain)
    # ---- exclusions
    scratch = eng.bind_exclusions(inp["excl8"])
    rounds(exp_excl)
    eng.unbind_exclusions()
    rounds(plain)
    del scratch
    # ---- guide
    eng.bind_guide(table, 5)
    rounds(exp_guide)
    eng.unbind_guide()
    rounds(plain)
    # ---- lookahead, with its record
    record = eng.bind_lookahead(KC, 8, E.P_GREEDY, record=True)

    def record_written():
        for got, exp in zip(record, exp_look_record):
            assert torch.equal(_bits(got), _bits(exp))
            got.zero_()
    rounds(exp_look, extra=record_written)
    torch.cuda.synchronize()
    eng.unbind_lookahead()
    rounds(plain)
    assert not any(bool(t.any()) for t in record)  # (unbound: nothing writes the record any more)
    # ---- path trace + arrival rule
    arrays = eng.bind_path_trace(8, E.P_GREEDY)
    eng.set_arrival_rule(rank_max=RANK)

    def trace_written(arrays=arrays):
        for got, exp in zip(arrays[:3], exp_trace_arrays):
            assert torch.equal(_bits(got), _bits(exp))
            got.zero_()
    rounds(exp_trace, extra=trace_written)
    torch.cuda.synchronize()
    # ---- the trace bound again, to fresh arrays (the old ones are held, so the allocator cannot hand them out again), with the
    # step captured under the first binding still the last thing the cache saw: the replay must write the new arrays only
    for t in arrays[:3]:
        t.zero_()
    eng.unbind_path_trace()
    again = eng.bind_path_trace(8, E.P_GREEDY)
    assert not {t.data_ptr() for t in again} & {t.data_ptr() for t in arrays}
    d = _diff(plain_p, _g8(env, True), exp_trace)
    assert d is None, f"rebound trace, graph=True: {d}"
    trace_written(again)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in arrays[:3])
    eng.set_arrival_rule(None, None)
    eng.unbind_path_trace()
    rounds(plain)
    assert not any(bool(t.any()) for t in arrays[:3] + again[:3])  # (unbound: nothing writes the arrays any more)
    # ---- survivor scratch: at k = 1 the one candidate is soon inside the window
    rounds(exp_k1_plain, k=1)
    surv = torch.empty(eng.survivor_scratch_bytes(8, 1), dtype=torch.uint8, device=DEV)
    eng._check(eng.lib.irs_bind_survivor_scratch(eng.h, _ptr(surv), surv.numel()))
    rounds(exp_k1_exact, k=1)
    rounds(plain)  # (k = 100: no window hides a list, the pass changes nothing)
    torch.cuda.synchronize()
    eng._check(eng.lib.irs_bind_survivor_scratch(eng.h, None, 0))
    rounds(exp_k1_plain, k=1)
    rounds(plain)
    torch.cuda.synchronize()
