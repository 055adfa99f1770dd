"""-m gpu: weights that change in place under a live engine -- after irs_finalize_weights a used engine equals a fresh one.

The life cycle the engine is built for is train -> the weights change in place -> re-finalise -> infer.  include/irs_hip.h asks
for irs_finalize_weights "again after any weight changes in place"; this module holds that sentence on every kernel family of
tests/decoder_route_cases.py and tests/long_window_cases.py (the representatives of tests/weight_lifecycle_cases.py), on the
scoring side and through the nn.Module front ends.

A USED engine has already decoded the case's batch and served a top-k, so its workspace, plans and carried state exist.  Weights
change by writes into the tensors the engine holds (eng._weights[name].copy_(...)), followed by eng.finalize().  A FRESH engine
is a new context, workspace and arena bound to new device tensors with the new values.  Packing is deterministic, so every
comparison is BIT equality of a used engine with a fresh one of the same build; no tolerance appears here.  The one number is
the condition ARENA_UNWRITTEN_MAX on the bytes of the arena that finalisation does not write.

What it finds when it fails: a pack launch skipped for one shape class, a vector missing from the sequence-resident kernel's
pack, cross-attention constants or filter norms that are not rebuilt, a float16 range bound that is not re-evaluated, carried
emission thresholds that survive a new catalog, a decode that reads arena bytes no pack wrote."""
import json
import os

import numpy as np
import pytest
import torch

import engine_state_cases as E
import weight_lifecycle_cases as W
from decoder_route_cases import BY_ID, Case
from gpu_util import _scoring_only, make_engine
from parity_record import OUT as PARITY_OUT
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_GEMM_F32, IRS_GEMM_H3, IRS_GEMM_X6, IRS_SWEEP_BF16, IRS_SWEEP_F32
from test_gpu_decoder_routes import _batch
from test_gpu_scoring import _rows, _weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OUT = os.path.join(os.path.dirname(PARITY_OUT), "weight_lifecycle_arena.json")
GEMM = {"h3": IRS_GEMM_H3, "x6": IRS_GEMM_X6, "f32": IRS_GEMM_F32}
SEQ = {0: 0, 1: 1, "auto": None}
K = 100
TOPK_ROWS = 33
_G = {}


# ---------------------------------------------------------------------------------------------------------------- engines
def _up(sd_np):
    """New device tensors with the values of a numpy state dict."""
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in sd_np.items()}


def _new_engine(cfg, sd_dev, *, evaluator=False, max_rows=64, max_seqs=0, attn="h3", poison=None, rank=0, world=1):
    """make_engine on device tensors.  poison: the arena exists before the first finalisation, every byte = poison."""
    return make_engine(cfg, sd_dev, evaluator=evaluator, max_rows=max_rows, max_seqs=max_seqs, rank=rank, world=world, max_k=K,
                       device=DEV, attn=attn, arena_fill=poison)


def _need(eng):
    return int(eng.lib.irs_derived_bytes(eng.h))


def _arena(eng):
    """The derived bytes of an engine, as they are now (a copy)."""
    return eng._arena[:_need(eng)].clone()


class _Group:
    """One engine group: the config, the two state dicts (numpy, and master copies on the device), the used engine."""

    def __init__(self, rep):
        c = rep.case
        self.cfg, self.evaluator, self.attn = c.config(), c.evaluator, c.attn
        self.n = max(W.group_seqs(rep.group()), TOPK_ROWS)
        self.a_np, self.b_np = W.state_dicts(self.cfg, c.evaluator)
        self.a, self.b = _up(self.a_np), _up(self.b_np)
        self.eng = self.fresh(self.a_np)
        self.batches = {}

    def fresh(self, sd_np, poison=None):
        return _new_engine(self.cfg, _up(sd_np), evaluator=self.evaluator, max_rows=self.n, max_seqs=self.n, attn=self.attn,
                           poison=poison)

    def batch(self, c):
        if c.id not in self.batches:
            seqs, users, pos, _ = _batch(c, self.cfg, seed=1000 + c.B)
            self.batches[c.id] = (torch.from_numpy(seqs).to(DEV), None if users is None else torch.from_numpy(users).to(DEV),
                                  torch.from_numpy(pos).to(DEV))
        return self.batches[c.id]


def _group(rep):
    key = rep.group()
    if key not in _G:
        _G.clear()  # one engine group resident at a time
        _G[key] = _Group(rep)
    return _G[key]


def _write(eng, src, keys=None, span=None):
    """In place, into the tensors the engine holds: src's values (every key, or `keys`; span: a flat element range)."""
    for k in (src if keys is None else keys):
        dst = eng._weights[k]
        assert dst.shape == src[k].shape and dst.data_ptr() != src[k].data_ptr()
        if span is None:
            dst.copy_(src[k])
        else:
            dst.view(-1)[span[0]:span[1]].copy_(src[k].view(-1)[span[0]:span[1]])


# ---------------------------------------------------------------------------------------------------------------- outputs
def _decode(eng, c, batch):
    """Everything the case's decode gives, and a top-k on its first rows: {name: tensor}, and the route of the case's own call."""
    seq, usr, pos = batch
    eng.decoder_gemm = GEMM[c.gemm]
    eng.decoder_seq = SEQ[c.seq]
    try:
        x, xr, ru = eng.decode(seq, usr, want_x=not c.rows_only, pos=pos, want_r_u=not c.evaluator)
        route = eng.decoder_route_last
        out = {"rows": xr}
        if x is not None:
            out["x"] = x
        if ru is not None:
            out["r_u"] = ru
        if c.rows_only and c.full_check:  # the case has both forms: the full window too
            out["full_x"], out["full_rows"], _ = eng.decode(seq, usr, want_x=True, pos=pos)
    finally:
        eng.decoder_gemm = IRS_GEMM_H3
        eng.decoder_seq = None
    rows = torch.nan_to_num(xr[:TOPK_ROWS]).contiguous()  # (a window without a visible key decodes to a NaN row)
    out["top_val"], out["top_ids"], out["top_status"] = eng.score_topk(rows, K, IRS_SWEEP_BF16)
    return out, route


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _diff(got, want, names=None):
    """None, or the first output in which two results differ in a bit."""
    assert set(got) == set(want)
    for k in (names or sorted(want)):
        g, w = got[k], want[k]
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{k}: {tuple(g.shape)} {g.dtype} against {tuple(w.shape)} {w.dtype}"
        if g.dtype.is_floating_point and not torch.equal(torch.isnan(g), torch.isnan(w)):
            return f"{k}: NaN in other places"
        if not torch.equal(_bits(g), _bits(w)):
            ne = (_bits(g) != _bits(w)).reshape(g.shape[0], -1)
            return f"{k}: {int(ne.sum())} of {ne.numel()} words differ, {int(ne.any(1).sum())} rows, first row {int(ne.any(1).nonzero()[0])}"
    return None


ROWS = ("rows", "x", "r_u", "full_x", "full_rows")
SCORES = ("top_val", "top_ids", "top_status")


def _only(out, names):
    return [k for k in names if k in out]


def _runs(mask):
    """[(first byte, bytes)] of the True runs of a 1-d bool tensor."""
    idx = mask.nonzero().view(-1).cpu().numpy()
    if idx.size == 0:
        return []
    cut = np.flatnonzero(np.diff(idx) != 1) + 1
    return [(int(r[0]), int(r.size)) for r in np.split(idx, cut)]


def _record(key, data):
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        cur = {}
        if os.path.exists(OUT):
            with open(OUT) as fh:
                cur = json.load(fh)
        cur[key] = data
        with open(OUT, "w") as fh:
            json.dump(cur, fh, indent=1, sort_keys=True)
    except OSError:
        pass  # a read-only tree must not fail the test


# ---------------------------------------------------------------------------------------------------------------- a. whole model
@pytest.mark.parametrize("rep", W.ordered(), ids=lambda r: r.id)
def test_whole_model_swapped_in_place_equals_a_fresh_engine(rep):
    """Seed A -> every tensor overwritten with seed B's -> back to A, a finalisation after each: the case's route every time, B's
    outputs those of a fresh engine on B and not A's, and A's outputs afterwards the ones from before, bit for bit."""
    g, c = _group(rep), rep.case
    eng, batch = g.eng, g.batch(c)
    try:
        r_a, route = _decode(eng, c, batch)
        assert route == c.route, {k: (route[k], c.route[k]) for k in route if route[k] != c.route[k]}
        _write(eng, g.b)
        eng.finalize()
        r_b, route = _decode(eng, c, batch)
        assert route == c.route, {k: (route[k], c.route[k]) for k in route if route[k] != c.route[k]}
        fresh = g.fresh(g.b_np)
        f_b, f_route = _decode(fresh, c, batch)
        del fresh
        assert f_route == c.route
        assert _diff(r_b, f_b) is None, (c.id, "the re-finalised engine against a fresh one", _diff(r_b, f_b))
        for k in _only(r_a, ROWS + ("top_val",)):
            assert not torch.equal(_bits(r_b[k]), _bits(r_a[k])), (c.id, k, "unchanged by another model")
    finally:
        _write(eng, g.a)
        eng.finalize()
    r_a2, route = _decode(eng, c, batch)
    assert route == c.route
    assert _diff(r_a2, r_a) is None, (c.id, "back on the first model", _diff(r_a2, r_a))


# ---------------------------------------------------------------------------------------------------------------- b. one tensor
@pytest.mark.parametrize("rep", W.one_per_kernel_triple(), ids=lambda r: r.id)
def test_one_tensor_changed_in_place_equals_a_fresh_engine(rep):
    """Every tensor family alone, one key at a time (per-layer kinds: the first, a middle and the last layer): a live one gives
    the outputs of a fresh engine on the mixed state dict and moves the rows (the user tensors: r_u as well; project.*: the
    scores, and only them); a dead one moves no output and no byte of the arena.  The one exception is named in
    weight_lifecycle_cases.REFERENCE_UNMOVED."""
    g, c = _group(rep), rep.case
    eng, batch = g.eng, g.batch(c)
    before, route = _decode(eng, c, batch)
    assert route == c.route
    arena = _arena(eng)
    bad = []
    for fam in W.families(c.evaluator):
        for key in fam.keys(g.cfg):
            span = fam.span(g.cfg, g.a[key].numel())
            try:
                _write(eng, g.b, [key], span)
                eng.finalize()
                got, route = _decode(eng, c, batch)
                what = f"{fam.id} / {key}"
                if route != c.route:
                    bad.append(f"{what}: another route")
                if not fam.live:
                    d = _diff(got, before)
                    if d is not None:
                        bad.append(f"{what}: a dead tensor moved {d}")
                    if not torch.equal(_arena(eng), arena):
                        bad.append(f"{what}: a dead tensor moved {int((_arena(eng) != arena).sum())} bytes of the arena")
                    continue
                fresh = g.fresh(W.mixed(g.cfg, g.a_np, g.b_np, fam, [key]))
                want, _ = _decode(fresh, c, batch)
                del fresh
                d = _diff(got, want)
                if d is not None:
                    bad.append(f"{what}: differs from a fresh engine in {d}")
                if fam.reach == "rows":
                    for name in ("rows",) + fam.also:
                        if torch.equal(_bits(got[name]), _bits(before[name])) and (c.id, fam.id, name) not in W.REFERENCE_UNMOVED:
                            bad.append(f"{what}: a live tensor left {name} unchanged")
                else:
                    if _diff(got, before, _only(got, ROWS)) is not None:
                        bad.append(f"{what}: the projection moved the decoder's rows")
                    if torch.equal(_bits(got["top_val"]), _bits(before["top_val"])):
                        bad.append(f"{what}: a live tensor left the scores unchanged")
            finally:
                _write(eng, g.a, [key])
                eng.finalize()
    after, _ = _decode(eng, c, batch)
    assert _diff(after, before) is None, (c.id, "after every tensor is back", _diff(after, before))
    assert not bad, (c.id, bad)


# ---------------------------------------------------------------------------------------------------------------- c. the arena
@pytest.mark.parametrize("rep", W.groups(), ids=lambda r: r.id)
def test_the_arena_is_determined_by_the_weights(rep):
    """The arena filled with 0xFF, then with 0x00, in front of a finalisation: the derived bytes equal those of a fresh engine
    whose arena held the same byte.  What differs between the two fills is what finalisation never writes: the same places in
    the used and the fresh engine, under ARENA_UNWRITTEN_MAX bytes, and no output of any representative of the engine group
    (every route that reads these packs) depends on them."""
    g, c = _group(rep), rep.case
    eng = g.eng
    members = [r.case for r in W.ordered() if r.group() == rep.group()]  # every route of this engine reads the filled arena
    assert members[0] is c
    for m in members:
        _decode(eng, m, g.batch(m))
    used, fresh, outs = {}, {}, {}
    try:
        for byte in (0xFF, 0x00):
            eng._arena.fill_(byte)
            eng.finalize()
            used[byte] = _arena(eng)
            for m in members:
                outs[byte, m.id], route = _decode(eng, m, g.batch(m))
                assert route == m.route, m.id
            assert torch.equal(_arena(eng), used[byte]), "a decode wrote into the arena"
            f = g.fresh(g.a_np, poison=byte)
            fresh[byte] = _arena(f)
            del f
            ne = used[byte] != fresh[byte]
            assert not bool(ne.any()), (c.id, hex(byte), "the used engine's arena against a fresh one's", _runs(ne)[:8])
    finally:
        eng.finalize()
    gap_used, gap_fresh = used[0xFF] != used[0x00], fresh[0xFF] != fresh[0x00]
    runs = _runs(gap_used)
    n = int(gap_used.sum())
    print(f"arena {c.id}: {n} of {gap_used.numel()} derived bytes unwritten, runs (offset, bytes) {runs}")
    _record("|".join(str(v) for v in rep.group()), dict(case=c.id, derived_bytes=int(gap_used.numel()), unwritten=n, runs=runs))
    assert torch.equal(gap_used, gap_fresh)
    assert n < W.ARENA_UNWRITTEN_MAX, (c.id, n, runs)
    for m in members:
        d = _diff(outs[0xFF, m.id], outs[0x00, m.id])
        assert d is None, (m.id, "an output depends on unwritten arena bytes", d)


def _greedy(eng, held, src, users, graph):
    seq, hep, paths, status = held
    seq.copy_(src)
    hep.fill_(eng.L - 2)
    paths.zero_()
    status.zero_()
    eng.generate_paths(seq, users, hep, 3, k=K, use_graph=graph, paths=paths, status=status)
    return dict(paths=paths.clone(), status=status.clone(), seq=seq.clone(), hep=hep.clone())


def test_the_arena_moves():
    """A finalisation into a new arena, the old one then filled with 0xFF: the rows and a captured greedy step (on caller-held
    buffers, so that its addresses stay the key of the captured step) are what they were, and equal the uncaptured step."""
    rep = W.REP_BY_ID["c2_b164_seq1"]
    g, c = _group(rep), rep.case
    eng, batch = g.eng, g.batch(c)
    seqs, users, _ = E._search_windows(8, g.cfg, 31)
    src, usr = torch.from_numpy(seqs).to(DEV), torch.from_numpy(users).to(DEV)
    held = (torch.empty_like(src), torch.empty(8, dtype=torch.int32, device=DEV), torch.empty((8, 3), dtype=torch.float32, device=DEV),
            torch.empty(8, dtype=torch.int32, device=DEV))
    rows0, _ = _decode(eng, c, batch)
    plain0 = _greedy(eng, held, src, usr, False)
    graph0 = _greedy(eng, held, src, usr, True)
    assert _diff(graph0, plain0) is None
    assert _diff(_greedy(eng, held, src, usr, True), plain0) is None  # (the replay of the step just captured)
    old = eng._arena
    eng._arena = None
    eng.finalize()
    assert eng._arena is not None and eng._arena.data_ptr() != old.data_ptr()
    old.fill_(0xFF)
    graph1 = _greedy(eng, held, src, usr, True)
    plain1 = _greedy(eng, held, src, usr, False)
    rows1, route = _decode(eng, c, batch)
    torch.cuda.synchronize()
    assert route == c.route
    assert _diff(graph1, plain0) is None, _diff(graph1, plain0)
    assert _diff(plain1, plain0) is None, _diff(plain1, plain0)
    assert _diff(rows1, rows0) is None, _diff(rows1, rows0)
    assert int(plain0["paths"].min()) >= 1  # (every user took three steps)


# ---------------------------------------------------------------------------------------------------------------- d. range bound
@pytest.mark.parametrize("B", [164, 384])
def test_the_float16_range_bound_follows_the_weights(B):
    """The recipe of test_float16_planes_fall_back_outside_their_range (linear1 x 4096, linear2.weight / 4096), in place on a used
    engine: finalisation re-evaluates the bound, IRS_GEMM_H3 runs as IRS_GEMM_X6 on the route and with the rows of a fresh engine
    on the scaled weights -- and back."""
    c = BY_ID["c2_b164" if B == 164 else "c2_b384"]
    assert c.B == B and c.gemm == "h3" and c.seq == "auto"
    g = _group(W.REP_BY_ID["c2_b164_seq1"])
    assert g.n >= B and g.cfg.name == "c2" and g.cfg.n_layers == 6
    eng, batch = g.eng, g.batch(c)
    before, route = _decode(eng, c, batch)
    assert route == c.route and eng.decoder_gemm == IRS_GEMM_H3 == eng.decoder_gemm_effective and 0 < eng.h3_range_bound < 32752
    big_np = dict(g.a_np)
    for l in range(g.cfg.n_layers):
        p = f"decoder.layers.{l}."
        big_np[p + "linear1.weight"] = g.a_np[p + "linear1.weight"] * np.float32(4096.0)
        big_np[p + "linear1.bias"] = g.a_np[p + "linear1.bias"] * np.float32(4096.0)
        big_np[p + "linear2.weight"] = g.a_np[p + "linear2.weight"] / np.float32(4096.0)
    try:
        for l in range(g.cfg.n_layers):
            p = f"decoder.layers.{l}."
            eng._weights[p + "linear1.weight"].mul_(4096.0)
            eng._weights[p + "linear1.bias"].mul_(4096.0)
            eng._weights[p + "linear2.weight"].div_(4096.0)
        eng.finalize()
        assert eng.h3_range_bound >= 32752, eng.h3_range_bound
        assert eng.decoder_gemm == IRS_GEMM_H3 and eng.decoder_gemm_effective == IRS_GEMM_X6
        got, route = _decode(eng, c, batch)
        fresh = g.fresh(big_np)
        assert fresh.h3_range_bound == eng.h3_range_bound and fresh.decoder_gemm_effective == IRS_GEMM_X6
        want, f_route = _decode(fresh, c, batch)
        del fresh
        assert route == f_route, {k: (route[k], f_route[k]) for k in route if route[k] != f_route[k]}
        assert route["npl"] == 3 and not route["kv_planes"] and not route["seq"] and route["layer"] == "FRAG_FUSED"
        assert _diff(got, want) is None, _diff(got, want)
        assert torch.isfinite(got["rows"]).sum() == torch.isfinite(before["rows"]).sum()
    finally:
        _write(eng, g.a)
        eng.finalize()
    assert eng.decoder_gemm_effective == IRS_GEMM_H3 and 0 < eng.h3_range_bound < 32752
    after, route = _decode(eng, c, batch)
    assert route == c.route
    assert _diff(after, before) is None, _diff(after, before)


# ---------------------------------------------------------------------------------------------------------------- e. scoring
def _score_all(eng, inp):
    """Every scoring entry point on the 33 rows: {name: tensor}."""
    x = inp["rows"]
    out = {}
    for name, sweep in (("bf16", IRS_SWEEP_BF16), ("f32", IRS_SWEEP_F32)):
        out[name + "_val"], out[name + "_ids"], out[name + "_status"] = eng.score_topk(x, K, sweep)
    out["lse_max"], out["lse_sum"] = eng.score_lse(x)
    out["dense"] = eng.score_dense(x)
    out["gather"] = eng.score_gather(x, inp["ids"])
    ref = eng.score_gather(x, inp["labels"].view(-1, 1))[:, 0].contiguous()
    out["ref"], out["count"] = ref, eng.score_count_before(x, ref, inp["labels"], inp["hist"])
    return out


def _scoring_inputs(n_item, d, lo, hi):
    g = np.random.default_rng(n_item + d)
    M = W.SCORING_ROWS
    ids = g.integers(lo, hi, size=(M, 7)).astype(np.int64)
    ids[0, 0], ids[1, 1] = -1, (hi if hi < n_item else 0)  # unused slot; an id of another shard where there is one
    hist = g.integers(lo, hi, size=(M, 11)).astype(np.int64)
    hist[:, 3], hist[:, 5] = hist[:, 4], -1
    inp = dict(rows=_rows(M, d, n_item), later=(_rows(M, d, n_item) + 0.02 * g.standard_normal((M, d))).astype(np.float32), ids=ids,
               labels=g.integers(lo, hi, size=M).astype(np.int64), hist=hist)
    return {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def _scoring_lifecycle(n_item, d, rank, world, steps, full=True):
    """A used scoring-only engine through `steps` = [(name, W, b)], written into the WHOLE tensors in place with a finalisation
    after each; behind each: the carried call first, then (full) every entry point and the arena, against a fresh engine.
    Every arena here starts as zeros, the used engine's once and each fresh engine's: the derived bytes then have to be equal
    as a whole, the ones finalisation does not write included, and a statistic that finalisation only ever raises shows."""
    W0, b0 = _weights(n_item, d, 1)
    cfg, sd_np = _scoring_only(n_item, d, W0, b0)
    sd = _up(sd_np)
    eng = _new_engine(cfg, sd, max_rows=64, max_seqs=1, rank=rank, world=world, poison=0x00)
    lo, hi = eng.item_lo, eng.item_hi
    assert (eng._weights["project.weight"].data_ptr() != sd["project.weight"].data_ptr()) == (world > 1 and rank > 0)
    inp = _scoring_inputs(n_item, d, lo, hi)
    if full:  # the bytes of the arena that finalisation does not write: those that follow the fill
        fills = [_arena(_new_engine(cfg, _up(sd_np), max_rows=64, max_seqs=1, rank=rank, world=world, poison=p)) for p in (0xFF, 0x00)]
        gap = fills[0] != fills[1]
        n = int(gap.sum())
        print(f"arena scoring {n_item} x {d} rank {rank}/{world}: {n} of {gap.numel()} derived bytes unwritten, runs {_runs(gap)}")
        _record(f"scoring|{n_item}|{d}|{rank}|{world}", dict(derived_bytes=int(gap.numel()), unwritten=n, runs=_runs(gap)))
        assert n < W.ARENA_UNWRITTEN_MAX
        assert torch.equal(_arena(eng), fills[1])
        _score_all(eng, inp)
    # the used engine ends on a plain call and a carried one: it holds thresholds of the catalog it is about to lose
    eng.score_topk(inp["rows"], K, IRS_SWEEP_BF16)
    eng.score_topk(inp["later"], K, IRS_SWEEP_BF16, carry=True)
    prev = None
    for name, Wn, bn in steps:
        new = dict(sd_np)
        new["project.weight"], new["project.bias"] = Wn, bn
        new_dev = _up(new)
        sd["project.weight"].copy_(new_dev["project.weight"])
        sd["project.bias"].copy_(new_dev["project.bias"])
        eng.finalize()
        fresh = _new_engine(cfg, new_dev, max_rows=64, max_seqs=1, rank=rank, world=world, poison=0x00)
        cv, ci, cs = eng.score_topk(inp["later"], K, IRS_SWEEP_BF16, carry=True)     # the first call behind the finalisation
        fv, fi, fs = fresh.score_topk(inp["later"], K, IRS_SWEEP_BF16, carry=True)   # a fresh engine's first call
        d_ = _diff(dict(val=cv, ids=ci, status=cs), dict(val=fv, ids=fi, status=fs))
        assert d_ is None, (name, "the carried call behind the finalisation", d_)
        if full:
            got, want = _score_all(eng, inp), _score_all(fresh, inp)
            assert _diff(got, want) is None, (name, _diff(got, want))
            ne = _arena(eng) != _arena(fresh)
            assert not bool(ne.any()), (name, "arena", int(ne.sum()), _runs(ne)[:8])
            if prev is not None:
                assert not torch.equal(_bits(got["bf16_val"]), _bits(prev["bf16_val"])), name
            prev = got
        # (and again a plain call and a carried one on the catalog of this step)
        eng.score_topk(inp["rows"], K, IRS_SWEEP_BF16)
        v2, i2, s2 = eng.score_topk(inp["later"], K, IRS_SWEEP_BF16, carry=True)
        assert torch.equal(i2, ci) and torch.equal(_bits(v2), _bits(cv)), (name, "the carried lists are exact lists")
        del fresh


@pytest.mark.parametrize("n_item,d,rank,world", W.SCORING, ids=[f"{n}x{d}-r{r}of{w}" for n, d, r, w in W.SCORING])
def test_scoring_follows_the_catalog_written_in_place(n_item, d, rank, world):
    """project.weight / project.bias overwritten in place with another seed, then that catalog x 8 and x 1/8 (the filter norms
    move both ways): top-k under both sweeps, log-sum-exp, dense scores, gather, rank counts, the arena and a carried call,
    each bit-identical to a fresh engine's."""
    W1, b1 = _weights(n_item, d, 2)
    eight, eighth = np.float32(8.0), np.float32(0.125)
    _scoring_lifecycle(n_item, d, rank, world, [("seed", W1, b1), ("x8", W1 * eight, b1 * eight), ("x1/8", W1 * eighth, b1 * eighth)])


def test_carried_thresholds_do_not_survive_a_new_catalog():
    """The carried call reuses thresholds only from 524288 items up (irs_launch_topk): below, the carried calls above run as plain
    ones.  Here the catalog of tests/engine_state_cases.py's engine L is scaled by 1/8 in place under thresholds selected on the
    unscaled one: kept, they would sit 8 x too high for every row, and the status words would report the fallback."""
    n_item, d = E.L_ITEMS, E.D
    W0, b0 = _weights(n_item, d, 1)
    eighth = np.float32(0.125)
    _scoring_lifecycle(n_item, d, 0, 1, [("x1/8", W0 * eighth, b0 * eighth)], full=False)


# ---------------------------------------------------------------------------------------------------------------- f. front end
def _fresh_for(net, cfg, causal, max_seqs, max_rows):
    sd = {k: v.detach().clone() for k, v in net.state_dict().items() if v.dtype == torch.float32}
    return _new_engine(cfg, sd, evaluator=causal, max_rows=max_rows, max_seqs=max_seqs)


def _front_compare(net, cfg, seq, user, pos, sizes, max_seqs, max_rows):
    """decode_rows of the module's engine at every batch size against a fresh engine on the module's state_dict; {B: rows}."""
    fresh = _fresh_for(net, cfg, False, max_seqs, max_rows)
    out = {}
    for B in sizes:
        xr = net.decode_rows(seq[:B], user[:B], pos[:B])
        eng = net._hip.engine
        _, fxr, _ = fresh.decode(seq[:B], user[:B], want_x=False, pos=pos[:B])
        assert eng.decoder_route_last == fresh.decoder_route_last, B
        assert torch.equal(torch.isnan(xr), torch.isnan(fxr)) and torch.equal(_bits(xr), _bits(fxr)), (B, "rows")
        rows = torch.nan_to_num(xr[:TOPK_ROWS]).contiguous()
        _, ids, _ = eng.score_topk(rows, K, IRS_SWEEP_BF16)
        _, fids, _ = fresh.score_topk(rows, K, IRS_SWEEP_BF16)
        assert torch.equal(ids, fids), (B, "top-k ids")
        out[B] = xr.clone()
    return out


@pytest.mark.parametrize("trunk", ["torch", "hip"])
def test_front_end_inference_after_training_equals_a_fresh_engine(trunk):
    """InfluentialNet at c2: the module's engine decodes, three train_batch steps move every parameter in place, and the next
    decode_rows (1, 40, 164 and 384 sequences: four routes) is a fresh engine's on the trained state_dict -- on the SAME engine
    object, which the steps in between used for the loss.  Then a .data write behind autograd's back, and invalidate()."""
    from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
    torch.manual_seed(5)
    cfg = synth.make_config("c2", dropout=0.0)
    net = InfluentialNet(cfg)
    a_np, b_np = W.state_dicts(cfg, False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in a_np.items()})
    net.to(DEV)
    net.trunk = trunk
    irn = IRSNN(cfg, net, DEV)
    sizes, S, R = (1, 40, 164, 384), 384, 512
    seqs, users, pos, _ = _batch(Case("front", "c2", S, {}), cfg, seed=1000 + S)
    seq, user, p = torch.from_numpy(seqs).to(DEV), torch.from_numpy(users).to(DEV), torch.from_numpy(pos).to(DEV)
    net.eval()
    eng = net._hip.get(S, R)  # sized once for everything below: the engine object stays
    r0 = net.decode_rows(seq, user, p).clone()
    assert net._hip.engine is eng
    train_seq, train_user = seq[2:4].contiguous(), user[2:4].contiguous()  # (a full window and a repeated item among them)
    for _ in range(3):
        irn.train_batch(train_seq, train_user)
    assert net._hip.engine is eng, "the training steps ran on another engine"
    net.eval()
    trained = _front_compare(net, cfg, seq, user, p, sizes, S, R)
    assert net._hip.engine is eng
    assert not torch.equal(_bits(trained[S]), _bits(r0))
    # a write that bumps no version counter
    name = "decoder.layers.3.linear2.weight"
    dict(net.named_parameters())[name].data.copy_(torch.from_numpy(b_np[name]).to(DEV))
    net._hip.invalidate()
    written = _front_compare(net, cfg, seq, user, p, sizes, S, R)
    assert net._hip.engine is eng
    for B in sizes:
        assert not torch.equal(_bits(written[B]), _bits(trained[B])), B


@pytest.mark.parametrize("trunk", ["torch", "hip"])
def test_evaluator_inference_after_training_equals_a_fresh_engine(trunk):
    """The same for SampleNet / Evaluator at eval_default (causal mask, post-padded windows, no user factor)."""
    from influentialrs_amd.model.evaluator import Evaluator
    from influentialrs_amd.model.uRS import SampleNet
    torch.manual_seed(6)
    cfg = synth.make_config("eval_default", dropout=0.0)
    net = SampleNet(cfg)
    a_np, _ = W.state_dicts(cfg, True)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in a_np.items()})
    net.to(DEV)
    net.trunk = trunk
    ev = Evaluator(cfg, net, DEV)
    S, R = 40, 256
    win = synth.random_windows(S, cfg.max_len, cfg.n_item, seed=S)
    win = np.stack([np.concatenate([r[r > 0], r[r == 0]]) for r in win])  # the evaluator's post-padded rows
    seq = torch.from_numpy(win).to(DEV)
    rows_b = torch.arange(S, device=DEV)
    rows_pos = (seq.gt(0).sum(1) - 1).clamp_(min=0)
    net.eval()
    eng = net._hip.get(S, R)
    r0 = net.decode_rows(seq, rows_b, rows_pos).clone()
    assert net._hip.engine is eng
    for _ in range(3):
        ev.train_batch(seq[:4].contiguous())
    assert net._hip.engine is eng, "the training steps ran on another engine"
    net.eval()
    fresh = _fresh_for(net, cfg, True, S, R)
    for B in (1, S):
        xr = net.decode_rows(seq[:B], rows_b[:B], rows_pos[:B])
        fx, _, _ = fresh.decode(seq[:B], None, want_x=True)
        fxr = fx[rows_b[:B], rows_pos[:B]].contiguous()
        assert net._hip.engine is eng
        assert eng.decoder_route_last == fresh.decoder_route_last
        assert torch.equal(_bits(xr), _bits(fxr)), (B, "rows")
        _, ids, _ = eng.score_topk(xr[:TOPK_ROWS].contiguous(), K, IRS_SWEEP_BF16)
        _, fids, _ = fresh.score_topk(xr[:TOPK_ROWS].contiguous(), K, IRS_SWEEP_BF16)
        assert torch.equal(ids, fids), (B, "top-k ids")
    assert not torch.equal(_bits(net.decode_rows(seq, rows_b, rows_pos)), _bits(r0))
