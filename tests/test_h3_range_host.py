"""not-gpu: the float16-plane range bound, restated (tests/h3_range_ref.py), at the edge of every term.

irs_h3_operand_bound folds eight statistics of the weights into one bound; at 32752 the engine leaves the float16-plane kernels.
Here, on the c2 (sequence-resident) and c4d (d = 256) dims with 2 layers, 257 items and 24-token windows:

- every tensor family of h3_range_ref.FAMILIES can be scaled to put the bound inside ([0.5, 0.9] x 32752) and outside ([1.1, 2.0] x
  32752), and the term that decides the bound there is the one named in DECIDING -- a change of the formula fails a named case;
- soundness: a float64 forward of the base model and of every inside model reaches no operand above the bound (a condition, not
  a measurement; the actual-to-bound ratios are printed, with no assertion on tightness);
- the V-row statistic covers the q and k rows on the sequence-resident dims only.

tests/test_gpu_h3_range.py holds the engine to this restatement."""
import numpy as np
import pytest

import h3_range_ref as R
from influentialrs_amd import synth

DIMS = ("c2", "c4d")
INSIDE, OUTSIDE = (0.5, 0.9), (1.1, 2.0)
# The deciding term per family, the same on both dims and on both sides of the limit.  At these dims a V row's bound is sqrt(d) x
# (row norm ~0.8) ~ 9 (d = 128) / 12 (d = 256) times the bound of the layer input it multiplies, and a hidden activation's ~7 / 10
# times the LayerNorm output's with a smaller input norm: whatever raises an embedded token (E, pe) or a LayerNorm output (gamma,
# beta, c_l) reaches the limit through `v` first.
DECIDING = {"E": "v", "pe": "v", "ln_gamma": "v", "ln_beta": "v", "cross_bias": "v", "ffn1": "hidden", "v_rows": "v", "out_w": "wplane"}
# what a family has to move on the way (terms that must grow with s besides the deciding one)
THROUGH = {"E": "embed", "pe": "embed", "ln_gamma": "ln", "ln_beta": "ln", "cross_bias": "ln"}
_MODEL = {}


def _model(name):
    if name not in _MODEL:
        cfg = synth.make_config(name, n_layers=2, n_item=257, max_len=24)
        sd = synth.irn_state_dict(cfg, 2027)
        L, n = cfg.max_len, cfg.n_item
        g = np.random.default_rng(24)
        seqs = np.zeros((6, L), dtype=np.int64)
        seqs[0] = g.integers(1, n + 1, size=L)                  # a full window
        seqs[1, L - 1] = int(g.integers(1, n + 1))              # a single token (the target alone)
        seqs[2] = int(g.integers(1, n + 1))                     # one item repeated across the window
        for b in (3, 4, 5):                                     # random lengths, pre-padded
            k = int(g.integers(2, L))
            seqs[b, L - k:] = g.integers(1, n + 1, size=k)
        users = g.integers(0, cfg.n_user, size=6).astype(np.int64)
        _MODEL[name] = (cfg, sd, seqs, users)
    return _MODEL[name]


def test_seq_shape_mirrors_the_source():
    """h3_range_ref.seq_shape restates irs_seq_shape: the same five conditions, read from irs_internal.h."""
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "influentialrs_amd", "csrc", "irs_internal.h")) as fh:
        m = re.search(r"irs_seq_shape\(const irs_dims &D\) \{\s*return ([^;]*);", fh.read())
    assert m and m.group(1).replace(" ", "") == "D.d==128&&D.ffn_dim==256&&D.n_heads==4&&D.max_len<=256&&D.n_layers>1"
    assert R.seq_shape(_model("c2")[0]) and not R.seq_shape(_model("c4d")[0])
    assert not R.seq_shape(synth.make_config("c2", n_layers=1)) and not R.seq_shape(synth.make_config("c2", max_len=257))
    assert not R.seq_shape(synth.make_config("c2", n_heads=8)) and not R.seq_shape(synth.make_config("c2", ffn_dim=128))


@pytest.mark.parametrize("name", DIMS)
def test_forward_equals_the_float64_oracle(oracle, name):
    """operand_maxima's forward is oracle_np.decode(..., dtype=np.float64): final rows to 1e-12 relative, the same NaNs."""
    cfg, sd, seqs, users = _model(name)
    for model in (sd, R.scaled(sd, cfg, "E", R.solve(sd, cfg, "E", *INSIDE)[0])):
        _, rows = R.operand_maxima(model, cfg, seqs, users)
        for b in range(len(seqs)):
            ref = oracle.decode(model, cfg, seqs[b], int(users[b]), dtype=np.float64)[0]
            assert np.array_equal(np.isnan(rows[b]), np.isnan(ref)) and np.isfinite(ref).all()
            assert np.abs(rows[b] - ref).max() <= 1e-12 * np.abs(ref).max(), b


def test_statistics_and_nan():
    """Each slot reads its own tensors (one planted value per slot moves that slot alone), and a NaN maps to inf."""
    cfg, sd, _, _ = _model("c2")
    d = cfg.emb_dim
    base = R.stats(sd, cfg)
    plant = [("item_embedder.weight", (5, 3)), ("pos_embedder.pe", (0, 7, 2)), ("decoder.layers.1.norm3.weight", (4,)),
             ("decoder.layers.1.norm1.bias", (4,)), ("decoder.layers.1.multihead_attn.out_proj.bias", (9,)),
             None, None, ("decoder.layers.1.self_attn.in_proj_bias", (2 * d + 1,))]
    for slot, p in enumerate(plant):
        if p is None:
            continue
        for val in (1000.0, np.nan):
            m = dict(sd)
            m[p[0]] = sd[p[0]].copy()
            m[p[0]][p[1]] = val
            st = R.stats(m, cfg)
            changed = [i for i in range(8) if st[i] != base[i]]
            assert changed == [slot], (slot, changed)
            assert st[slot] == (np.inf if np.isnan(val) else pytest.approx(1000.0, rel=1e-3)), (slot, st[slot])
    # the row-norm slots: a row of W1 (5, and 7 as a weight), a V row (6 and 7)
    m = dict(sd)
    m["decoder.layers.1.linear1.weight"] = sd["decoder.layers.1.linear1.weight"].copy()
    m["decoder.layers.1.linear1.weight"][255] = 3.0
    st = R.stats(m, cfg)
    assert st[5] == pytest.approx(3.0 * np.sqrt(d)) and st[7] == 3.0 and np.array_equal(st[[0, 1, 2, 3, 4, 6]], base[[0, 1, 2, 3, 4, 6]])
    m = dict(sd)
    m["decoder.layers.1.self_attn.in_proj_weight"] = sd["decoder.layers.1.self_attn.in_proj_weight"].copy()
    m["decoder.layers.1.self_attn.in_proj_weight"][3 * d - 1] = -3.0
    st = R.stats(m, cfg)
    assert st[6] == pytest.approx(3.0 * np.sqrt(d)) and st[7] == 3.0 and np.array_equal(st[:6], base[:6])
    assert R.terms(R.stats(m, cfg), d)["wplane"] == 3.0 * 256.0
    # a tensor outside the decoder's operands moves nothing
    m = dict(sd)
    m["project.weight"] = sd["project.weight"] * 1e6
    m["decoder.layers.0.multihead_attn.in_proj_weight"] = sd["decoder.layers.0.multihead_attn.in_proj_weight"] * 1e6
    assert np.array_equal(R.stats(m, cfg), base)


@pytest.mark.parametrize("which", R.FAMILIES)
@pytest.mark.parametrize("name", DIMS)
def test_deciding_term_and_soundness(name, which, capsys):
    cfg, sd, seqs, users = _model(name)
    b0, _, t0 = R.bound(sd, cfg)
    assert 0 < b0 < 0.5 * R.LIMIT  # a model of ordinary scale sits well inside
    for side, (lo, hi) in (("inside", INSIDE), ("outside", OUTSIDE)):
        s, term = R.solve(sd, cfg, which, lo, hi)
        model = R.scaled(sd, cfg, which, s)
        b, term2, t = R.bound(model, cfg)
        assert lo * R.LIMIT <= b <= hi * R.LIMIT and term == term2
        assert term == DECIDING[which], (name, which, side, t)
        assert t[term] > t0[term] * 10  # the family moved its term: the base model's did not decide by itself
        if which in THROUGH:
            assert t[THROUGH[which]] > t0[THROUGH[which]] * 10, (name, which, side, t)
        if side == "inside":
            mx, rows = R.operand_maxima(model, cfg, seqs, users)
            assert np.isfinite(rows).all()
            ratios = {k: v / b for k, v in mx.items()}
            with capsys.disabled():
                print(f"\n[h3-range] {name} {which} s={s:.6g} {term} bound={b:.1f} actual/bound " +
                      " ".join(f"{k}={r:.4f}" for k, r in ratios.items()))
            assert all(r <= 1.0 for r in ratios.values()), (name, which, ratios)
            if which in ("ffn1", "v_rows"):  # the function-preserving pairs compute what the base model computes
                ref = R.operand_maxima(sd, cfg, seqs, users)[1]
                assert np.abs(rows - ref).max() < 1e-5


@pytest.mark.parametrize("name", DIMS)
def test_base_model_is_sound(name, capsys):
    cfg, sd, seqs, users = _model(name)
    b, term, _ = R.bound(sd, cfg)
    mx, _ = R.operand_maxima(sd, cfg, seqs, users)
    with capsys.disabled():
        print(f"\n[h3-range] {name} base {term} bound={b:.1f} actual/bound " + " ".join(f"{k}={v / b:.4f}" for k, v in mx.items()))
    assert all(v <= b for v in mx.values()), (name, mx, b)


def test_q_rows_count_on_the_sequence_resident_dims_only():
    """Slot 6 holds all of W_in's rows where the sequence-resident kernel splits q and k into float16 planes too (c2 dims), the V
    rows alone elsewhere (c4d dims): the q rows of layer 0 scaled by the v_rows outside factor move `v` on c2 and not on c4d."""
    for name, moves in (("c2", True), ("c4d", False)):
        cfg, sd, _, _ = _model(name)
        d = cfg.emb_dim
        s, _ = R.solve(sd, cfg, "v_rows", *OUTSIDE)
        m = dict(sd)
        key = "decoder.layers.0.self_attn.in_proj_weight"
        m[key] = sd[key].copy()
        m[key][:d] *= np.float32(s)
        st0, st = R.stats(sd, cfg), R.stats(m, cfg)
        t0, t = R.terms(st0, d), R.terms(st, d)
        assert st[7] > st0[7]  # (a weight plane either way)
        if moves:
            assert st[6] > st0[6] * (s / 2) and t["v"] > R.LIMIT and R.deciding(t) == "v"
        else:
            assert st[6] == st0[6] and t["v"] - t0["v"] == pytest.approx(st[7] - st0[7]) and t["bound"] < R.LIMIT
