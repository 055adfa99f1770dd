"""not-gpu: the tables of tests/weight_lifecycle_cases.py cover what tests/test_gpu_weight_lifecycle.py is there to run.

- The tensor families stand for the key set of synth.irn_state_dict exactly, IRN and evaluator: no key is missing, none appears
  twice, and a key that is split into parts is split completely.
- Every kernel family of tests/decoder_route_cases.py and of tests/long_window_cases.py that a decode of at most MAX_SEQS
  sequences reaches has a representative, the one with the fewest sequences, and no representative needs more."""
import pytest

import decoder_route_cases as RC
import long_window_cases as LW
import weight_lifecycle_cases as W
from influentialrs_amd import synth

CONFIGS = [("tiny", False, {}), ("c2", False, {}), ("c2", False, {"n_layers": 1}), ("c2", False, {"n_layers": 2}), ("default", False, {}),
           ("eval_default", True, {}), ("c2", True, {})]


@pytest.mark.parametrize("name,evaluator,over", CONFIGS, ids=["-".join([n] + ["eval"] * e + [f"{k}{v}" for k, v in o.items()]) for n, e, o in CONFIGS])
def test_families_cover_the_state_dict_exactly(name, evaluator, over):
    cfg = synth.make_config(name, **({"n_user": 0} if evaluator else {}), **over)
    keys = set(synth.irn_state_dict(cfg, 1, evaluator=evaluator))
    got = W.covered_keys(cfg, evaluator)
    assert keys - set(got) == set(), "keys without a family"
    assert set(got) - keys == set(), "families for keys the state_dict does not have"
    for k, parts in got.items():
        assert parts == [None] or sorted(parts) == ["qk", "v"], (k, parts)  # once, or as the two parts of a complete split
    split = {k for k, parts in got.items() if parts != [None]}
    assert split == {f"decoder.layers.{l}.{W.CROSS_BIAS}" for l in range(cfg.n_layers)}


def test_dead_families_are_the_projects_own_statement():
    dead = {(f.kind, f.part) for f in W.FAMILIES if not f.live}
    assert dead == {("multihead_attn.in_proj_weight", None), (W.CROSS_BIAS, "qk")}
    cfg = synth.make_config("tiny")
    qk, v = W.FAMILY_BY_ID[W.CROSS_BIAS + ":qk"], W.FAMILY_BY_ID[W.CROSS_BIAS + ":v"]
    d = cfg.emb_dim
    assert qk.span(cfg, 3 * d) == (0, 2 * d) and v.span(cfg, 3 * d) == (2 * d, 3 * d) and v.live
    assert {f.reach for f in W.FAMILIES} == {"rows", "scores"}
    users = {"user_embedder.weight", "user_mask_layer.weight", "user_mask_layer.bias"}
    assert {f.kind for f in W.FAMILIES if f.also} == users and all(f.also == ("r_u",) and f.reach == "rows" for f in W.FAMILIES if f.also)
    # one window of a one-layer model is the only exception to "a live tensor moves the rows"
    assert W.REFERENCE_UNMOVED == {("c2_nl1_b1", k, "rows") for k in users}
    assert "c2_nl1_b1" in {r.id for r in W.one_per_kernel_triple()} and W.REP_BY_ID["c2_nl1_b1"].case.B == 1
    assert {f.kind for f in W.FAMILIES if f.reach == "scores"} == {"project.weight", "project.bias"}


def test_a_family_changes_the_first_a_middle_and_the_last_layer():
    f = W.FAMILY_BY_ID["norm3.weight"]
    assert f.layers(6) == [0, 3, 5] and f.layers(2) == [0, 1] and f.layers(1) == [0] and f.layers(3) == [0, 1, 2]
    assert W.FAMILY_BY_ID["project.bias"].layers(6) == []


@pytest.mark.parametrize("evaluator", [False, True])
def test_the_two_state_dicts_differ_in_every_tensor(evaluator):
    import numpy as np
    cfg = synth.make_config("eval_tiny" if evaluator else "tiny", **({"n_user": 0} if evaluator else {}))
    a, b = W.state_dicts(cfg, evaluator)
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype == np.float32 and not np.array_equal(a[k], b[k]), k
    emb = "word_embedder.weight" if evaluator else "item_embedder.weight"
    assert not a[emb][0].any() and not b[emb][0].any()
    for f in W.families(evaluator):  # a mixed state dict differs from A in the family's span of the family's keys, nowhere else
        m = W.mixed(cfg, a, b, f)
        for k in a:
            if k in f.keys(cfg):
                lo, hi = f.span(cfg, a[k].size)
                am, bm, mm = a[k].reshape(-1), b[k].reshape(-1), m[k].reshape(-1)
                assert np.array_equal(mm[lo:hi], bm[lo:hi]) and np.array_equal(mm[:lo], am[:lo]) and np.array_equal(mm[hi:], am[hi:])
            else:
                assert m[k] is a[k]


@pytest.mark.parametrize("table", sorted(W.TABLES))
def test_every_kernel_family_has_its_smallest_representative(table):
    cases = W.TABLES[table]
    assert cases is (RC.CASES if table == "routes" else LW.CASES)
    reps = [r.case for r in W.REPRESENTATIVES if r.table == table]
    assert all(any(c is x for x in cases) for c in reps), "a representative is a Case object of the route table"
    by_family = {W.kernel_family(c): c for c in reps}
    assert len(by_family) == len(reps), "two representatives of one kernel family"
    for c in cases:
        if c.B > W.MAX_SEQS:
            continue
        fam = W.kernel_family(c)
        assert fam in by_family, f"{c.id}: kernel family {fam} has no representative"
        assert by_family[fam].B <= c.B, (c.id, by_family[fam].id)
    # the families that only the cases beyond the cap reach would be a gap: there is none
    capped = {W.kernel_family(c) for c in cases if c.B > W.MAX_SEQS}
    assert capped <= set(by_family), capped - set(by_family)


EXPECTED = {  # written down by hand: a table that shrinks, or a selection that changes, shows here
    "routes": ["c2_b1_att_fused", "c2_b2", "default_b1_any", "c4d_b1", "c2_nl1_b1", "tiny_L2", "c2_L256_b129", "default_b1093",
               "c1_b1311", "c2_h8_b72", "c2_h8_b176", "c2_f128_b10", "c2_f128_b11", "c4d_b164", "c4d_b163_f32", "c4d_b164_f32",
               "c4d_full_b163", "c4d_full_b164", "c4d_f128_b16", "d192_b168", "c2_b164_attn_f32", "c2_b164_f32", "c2_nl1_b164",
               "c2_b600_x6", "c2_full_b8", "c2_b164_seq1", "eval_c2_b16", "eval_c2_b600", "eval_default_b40"],
    "long": ["tiny_L1024_b3", "c2_L320_b1", "c2_L320_b110", "c2_h2_L288_b6", "c4d_L320_b4", "eval_c2_L320_b6", "eval_default_L300_b6"],
}


@pytest.mark.parametrize("table", sorted(W.TABLES))
def test_the_representatives_are_the_expected_ones(table):
    assert [r.id for r in W.REPRESENTATIVES if r.table == table] == EXPECTED[table]
    assert (len(EXPECTED["routes"]), len(EXPECTED["long"])) == (29, 7)


def test_kernel_family_is_the_twelve_fields():
    c = RC.BY_ID["c2_b164"]
    assert W.kernel_family(c) == ("FRAG_QKV", "FRAG_FUSED", "SMALL16", False, True, False, True, 2, 4, False, "h3", "h3")
    assert len(W.FAMILY_FIELDS) + 3 == 12
    # every family the issue names is reached: the c2 and c4d routes, the per-GEMM and fragment-major families, the evaluator
    have = {(r.case.route["embed"], r.case.route["layer"], r.case.route["tail"]) for r in W.REPRESENTATIVES}
    for triple in [RC.SM16, RC.FUSED, RC.SEQ, ("PACKED", "WIDE", "WIDE"), ("FRAG_QKV", "FRAG_FUSED", "GEMM"), ("PACKED", "GEMM_LN", "ANY"),
                   ("FRAG", "FRAG_GEMM", "GEMM_LN"), ("FRAG_QKV", "FRAG_BLOCK", "SMALL16"), ("ANY_QKV", "ANY", "ANY")]:
        assert triple in have, triple
    assert any(r.case.route["att_fused"] for r in W.REPRESENTATIVES)
    assert {r.case.gemm for r in W.REPRESENTATIVES} == {"h3", "x6", "f32"} and {r.case.attn for r in W.REPRESENTATIVES} == {"h3", "f32"}
    assert any(r.case.evaluator for r in W.REPRESENTATIVES) and any(not r.case.rows_only for r in W.REPRESENTATIVES)
    assert any(r.case.route["nt"] == 8 for r in W.REPRESENTATIVES)


def test_no_representative_needs_more_than_the_cap():
    assert W.MAX_SEQS == 2049
    assert all(r.case.B <= W.MAX_SEQS for r in W.REPRESENTATIVES)
    assert all(W.group_seqs(r.group()) <= W.MAX_SEQS for r in W.REPRESENTATIVES)
    assert len(W.REPRESENTATIVES) <= 48


def test_the_one_tensor_subset_holds_every_kernel_triple():
    sub = W.one_per_kernel_triple()
    want = {W._triple(r) + (r.case.evaluator,) for r in W.REPRESENTATIVES}
    got = [W._triple(r) + (r.case.evaluator,) for r in sub]
    assert set(got) == want and len(got) == len(set(got))
    assert {r.id for r in sub} <= set(W.REP_BY_ID)


def test_groups_and_order():
    order = W.ordered()
    assert sorted(r.id for r in order) == sorted(W.REP_BY_ID)
    seen, last = set(), None
    for r in order:  # one engine group is resident at a time: a group's representatives are adjacent
        if r.group() != last:
            assert r.group() not in seen, r.id
            seen.add(r.group())
            last = r.group()
    assert [r.group() for r in W.groups()] == list(dict.fromkeys(r.group() for r in order))


def test_scoring_cases():
    from influentialrs_amd.engine import shard_bounds
    assert [(n, d) for n, d, _, w in W.SCORING if w == 1] == [(2085, 30), (4097, 128), (9000, 30), (70_001, 128)]
    assert [(n, r, w) for n, _, r, w in W.SCORING if w > 1] == [(70_001, 1, 3)]
    lo, hi = shard_bounds(70_001, 3, 1)
    assert 0 < lo < hi < 70_001  # the shard binds an inner view of the whole tensor
    assert W.SCORING_ROWS == 33 and W.ARENA_UNWRITTEN_MAX == 2048
