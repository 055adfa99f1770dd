"""not-gpu: the probe table and the schedules of tests/engine_state_cases.py.

The GPU module (tests/test_gpu_engine_state.py) can only find what the table reaches: every state holder of a context must be
written by one probe and relied on by another, the all-pairs schedule must really hold every ordered pair, every exported function
that takes a stream must be reached or excused by name, and the stop-at-target probe's windows must make the compaction run."""
import os

import numpy as np

import decoder_route_cases as RC
import engine_state_cases as E
from influentialrs_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_state_holder_is_written_by_one_probe_and_relied_on_by_another():
    probes = E.S_PROBES + E.L_PROBES
    for p in probes:
        assert set(p.writes) <= set(E.HOLDERS) and set(p.relies) <= set(E.HOLDERS), p.id
        assert p.engine in ("S", "L") and p in E.PROBES[p.engine]
    for h in E.HOLDERS:
        for eng in ("S", "L"):  # (a holder lives in one context: writer and reader run on the same engine)
            w = {p.id for p in E.PROBES[eng] if h in p.writes}
            r = {p.id for p in E.PROBES[eng] if h in p.relies}
            if any(a != b for a in w for b in r):
                break
        else:
            raise AssertionError(f"{h}: no probe writes it before ANOTHER probe relies on it")
    assert not set(E.UNPROBED_HOLDERS) & set(E.HOLDERS)
    # the holders are the context's: every name stands in the sources
    src = "".join(open(os.path.join(REPO, "influentialrs_amd", "csrc", f)).read() for f in ("irs_internal.h", "capi.hip", "score.hip"))
    for name in ("step_ctr", "arrive", "fb_count", "cand_cnt", "m_dev", "n_wg_dev", "un_count", "step_pair", "thr_valid", "proj_stale",
                 "surv_rows", "seq_last", "g_greedy", "g_beam", "g_sharded", "tok_row", "act_x", "bm[2]", "un_seq"):
        assert name in src, name


def test_all_pairs_holds_every_ordered_pair():
    for probes in (E.S_PROBES, E.L_PROBES, E.S_PROBES[:1], E.S_PROBES[:2]):
        for seed in (0, 1):
            walk = E.all_pairs(probes, seed)
            n = len(probes)
            assert len(walk) == n * n + 1 and walk[0] is walk[-1]
            pairs = {(a.id, b.id) for a, b in zip(walk, walk[1:])}
            assert pairs == {(a.id, b.id) for a in probes for b in probes}
    a, b = E.all_pairs(E.S_PROBES, 0), E.all_pairs(E.S_PROBES, 1)
    assert [p.id for p in a] != [p.id for p in b]                                       # a function of the seed
    assert [p.id for p in a] == [p.id for p in E.all_pairs(E.S_PROBES, 0)]              # and only of the seed


def test_shuffled_is_seeded_permutations():
    for probes in (E.S_PROBES, E.L_PROBES):
        s = E.shuffled(probes, 5, times=3)
        n = len(probes)
        assert len(s) == 3 * n
        for t in range(3):
            assert sorted(p.id for p in s[t * n:(t + 1) * n]) == sorted(p.id for p in probes)
        assert [p.id for p in s] == [p.id for p in E.shuffled(probes, 5, times=3)]
        assert [p.id for p in s] != [p.id for p in E.shuffled(probes, 6, times=3)]
        assert [p.id for p in s[:n]] != [p.id for p in s[n:2 * n]]


def test_every_stream_function_is_probed_or_excused_by_name():
    with open(os.path.join(REPO, "include", "irs_hip.h")) as fh:
        declared = E.stream_functions(fh.read())
    assert len(declared) >= 35 and "irs_decode" in declared and "irs_bind_workspace" not in declared, declared
    reached = {f for p in E.S_PROBES + E.L_PROBES for f in p.abi}
    assert reached <= set(declared), sorted(reached - set(declared))
    assert not reached & set(E.NOT_PROBED), sorted(reached & set(E.NOT_PROBED))
    missing = sorted(set(declared) - reached - set(E.NOT_PROBED))
    stale = sorted(set(E.NOT_PROBED) - set(declared))
    assert not missing and not stale, f"neither probed nor excused: {missing}; excused but not declared: {stale}"
    assert all(len(why) > 20 for why in E.NOT_PROBED.values())
    sharded = [f for f in declared if "sharded" in f or f in ("irs_allgather_rows", "irs_exchange_topk")]
    assert sharded and all("one GPU" in E.NOT_PROBED[f] for f in sharded)


def test_decode_probes_sit_on_the_table_s_side_of_every_threshold():
    """The decode probes take their routes from decoder_route_cases.py: each B lies between the table's case of that route and the
    next threshold, so a moved threshold fails the table's own case and this probe by name."""
    by = {p.id: p for p in E.S_PROBES}
    b = lambda cid: RC.BY_ID[cid].B  # noqa: E731
    assert by["dec_b1"].case.B == b("c2_b1_att_fused") == 1
    assert b("c2_b2") <= by["dec_b8"].case.B <= b("c2_b64")
    assert b("c2_b65") <= by["dec_b70"].case.B <= b("c2_b163")
    for pid in ("dec_b165_seq1", "dec_b176_seq1", "dec_b176_seq0"):
        assert b("c2_b164") <= by[pid].case.B <= b("c2_b383") and by[pid].case.B <= E.S_ROWS
    assert by["dec_b176_seq1"].case.seq == 1 and by["dec_b176_seq0"].case.seq == 0
    assert by["dec_full_b8"].case.rows_only is False and by["dec_full_b8"].case.B == b("c2_full_b8")
    cfg = E.s_config()
    assert (cfg.n_item, cfg.emb_dim, cfg.max_len, cfg.n_heads, cfg.ffn_dim, cfg.n_layers) == (3415, 128, 200, 4, 256, 2)
    for p in E.S_PROBES:
        if p.kind == "decode":
            assert p.case.route == RC.BY_ID[p.route].route and p.case.config().n_layers == 2
            assert RC.BY_ID[p.route].config().emb_dim == cfg.emb_dim and RC.BY_ID[p.route].config().max_len == cfg.max_len


def test_inputs_are_seeded_and_in_range():
    cfg = E.s_config()
    a, b, c = E.s_inputs(0), E.s_inputs(0), E.s_inputs(1)
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert not np.array_equal(a["win8_seq"], c["win8_seq"])
    for k, v in a.items():
        if k.endswith("_seq"):
            assert v.dtype == np.int64 and v.shape[1] == cfg.max_len and v.min() >= 0 and v.max() <= cfg.n_item, k
        if k.endswith("_usr"):
            assert v.min() >= 0 and v.max() < cfg.n_user, k
        if k.endswith("_pos") or k.endswith("_hep"):
            assert v.dtype == np.int32 and v.min() >= 0 and v.max() < cfg.max_len, k
    for name in ("s8", "s70", "beam"):  # search windows: the target last, the history end in front of it
        assert (a[f"{name}_seq"][:, -1] > 0).all() and (a[f"{name}_hep"] == cfg.max_len - 2).all()
    assert a["gather_ids"].max() < cfg.n_item and a["excl8"].max() < cfg.n_item and a["ce_labels"].min() == -1
    assert not np.array_equal(a["s8_seq"][:2], a["beam_seq"])
    rows = lambda M, d, seed: np.random.default_rng(seed + 100).standard_normal((M, d)).astype(np.float32)  # noqa: E731
    li = E.l_inputs(rows)
    assert li["m288"].shape == (288, E.D) and li["m288"].shape[0] <= E.L_ROWS and li["l_ids"].max() < E.L_ITEMS
    assert np.abs(li["m70_later"] - li["m70"]).max() < 0.2 and E.L_ITEMS >= 524288


def test_until_windows_make_the_compaction_run(oracle):
    """At least two and not all of the users reach their target before step 6 under oracle.get_seq, at different steps."""
    cfg = E.s_config()
    sd = synth.irn_state_dict(cfg, 2027)
    seqs, users, targets, arrive = E.until_windows(oracle, sd, cfg)
    assert seqs.shape == (8, cfg.max_len) and np.array_equal(seqs[:, -1], targets)
    early = arrive[(arrive >= 0) & (arrive < E.P_UNTIL - 1)]
    assert 2 <= len(early) < 8, arrive
    assert len(set(early.tolist())) >= 2, arrive  # (users leave at different checks: more than one compaction)
    for b in range(8):  # a target never sits in its own history
        assert targets[b] not in seqs[b, :-1]
