"""not-gpu: the workspace's size is part of the C ABI's behaviour (callers allocate irs_workspace_bytes and every buffer's offset
follows from the same walk), so it is pinned for a list of shapes that takes every presence condition of a buffer both ways."""
import ctypes

import pytest

from influentialrs_amd import _lib

BASE = dict(n_item=1000, n_user=10, d=64, max_len=50, n_heads=4, ffn_dim=256, n_layers=6, u_dim=10, mask_mode=0, max_rows=8,
            max_k=100, max_seqs=0)
SEQ = dict(d=128, ffn_dim=256, n_heads=4, max_len=200, n_layers=6)  # the sequence-resident decoder's shape

# (name, dims over BASE, shard (rank, world, item_lo, item_hi) or None, irs_workspace_bytes)
# The sizes were recorded from a build of commit 84e4b27, the last one with a separate plan and binding list.
CASES = [
    ("seq_resident", dict(SEQ, max_rows=64), None, 74077184),
    ("seq_resident_max_seqs", dict(SEQ, max_rows=200, max_seqs=24), None, 40192512),
    ("not_seq_resident", dict(), None, 4174080),
    ("max_seqs_set", dict(max_rows=40, max_seqs=16), None, 7034368),
    ("one_layer_is_not_seq_resident", dict(SEQ, n_layers=1, max_rows=64), None, 70398208),
    ("d256", dict(d=256, ffn_dim=256, max_rows=40, max_seqs=16), None, 12295680),
    ("world2", dict(max_rows=40, max_seqs=16), (1, 2, 500, 1000), 7034624),
    ("shard_262144", dict(n_item=524288), (0, 2, 0, 262144), 20951296),
    ("shard_262143", dict(n_item=524288), (1, 2, 262145, 524288), 4174080),
    ("whole_catalog_300000", dict(n_item=300000, max_rows=33), None, 26803200),
]


def workspace_bytes(dims, shard):
    lib = _lib.load()
    h = ctypes.c_void_p()
    d = _lib.IrsDims(**dict(BASE, **dims))
    sh = ctypes.byref(_lib.IrsShard(*shard)) if shard else None
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(d), sh) == 0, lib.irs_last_error(None)
    try:
        return lib.irs_workspace_bytes(h)
    finally:
        lib.irs_destroy(h)


@pytest.mark.parametrize("name,dims,shard,expected", CASES, ids=[c[0] for c in CASES])
def test_workspace_bytes_are_those_of_the_separate_plan(name, dims, shard, expected):
    assert workspace_bytes(dims, shard) == expected


def test_cases_take_every_presence_condition_both_ways():
    seq = lambda dm: (dm["d"], dm["ffn_dim"], dm["n_heads"]) == (128, 256, 4) and dm["max_len"] <= 256 and dm["n_layers"] > 1
    local = lambda dm, sh: sh[3] - sh[2] if sh else dm["n_item"]
    full = [(dict(BASE, **dm), sh) for _, dm, sh, _ in CASES]
    assert {seq(dm) for dm, _ in full} == {True, False}
    assert {local(dm, sh) >= 262144 for dm, sh in full} == {True, False}
    assert {dm["max_seqs"] > 0 for dm, _ in full} == {True, False}
    assert {sh[1] if sh else 1 for _, sh in full} == {1, 2}
    assert any(dm["d"] == 256 for dm, _ in full)
