"""not-gpu: the float32 sweep's case table (tests/sweep_mode_cases.py) reaches every cell of the launchers' geometry that
tests/test_gpu_sweep_modes.py is there to run, and stays small.

Every cell is computed with sweep_mode_cases.geometry(), the restatement of launch_sweep_f32 / sweep_common / ub_f32 /
sweep_decompose / lse_fast_ok / lse_ring_ok / launch_lse_f32 (influentialrs_amd/csrc/score.hip); nothing is written down by hand.
If a threshold in score.hip moves, the constants restated in sweep_mode_cases.py are what a reviewer updates; this file then names
the cell the table lost.  The restated constants are compared with the source text below, so a moved threshold fails here first."""
import os
import re

import pytest

import sweep_mode_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE = os.path.join(REPO, "influentialrs_amd", "csrc", "score.hip")
CAPI = os.path.join(REPO, "influentialrs_amd", "csrc", "capi.hip")
INTERNAL = os.path.join(REPO, "influentialrs_amd", "csrc", "irs_internal.h")

GEO = [(c, c.geometry()) for c in C.CASES]


def _read(path):
    with open(path) as fh:
        return fh.read()


def _cells(KS):
    return [(c, g) for c, g in GEO if g["KS"] == KS]


def test_restated_constants_match_the_source():
    src = _read(SCORE)
    m = re.search(r"static inline int ub_f32\(int KS\) \{ return KS >= 16 \? (\d+) : KS >= 8 \? (\d+) : (\d+); \}", src)
    assert m, "ub_f32 not found in score.hip"
    assert tuple(int(v) for v in m.groups()) == (C.ub_f32(16), C.ub_f32(8), C.ub_f32(4)) and C.ub_f32(1) == C.ub_f32(2) == C.ub_f32(4)
    m = re.search(r"int target_wgs = (\d+), int max_tpw = (\d+)\);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (C.TARGET_WGS, C.MAX_TPW)
    assert "const bool vec = (a.d % 8 == 0) && (a.d == KS * 16) && ((((uintptr_t)a.w32) & 15) == 0);" in src
    assert ("return ctx->KS >= 2 && a.d == ctx->KS * 16 && ((((uintptr_t)a.w32) & 15) == 0) && ((((uintptr_t)a.x32) & 15) == 0);"
            in src), "lse_fast_ok"
    assert "return a.UT == 1 && (ctx->KS == 16 || ctx->KS == 8) && !ctx->lse_no_ring && lse_fast_ok(ctx, a);" in src, "lse_ring_ok"
    assert "const bool xreg = a.UT == 1 && KS == 16;" in src
    m = re.search(r"c->lse_slots = (\d+);", _read(CAPI))
    assert m and int(m.group(1)) == C.LSE_SLOTS
    m = re.search(r"#define IRS_LSE_SLOTS_RING (\d+)", _read(INTERNAL))
    assert m and int(m.group(1)) == C.LSE_SLOTS_RING


def test_geometry_of_the_catalogs():
    g = C.geometry(C.N_A, 32, 33)
    assert (g["n_tiles"], g["last_tile_items"], g["n_strips"], g["dead_strips"]) == (66, 5, 17, 7)
    g = C.geometry(C.N_B, 32, 33)
    assert (g["n_tiles"], g["last_tile_items"], g["n_strips"]) == (129, 1, 33) and g["dead_strips"] > 0
    g = C.geometry(C.N_TINY, 32, 33)
    assert g["n_tiles"] == 2 and g["n_strips"] == 1
    assert {c.n_item for c in C.CASES} == {C.N_A, C.N_B, C.N_TINY}


def test_geometry_lse_forms():
    assert C.geometry(4097, 16, 300)["lse_form"] == "generic"            # KS 1 never loads 16-byte fragments
    assert C.geometry(4097, 30, 300)["lse_form"] == "generic"            # d != d_pad
    assert C.geometry(4097, 32, 300)["lse_form"] == "fast"
    assert C.geometry(4097, 32, 300, aligned=False)["lse_form"] == "generic"
    assert C.geometry(4097, 32, 32)["lse_form"] == "fast"                # one row tile, but no ring below d_pad = 128
    assert C.geometry(4097, 128, 32)["lse_form"] == "ring" and C.geometry(4097, 256, 1)["lse_form"] == "ring"
    assert C.geometry(4097, 128, 33)["lse_form"] == "fast"
    assert C.geometry(4097, 256, 32, lse_ring=False)["lse_form"] == "xreg"
    assert C.geometry(4097, 128, 32, lse_ring=False)["lse_form"] == "fast"
    assert C.geometry(4097, 256, 32, aligned=False)["lse_form"] == "generic"


@pytest.mark.parametrize("KS", C.KS_ALL)
def test_every_row_block_cell_is_reached(KS):
    cells = _cells(KS)
    assert cells, f"no case at KS {KS}"
    UB = C.ub_f32(KS)
    assert all(g["UB"] == UB for _, g in cells)
    # one full block, exactly
    assert any(g["n_ublocks"] == 1 and c.M == 32 * UB for c, g in cells), f"KS {KS}: no case with M = 32 UB"
    # two blocks, one row in the last
    assert any(g["n_ublocks"] == 2 and g["last_block_rows"] == 1 and c.M == 32 * UB + 1 for c, g in cells), f"KS {KS}: no M = 32 UB + 1"
    # three blocks, the last ragged (neither full nor a whole number of row tiles)
    assert any(g["n_ublocks"] == 3 and g["last_block_rows"] % 32 != 0 for c, g in cells), f"KS {KS}: no ragged third block"
    # two row tiles, the second holding one row
    assert any(c.M == 33 and g["M_pad"] == 64 and g["UT"] == 2 for c, g in cells), f"KS {KS}: no M = 33"
    # both stagings; more than one row block under each
    for vec in (True, False):
        assert any(g["vec"] == vec for _, g in cells), f"KS {KS}: vec = {vec} not reached"
        assert any(g["vec"] == vec and g["n_ublocks"] >= 2 for _, g in cells), f"KS {KS}: vec = {vec} only inside one row block"
    widths = {c.d for c, g in cells if not g["vec"]}
    assert set(C.NON_VECTOR_WIDTHS[KS]) <= widths, f"KS {KS}: scalar-staging widths {C.NON_VECTOR_WIDTHS[KS]}, table has {sorted(widths)}"
    assert {c.d for c, g in cells if g["vec"]} == {16 * KS}
    # catalogs: ragged last tile, dead strips in the grid's round-up, and one below a strip
    assert any(g["dead_strips"] > 0 and g["last_tile_items"] < 32 and g["n_ublocks"] >= 2 for _, g in cells)
    assert {C.N_A, C.N_B} <= {c.n_item for c, _ in cells}


def test_one_strip_catalog_under_several_row_blocks():
    tiny = [(c, g) for c, g in GEO if c.n_item == C.N_TINY]
    assert all(g["n_strips"] == 1 and g["dead_strips"] == 7 for _, g in tiny)
    assert any(g["n_ublocks"] >= 2 for _, g in tiny) and any(g["n_ublocks"] == 1 for _, g in tiny)


def test_lse_forms_of_the_table():
    forms = {g["lse_form"] for _, g in GEO}
    assert {"generic", "fast", "ring"} <= forms  # xreg exists only under IRS_LSE_RING=0 (test_lse_ring_equals_register_form)
    for KS in C.KS_ALL:
        assert any(g["lse_form"] == "generic" and g["n_ublocks"] >= 2 for _, g in _cells(KS)), KS
    for KS in C.KS_ALL[1:]:
        assert any(g["lse_form"] == "fast" and g["n_ublocks"] == 3 for _, g in _cells(KS)), KS
    mis = C.misaligned_lse_cases()
    assert [c.geometry()["KS"] for c in mis] == list(C.KS_ALL[1:])
    for c in mis:
        g = c.geometry(aligned=False)
        assert c.geometry()["lse_form"] == "fast" and g["lse_form"] == "generic" and g["vec"] and g["n_ublocks"] == 2
    # the slot budget is never exceeded (lse_decompose refuses otherwise)
    assert all(g["lse_slots"] <= (C.LSE_SLOTS_RING if g["lse_form"] == "ring" else C.LSE_SLOTS) for _, g in GEO)


def test_sharded_and_trace_cases():
    sh = [(c, c.geometry()) for c in C.CASES if c.shards]
    assert sorted(g["KS"] for _, g in sh) == [2, 8, 16]
    assert all(g["n_ublocks"] == 2 for _, g in sh)
    assert not next(g for _, g in sh if g["KS"] == 2)["vec"]
    for c, _ in sh:
        bounds = [C.shard_bounds(c.n_item, C.WORLD, r) for r in range(C.WORLD)]
        assert bounds[0][0] == 0 and bounds[-1][1] == c.n_item and all(bounds[r][1] == bounds[r + 1][0] for r in range(C.WORLD - 1))
        assert all(hi > lo for lo, hi in bounds) and (bounds[-1][1] - bounds[-1][0]) % 32 != 0  # a ragged last shard
    tr = sorted((c.geometry()["KS"], c.geometry()["n_ublocks"]) for c in C.CASES if c.trace)
    assert tr == [(KS, n) for KS in (2, 8, 16) for n in (2, 3)]
    assert all(c.geometry()["n_strips"] >= 2 for c in C.CASES if c.trace)


def test_shard_bounds_restated():
    from influentialrs_amd import engine
    for n in (C.N_A, C.N_B, C.N_TINY, 100, 3415):
        for world in (1, 2, 3, 8):
            for r in range(world):
                assert C.shard_bounds(n, world, r) == engine.shard_bounds(n, world, r)


def test_cases_stay_small():
    assert all(c.M <= C.MAX_ROWS == 520 for c in C.CASES)
    assert all(c.n_item <= C.MAX_ITEMS == 4097 for c in C.CASES)
    assert len(C.CASES) <= 40
