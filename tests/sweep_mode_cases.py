"""The float32 catalog sweep's launch geometry as a table of cases (test infrastructure, shared by tests/test_sweep_mode_cases.py
on the CPU and tests/test_gpu_sweep_modes.py on the GPU).

k_sweep_f32 and its log-sum-exp siblings (k_lse_f32, k_lse_ring) in influentialrs_amd/csrc/score.hip serve every scoring entry
point that is not the top-k: dense logits, count-before, log-sum-exp, the cross entropy's forward and gradient, the path trace.
geometry() restates, as plain arithmetic, how their launchers cut a call of M rows over a catalog of n_item items of width d into
workgroups; CASES names (n_item, d, M) so that every row-block cell of every width class is reached.  If a threshold in score.hip
moves (UB of ub_f32, the vector-staging predicate, the log-sum-exp forms), the constants restated HERE are what a reviewer updates,
and tests/test_sweep_mode_cases.py says which cell the table no longer reaches."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

D_PADS = (16, 32, 64, 128, 256)
TARGET_WGS = 2048    # sweep_decompose's default target_wgs
MAX_TPW = 16         # sweep_decompose's default max_tpw
LSE_SLOTS = 2048     # ctx->lse_slots (irs_create): (max, sum) partial slots of the register-form sweeps
LSE_SLOTS_RING = 4096  # IRS_LSE_SLOTS_RING (irs_internal.h)
MAX_ROWS = 520       # the table's limits (tests/test_sweep_mode_cases.py): a few row blocks and a few thousand items keep
MAX_ITEMS = 4097     # every GPU case within seconds; large catalogs and the top-k are covered by tests/test_gpu_scoring.py


def d_pad_of(d: int) -> int:
    """irs_create: the smallest power of two >= max(d, 16)."""
    dp = 16
    while dp < d:
        dp <<= 1
    assert dp in D_PADS, d
    return dp


def ub_f32(KS: int) -> int:
    """ub_f32: row tiles of 32 rows one workgroup of k_sweep_f32 / k_lse_f32 owns."""
    return 2 if KS >= 16 else 4 if KS >= 8 else 8


def shard_bounds(n_item: int, world: int, rank: int) -> Tuple[int, int]:
    """influentialrs_amd.engine.shard_bounds, restated so that this file needs no GPU library."""
    tiles = (n_item + 31) // 32
    per, rem = divmod(tiles, world)
    lo_t = rank * per + min(rank, rem)
    hi_t = lo_t + per + (1 if rank < rem else 0)
    return min(lo_t * 32, n_item), min(hi_t * 32, n_item)


def geometry(n_item: int, d: int, M: int, aligned: bool = True, lse_ring: bool = True) -> Dict[str, object]:
    """The launch of one float32 sweep over a whole (unsharded) catalog.  aligned: xrows is 16-byte aligned (project.weight
    always is: torch allocations are).  lse_ring: the context was not created under IRS_LSE_RING=0."""
    d_pad = d_pad_of(d)                      # irs_create
    KS = d_pad // 16                         # irs_create
    UB = ub_f32(KS)                          # ub_f32
    M_pad = (M + 31) & ~31                   # sweep_common
    UT = M_pad // 32                         # sweep_common: ceil(M / 32)
    n_ublocks = (UT + UB - 1) // UB          # launch_sweep_f32 (and sweep_f32_whole's hint)
    vec = d % 8 == 0 and d == d_pad          # launch_sweep_f32 (the weights' alignment holds)
    n_tiles = (n_item + 31) // 32            # irs_create
    # sweep_decompose with its defaults, as sweep_f32_whole calls it (dense, count-before, CE gradient)
    t = (n_tiles * n_ublocks) // (4 * TARGET_WGS)
    tpw = min(max(t, 1), MAX_TPW)
    n_strips = max((n_tiles + 4 * tpw - 1) // (4 * tpw), 1)
    grid = (n_strips + 7) // 8 * 8 * n_ublocks  # launch_sweep_f32: strips round up to a multiple of 8 (sweep_map drops the rest)
    # lse_fast_ok / lse_ring_ok / launch_lse_f32
    fast = KS >= 2 and d == d_pad and aligned
    if not fast:
        lse_form = "generic"                 # irs_launch_lse: launch_sweep_f32<MODE_LSE>
    elif UT == 1 and KS in (8, 16) and lse_ring:
        lse_form = "ring"                    # k_lse_ring
    elif UT == 1 and KS == 16:
        lse_form = "xreg"                    # k_lse_f32<16, 1, ., XREG>
    else:
        lse_form = "fast"                    # k_lse_f32<KS, UB>
    # lse_decompose: tiles per wave from the slot budget (also the path trace's decomposition, with LSE_SLOTS)
    waves = (LSE_SLOTS_RING if lse_form == "ring" else LSE_SLOTS) // 2
    lse_tpw = max((n_tiles + waves - 1) // waves, 1)
    lse_strips = max((n_tiles + 4 * lse_tpw - 1) // (4 * lse_tpw), 1)
    return dict(d_pad=d_pad, KS=KS, UB=UB, M_pad=M_pad, UT=UT, n_ublocks=n_ublocks, vec=vec, n_tiles=n_tiles, tpw=tpw,
                n_strips=n_strips, grid=grid, dead_strips=(n_strips + 7) // 8 * 8 - n_strips, last_tile_items=n_item - 32 * (n_tiles - 1),
                last_block_rows=M - 32 * UB * (n_ublocks - 1), lse_form=lse_form, lse_strips=lse_strips,
                lse_slots=lse_strips * 8)


@dataclass(frozen=True)
class Case:
    n_item: int
    d: int
    M: int
    shards: bool = False    # also run on world = 3 item shards
    trace: bool = False     # also run irs_score_target_trace's sweep test at this shape

    @property
    def id(self) -> str:
        return f"n{self.n_item}_d{self.d}_m{self.M}"

    def geometry(self, **kw):
        return geometry(self.n_item, self.d, self.M, **kw)


N_A, N_B, N_TINY = 2085, 4097, 37  # 66 tiles (5 items in the last), 17 strips; 129 tiles (1 item in the last), 33 strips; below one strip

CASES = [
    # ---- KS 1 (d_pad 16, UB 8: 256 rows per workgroup); d = 16 vector staging, 8 and 6 scalar
    Case(N_A, 16, 256), Case(N_B, 16, 257), Case(N_A, 16, 520), Case(N_TINY, 16, 33),
    Case(N_A, 8, 257), Case(N_B, 6, 33),
    # ---- KS 2 (d_pad 32, UB 8); 30 (the reference's default width) and 24 scalar
    Case(N_B, 32, 256), Case(N_A, 32, 257, trace=True), Case(N_A, 32, 520, trace=True), Case(N_A, 32, 33),
    Case(N_A, 30, 257, shards=True), Case(N_B, 24, 33), Case(N_TINY, 30, 520),
    # ---- KS 4 (d_pad 64, UB 8); 40 scalar
    Case(N_A, 64, 256), Case(N_B, 64, 257), Case(N_A, 64, 520), Case(N_TINY, 64, 33),
    Case(N_A, 40, 257), Case(N_B, 40, 33),
    # ---- KS 8 (d_pad 128, UB 4: 128 rows per workgroup); 96 scalar; 32 rows: the ring log-sum-exp
    Case(N_A, 128, 128), Case(N_B, 128, 129, shards=True, trace=True), Case(N_A, 128, 260, trace=True), Case(N_A, 128, 33),
    Case(N_A, 96, 129), Case(N_B, 96, 33), Case(N_TINY, 128, 260), Case(N_A, 128, 32),
    # ---- KS 16 (d_pad 256, UB 2: 64 rows per workgroup); 160 and 192 scalar
    Case(N_A, 256, 64), Case(N_B, 256, 65, shards=True, trace=True), Case(N_A, 256, 130, trace=True), Case(N_A, 256, 33),
    Case(N_A, 160, 65), Case(N_B, 192, 130), Case(N_A, 192, 33), Case(N_TINY, 256, 65), Case(N_B, 256, 7),
]

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case ids"

KS_ALL = (1, 2, 4, 8, 16)
# widths that must take the scalar staging (vec == False), per KS
NON_VECTOR_WIDTHS = {1: (8, 6), 2: (30, 24), 4: (40,), 8: (96,), 16: (160, 192)}
WORLD = 3  # the sharded cases


def misaligned_lse_cases():
    """One case per KS >= 2 whose aligned log-sum-exp takes a 16-byte-fragment form (fast): the same rows passed 4 bytes into their
    buffer fail lse_fast_ok and run the generic sweep.  More than one row block each."""
    out = []
    for KS in KS_ALL[1:]:
        c = next(c for c in CASES if c.geometry()["KS"] == KS and c.geometry()["lse_form"] == "fast" and c.geometry()["n_ublocks"] == 2)
        out.append(c)
    return out
