"""Compile-time check that the sequence-resident decoder launch does not wait for global memory one round trip at a time where
the program asks for no such thing (no GPU needed: hipcc -S, tools/isa_vm_drain_scan.py).

A `s_waitcnt vmcnt` the COMPILER writes stands in front of an operation it tracks itself; a chain of them is a chain of dependent
round trips.  Two phases of k_block_x6<3, 8, false, 4, 2, SEQ = true> store sixteen 16-byte pieces of a token tile: the prologue
(the embedded tokens, layer 0's residual) and LayerNorm 3 (x').  Before the batched form the first held 22 compiler-written vmcnt
waits (a pair of row pieces per round trip: the store of piece i may alias the tables) and the second 17 (one in front of every
store: the address came back from scratch inside an `if (a.Xf)` block, and stores count in vmcnt on gfx9).  Now every batch of
loads is inline asm with one wait that names its registers, the stores are inline asm, and what is left to the compiler is the
load of the item id in the prologue and a scratch reload in LayerNorm 3."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "influentialrs_amd", "csrc", "decoder.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SEQ_KERNEL = "_Z10k_block_x6ILi3ELi8ELb0ELi4ELi2ELb1EEv11BlockX6Args"
MAX_WAITS = 2  # compiler-written vmcnt waits in a segment that stores a token tile


@pytest.fixture(scope="module")
def seq_segments(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = os.path.join(tmp_path_factory.mktemp("isa_rt"), "decoder.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-I" + os.path.join(REPO, "include"),
                        SRC, "-o", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_pending_read_scan as pending
    import isa_vm_drain_scan as drain
    lines = open(out).read().split("\n")
    body = drain.kernel_lines(lines, SEQ_KERNEL)  # (the whole function: the idle waves' path ends in an s_endpgm of its own)
    assert len(body) > 20000 and sum(l.strip().startswith("s_barrier") for l in body) == 76, len(body)
    return body, drain.segments(body), pending


def test_tile_store_segments_wait_at_most_twice(seq_segments):
    _, segs, _ = seq_segments
    tiles = [s for s in segs if s["st128"] >= 16]
    for s in tiles:
        print(f"segment at line {s['line']}: {s['st128']} global_store_dwordx4, compiler-written vmcnt waits {s['waits']}, in asm {s['asm_waits']}")
    assert len(tiles) == 2, [(s["line"], s["st128"]) for s in segs if s["st128"]]  # the prologue and LayerNorm 3
    for s in tiles:
        assert s["st128"] == 16, s
        assert len(s["waits"]) <= MAX_WAITS, s


def test_batched_loads_are_waited_for_before_they_are_used(seq_segments):
    """the new inline-asm loads (parameter vectors, row index, 32 row pieces) are pending registers the compiler does not know of"""
    body, segs, pending = seq_segments
    assert pending.scan(body) == 0
    prologue = next(s for s in segs if s["st128"] >= 16)
    assert prologue["gld"] >= 32 + 5 + 1, prologue  # the gather's pieces, the vectors, the row index: all in the one segment
