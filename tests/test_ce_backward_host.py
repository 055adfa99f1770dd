"""not-gpu: the host side of the fused projection + cross-entropy backward (include/irs_hip.h irs_ce_backward) -- the two
names in header, exports and ctypes table, argument validation before any device work, the IRS_CE_BACKWARD switch, and
the matrix-result hazard scan of the new kernels' ISA."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

from influentialrs_amd import _lib, synth
from influentialrs_amd.model import _backend
from influentialrs_amd.model.influentialRS import InfluentialNet
from influentialrs_amd.model.uRS import SampleNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _ctx(world=1, **kw):
    lib = _lib.load()
    h = ctypes.c_void_p()
    base = dict(n_item=1000, n_user=10, d=30, max_len=60, n_heads=6, ffn_dim=256, n_layers=2, u_dim=10, mask_mode=0,
                max_rows=64, max_k=100, max_seqs=0)
    base.update(kw)
    dims = _lib.IrsDims(**base)
    shard = _lib.IrsShard(0, world, 0, base["n_item"] // world) if world > 1 else None
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), ctypes.byref(shard) if shard else None) == 0
    return lib, h


def test_names_in_header_exports_and_ctypes_table():
    lib = _lib.load()
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("irs_ce_backward_scratch_bytes", 2), ("irs_ce_backward", 13)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, f"{name} not declared"
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), f"{name} not exported"
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.SIGNATURES["irs_ce_backward_scratch_bytes"][0] is ctypes.c_size_t
    # the reference call sites it replaces are cited where the entry point is documented
    assert "influentialRS.py:278-310" in txt and "evaluator.py:53-68" in txt


def test_scratch_size_is_zero_for_an_invalid_row_count():
    lib, h = _ctx()
    try:
        for M in (0, -1, 65, 1 << 30):
            assert lib.irs_ce_backward_scratch_bytes(h, M) == 0, M
        assert lib.irs_ce_backward_scratch_bytes(None, 8) == 0
        a, b = lib.irs_ce_backward_scratch_bytes(h, 1), lib.irs_ce_backward_scratch_bytes(h, 64)
        assert 0 < a <= b <= (64 << 20) + 4 * (64 * 30 + 1000 * 30)
        assert lib.irs_ce_backward_scratch_bytes(h, 64) == b  # a function of the shape alone
    finally:
        lib.irs_destroy(h)


def test_entry_point_validates_before_device_work():
    lib, h = _ctx()
    fake = ctypes.c_void_p(0x10000)
    need = lib.irs_ce_backward_scratch_bytes(h, 8)

    def call(x=fake, lab=fake, lse=fake, M=8, dx=fake, dw=fake, db=fake, scratch=fake, nbytes=need):
        return lib.irs_ce_backward(h, x, lab, lse, M, 1.0, 0, dx, dw, db, scratch, nbytes, None)

    try:
        for kw in (dict(x=None), dict(lab=None), dict(lse=None), dict(dx=None), dict(dw=None), dict(db=None),
                   dict(scratch=None), dict(M=0), dict(M=65), dict(nbytes=need - 1), dict(scratch=ctypes.c_void_p(0x10004)),
                   dict(x=ctypes.c_void_p(0x10004))):
            assert call(**kw) == -1, kw
            assert lib.irs_last_error(h)
        assert lib.irs_ce_backward(None, fake, fake, fake, 8, 1.0, 0, fake, fake, fake, fake, need, None) == -1
        assert call() == -2  # project.* not bound: nothing runs
        assert b"not bound" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)
    lib, h = _ctx(world=2)
    try:
        assert lib.irs_ce_backward(h, fake, fake, fake, 8, 1.0, 0, fake, fake, fake, fake, 1 << 20, None) == -4
        assert b"whole catalog" in lib.irs_last_error(h)
    finally:
        lib.irs_destroy(h)


def test_ce_backward_switch(monkeypatch):
    cfg, ecfg = synth.make_config("tiny"), synth.make_config("eval_tiny")
    monkeypatch.delenv("IRS_CE_BACKWARD", raising=False)
    assert _backend.ce_backward_default() == "chunked"
    assert InfluentialNet(cfg).ce_backward == "chunked" and SampleNet(ecfg).ce_backward == "chunked"
    for v in ("chunked", "fused"):
        monkeypatch.setenv("IRS_CE_BACKWARD", v)
        assert InfluentialNet(cfg).ce_backward == v and SampleNet(ecfg).ce_backward == v
    for v in ("bogus", "", "FUSED", "1"):
        monkeypatch.setenv("IRS_CE_BACKWARD", v)
        with pytest.raises(ValueError, match="IRS_CE_BACKWARD"):
            InfluentialNet(cfg)
        with pytest.raises(ValueError):
            SampleNet(ecfg)
    monkeypatch.delenv("IRS_CE_BACKWARD")
    for net in (InfluentialNet(cfg), SampleNet(ecfg)):
        for v in ("fused", "chunked"):
            net.ce_backward = v
            assert net.ce_backward == v and net._hip.ce_backward == v
        with pytest.raises(ValueError):
            net.ce_backward = "dense"
        assert net.ce_backward == "chunked"
    import copy
    net = InfluentialNet(cfg)
    net.ce_backward = "fused"
    assert copy.deepcopy(net).ce_backward == "fused"


def test_no_matrix_result_is_read_early_behind_a_taken_branch(tmp_path):
    """tools/isa_mfma_branch_scan.py (see tests/test_isa_invariants.py) over every instantiation of the new kernel."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "ce_backward.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "influentialrs_amd", "csrc", "ce_backward.hip"),
                        "-o", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_mfma_branch_scan as scan
    ks = [(n, ins) for n, ins in scan.parse(open(out).read().split("\n")) if any(op and op.startswith("v_mfma") for _, op, _, _ in ins)]
    assert len(ks) == 16, [n for n, _ in ks]  # d_pad 32 / 64 / 128 / 256 x item- / row-owned x 16- / 8-byte staging
    for n, ins in ks:
        assert scan.scan_kernel(n, ins) == 0, n
