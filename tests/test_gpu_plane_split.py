"""gpu: the float16 plane-split helper (influentialrs_amd/csrc/plane_split.h: one packed conversion and two mixed fmas per
value pair) gives the bits of the plain statement h = (_Float16)v, l = (_Float16)(v - (float)h) for every finite float32.

tests/plane_split_check.hip is a stand-alone program: on the device it runs both forms over all 2^32 float32 patterns, each
pattern once in each half of the pair -- every exponent from 2^-149 to 2^15 and beyond with every mantissa, both signs, +-0, the
2^16 exact float16 values, the whole of |v| < 2^-2 (where l is a float16 subnormal or zero: an output-denormal difference
would show there) and everything up to 32752, the bound irs_finalize_weights enforces.  Requirement: no finite pattern
differs; for +-inf and NaN inputs a plane may differ only where both forms give a NaN."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.gpu
def test_split_helper_equals_the_plain_statement_on_every_float32(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "plane_split_check")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-I" + os.path.join(REPO, "influentialrs_amd", "csrc"),
                        os.path.join(REPO, "tests", "plane_split_check.hip"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout.strip())
    m = re.search(r"^plane_split_check patterns=(\d+) slots=2 finite_diff=(\d+) nonfinite_bad=(\d+) first=(\S*)$", r.stdout, re.M)
    assert m, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert int(m.group(1)) == 1 << 32
    assert int(m.group(2)) == 0, f"finite float32 patterns whose planes differ, the first of them: {m.group(4)}"
    assert int(m.group(3)) == 0, "a plane of an inf / NaN input that is neither equal nor NaN in both forms"
    assert r.returncode == 0
