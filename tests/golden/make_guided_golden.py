#!/usr/bin/env python3
"""Generate tests/golden/guided_choice.npz: what the UNMODIFIED reference chooses among a short candidate list, by its own
distance function -- np.argsort([cal_fv_dist(c, target, fv, binary) for c in candidates])[0], the line of get_path
(main_baselines.py:111-112) with utils.cal_fv_dist (utils.py:202-206).

Runs only where the reference is mounted (like make_golden.py); only the arrays written here are committed.  utils.py imports
pandas and sklearn at module level for functions that are not called here: whichever is not installed is shimmed in
sys.modules with an empty module, no reference file is touched.

Groups (one feature table each, rows = 1-based items, row 0 unused):
  binary 18 bits, few distinct rows   -> many exact ties
  float F = 1, 3, 64, small integers and dyadic values -> the float64 norm and the float32 squared chain order the
                                         candidates identically, ties included (every partial sum is exact in float32)
For each group: rows of (candidates padded with 0 to 32, their count 1 .. 32, target, the reference's chosen index).

Two chosen indices are recorded.  `chosen` is the reference's line verbatim.  np.argsort's default kind is not stable: the numpy
the reference pins (1.23) sorts up to 16 elements by insertion, which keeps the first of equal distances, but a numpy with SIMD
sorting returns any of them, at every length.  `chosen_stable` is the same line with kind="stable": the first of the nearest,
which is what the library defines (include/irs_hip.h) and what the pinned numpy returns for the default k_c = 5.  The two differ
only inside an exact tie; tests/test_guided_host.py checks exactly that.

Usage:  python tests/golden/make_guided_golden.py
"""
import importlib
import os
import sys
import types

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "guided_choice.npz")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

for name in ("pandas", "sklearn", "sklearn.preprocessing"):
    try:
        importlib.import_module(name)
    except ImportError:
        mod = types.ModuleType(name)
        if name == "sklearn.preprocessing":
            mod.Normalizer = object
        sys.modules[name] = mod

from utils import cal_fv_dist  # noqa: E402  (reference)

ROWS, PER_GROUP, MAX_C = 48, 96, 32


def tables(rng):
    protos = rng.integers(0, 2, size=(6, 18))
    binary = protos[rng.integers(0, 6, size=ROWS)].copy()
    flip = rng.random(ROWS) < 0.3
    binary[flip, rng.integers(0, 18, size=int(flip.sum()))] ^= 1
    out = [("bin18", True, binary.astype(np.int64))]
    out.append(("f1", False, rng.integers(-4, 5, size=(ROWS, 1)).astype(np.float32)))
    out.append(("f3", False, (rng.integers(-8, 9, size=(ROWS, 3)) * 0.25).astype(np.float32)))
    out.append(("f64", False, (rng.integers(-2, 3, size=(ROWS, 64)) * 0.5).astype(np.float32)))
    return out


def main():
    rng = np.random.default_rng(20240)
    arrays = {}
    for name, binary, table in tables(rng):
        fv = {i: table[i] for i in range(1, ROWS)}
        cands = np.zeros((PER_GROUP, MAX_C), dtype=np.int64)
        count = np.zeros(PER_GROUP, dtype=np.int32)
        target = np.zeros(PER_GROUP, dtype=np.int64)
        chosen = np.zeros(PER_GROUP, dtype=np.int32)
        stable = np.zeros(PER_GROUP, dtype=np.int32)
        for r in range(PER_GROUP):
            n = 1 + r % MAX_C
            items = rng.choice(np.arange(1, ROWS), size=n, replace=False)
            t = int(rng.integers(1, ROWS)) if r % 3 else int(items[rng.integers(0, n)])  # every third row: the target is offered
            dists = np.array([cal_fv_dist(k, t, fv, binary) for k in items])
            cands[r, :n], count[r], target[r], chosen[r] = items, n, t, np.argsort(dists)[0]
            stable[r] = np.argsort(dists, kind="stable")[0]
        arrays.update({f"{name}_table": table, f"{name}_cands": cands, f"{name}_count": count, f"{name}_target": target,
                       f"{name}_chosen": chosen, f"{name}_chosen_stable": stable})
    np.savez_compressed(OUT, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
