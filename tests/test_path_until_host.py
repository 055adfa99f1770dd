"""not-gpu: the stop-at-target search is declared, bound with the declared arguments, and the front end refuses what
is not built before it touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from influentialrs_amd import _lib, synth
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declaration(name):
    txt = open(os.path.join(REPO, "include", "irs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/irs_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_is_declared_exported_and_bound_with_its_arguments():
    args = _declaration("irs_generate_paths_until")
    plain = _declaration("irs_generate_paths")
    # the arguments of irs_generate_paths without use_graph, plus check_every and host_stats
    names = [a.split()[-1].lstrip("*") for a in args]
    plain_names = [a.split()[-1].lstrip("*") for a in plain]
    assert [n for n in names if n not in ("check_every", "host_stats")] == [n for n in plain_names if n != "use_graph"]
    assert "int32_t check_every" in args and any(re.fullmatch(r"int64_t\s*\*\s*host_stats", a) for a in args)
    res, argtypes = _lib.SIGNATURES["irs_generate_paths_until"]
    assert res is ctypes.c_int32 and len(argtypes) == len(args) == 16
    assert argtypes[names.index("check_every")] is ctypes.c_int32
    assert argtypes[names.index("seed")] is ctypes.c_uint64
    assert argtypes[names.index("host_stats")] is ctypes.POINTER(ctypes.c_int64)
    lib = _lib.load()
    assert hasattr(lib, "irs_generate_paths_until")
    # no context: refused like every other entry, nothing touched
    assert lib.irs_generate_paths_until(None, None, None, None, 1, 1, 1, 0, 0, 0, 0, 1, None, None, None, None) < 0


def test_stop_at_target_with_beams_is_refused_without_a_device():
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg)
    irn = IRSNN(cfg, net, "cpu")
    B, L = 2, cfg.max_len
    seqs = torch.ones((B, L), dtype=torch.int64)
    users = torch.zeros(B, dtype=torch.int64)
    targets = torch.ones(B, dtype=torch.int64)
    with pytest.raises(ValueError, match="beam"):
        irn.get_seq_in_batch(seqs, users, targets, 5, 0, beam_width=2, stop_at_target=True)
    # the keyword defaults to the search as it was
    import inspect
    assert inspect.signature(IRSNN.get_seq_in_batch).parameters["stop_at_target"].default is False
    assert np.array_equal(seqs.numpy(), np.ones((B, L), dtype=np.int64))


def test_harness_passes_the_keyword_only_when_the_config_sets_it():
    """A handler written against the reference's signature (no stop_at_target keyword) keeps working while the config
    leaves the switch off; with the switch on the keyword reaches the handler."""
    from influentialrs_amd import harness
    cfg = synth.make_config("tiny")
    for k, v in dict(gap_len=0, batch_size=2, top_k=5, use_h=False, max_path_len=3, sample=False, sample_k=3).items():
        setattr(cfg, k, v)
    rows = [(np.array([1, 2, 3]), 0, 9, 4), (np.array([2, 5]), 1, 8, 6)]
    seen = []

    class Handler:
        def eval(self):
            pass

        def get_pif_in_batch(self, seq, u):
            return np.zeros((seq.shape[0], 1), dtype=np.float32)

        def get_accuracy_metrics_in_batch(self, raw, seq, u, t, l, top_k, gap_len, use_h):
            return 0, np.ones(seq.shape[0])

        def get_seq_in_batch(self, seq, u, t, max_path_len, gap_len, sample, sample_k, **kw):
            seen.append(kw)
            B = seq.shape[0]
            return np.zeros((B, max_path_len), dtype=np.float32), t.numpy(), [np.array([1])] * B, 0

    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    assert seen == [{}]
    cfg.stop_at_target = True
    harness.test_model(cfg, rows, Handler(), "cpu", verbose=False)
    assert seen == [{}, {"stop_at_target": True}]
