"""not-gpu: the native training trunk's host side -- argument validation of irs_train_* before any device work, the
IRS_TRAIN_TRUNK switch, and the numpy restatement of the dropout generator (include/irs_hip.h) the GPU tests rebuild
masks with."""
import ctypes
import math

import numpy as np
import pytest
import torch

from influentialrs_amd import _lib, synth
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model import _backend
from influentialrs_amd.model.influentialRS import InfluentialNet
from influentialrs_amd.model.uRS import SampleNet

from train_trunk_ref import drop_mult, keep_words, philox4x32_10


@pytest.fixture()
def ctx():
    lib = _lib.load()
    h = ctypes.c_void_p()
    dims = _lib.IrsDims(n_item=1000, n_user=10, d=30, max_len=60, n_heads=6, ffn_dim=256, n_layers=2, u_dim=10, mask_mode=0,
                        max_rows=8, max_k=100, max_seqs=0)
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), None) == 0
    yield lib, h
    lib.irs_destroy(h)


def test_saved_state_and_gradient_layout(ctx):
    lib, h = ctx
    assert lib.irs_train_saved_bytes(h, 4, 0) == 0 and lib.irs_train_saved_bytes(h, 4, 61) == 0
    assert lib.irs_train_saved_bytes(h, 0, 10) == 0 and lib.irs_train_saved_bytes(h, (1 << 22) // 60 + 1, 60) == 0
    a, b = lib.irs_train_saved_bytes(h, 4, 60), lib.irs_train_saved_bytes(h, 8, 60)
    assert 0 < a < b and a % 256 == 0
    assert lib.irs_train_grad_offset(h, b"item_embedder.weight") == 0
    assert lib.irs_train_grad_offset(h, b"word_embedder.weight") == 0
    offs = [lib.irs_train_grad_offset(h, f"decoder.layers.{l}.{n}".encode()) for l in range(2) for n in
            ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "norm3.bias")]
    assert all(o > 0 and o % 64 == 0 for o in offs) and offs == sorted(offs)
    assert offs[0] >= 1001 * 30 and offs[1] - offs[0] >= 3 * 30 * 30
    assert lib.irs_train_grad_offset(h, b"module.decoder.layers.1.norm3.bias") == offs[-1]
    for bad in (b"decoder.layers.2.norm3.bias", b"project.weight", b"user_embedder.weight", b"pos_embedder.pe", b"x"):
        assert lib.irs_train_grad_offset(h, bad) == -1, bad
    assert lib.irs_train_grad_bytes(h) >= 4 * (offs[-1] + 30)


def test_entry_points_validate_before_device_work(ctx):
    lib, h = ctx
    fake = ctypes.c_void_p(0x10000)
    need = lib.irs_train_saved_bytes(h, 4, 60)

    def fwd(seq=fake, user=fake, B=4, L=60, p=0.0, saved=fake, nbytes=need, x=fake):
        return lib.irs_train_forward(h, seq, user, B, L, p, 7, saved, nbytes, x, None)

    for kw in (dict(seq=None), dict(user=None), dict(B=0), dict(L=0), dict(L=61), dict(p=-0.1), dict(p=1.0),
               dict(p=float("nan")), dict(saved=None), dict(nbytes=need - 1), dict(saved=ctypes.c_void_p(0x10004))):
        assert fwd(**kw) == -1, kw
        assert lib.irs_last_error(h)
    assert fwd() == -2  # weights not bound: nothing runs
    assert b"not bound" in lib.irs_last_error(h)
    names = ["item_embedder.weight", "user_embedder.weight", "pos_embedder.pe", "user_mask_layer.weight",
             "user_mask_layer.bias"]
    numel = {"item_embedder.weight": 1001 * 30, "user_embedder.weight": 100, "pos_embedder.pe": 60 * 30,
             "user_mask_layer.weight": 10, "user_mask_layer.bias": 1}
    for l in range(2):
        for n, k in (("self_attn.in_proj_weight", 2700), ("self_attn.in_proj_bias", 90), ("self_attn.out_proj.weight", 900),
                     ("self_attn.out_proj.bias", 30), ("multihead_attn.in_proj_weight", 2700),
                     ("multihead_attn.in_proj_bias", 90), ("multihead_attn.out_proj.weight", 900),
                     ("multihead_attn.out_proj.bias", 30), ("linear1.weight", 7680), ("linear1.bias", 256),
                     ("linear2.weight", 7680), ("linear2.bias", 30), ("norm1.weight", 30), ("norm1.bias", 30),
                     ("norm2.weight", 30), ("norm2.bias", 30), ("norm3.weight", 30), ("norm3.bias", 30)):
            names.append(f"decoder.layers.{l}.{n}")
            numel[names[-1]] = k
    for n in names:
        assert lib.irs_bind_weight(h, n.encode(), fake, numel[n]) == 0, n
    assert fwd(x=None) == -1  # x_out is checked once the weights are bound
    gb = lib.irs_train_grad_bytes(h)

    def bwd(dx=fake, grads=fake, gbytes=gb, p=0.0):
        return lib.irs_train_backward(h, fake, fake, 4, 60, p, 7, fake, need, dx, grads, gbytes, None)

    for kw in (dict(dx=None), dict(grads=None), dict(gbytes=gb - 4), dict(grads=ctypes.c_void_p(0x10010)), dict(p=1.5)):
        assert bwd(**kw) == -1, kw


def test_train_trunk_switch(monkeypatch):
    cfg = synth.make_config("tiny")
    monkeypatch.delenv("IRS_TRAIN_TRUNK", raising=False)
    assert _backend.train_trunk_default() == "torch"
    assert InfluentialNet(cfg).trunk == "torch"
    for v in ("torch", "hip"):
        monkeypatch.setenv("IRS_TRAIN_TRUNK", v)
        assert InfluentialNet(cfg).trunk == v and SampleNet(synth.make_config("eval_tiny")).trunk == v
    for v in ("", "HIP", "native", "1"):
        monkeypatch.setenv("IRS_TRAIN_TRUNK", v)
        with pytest.raises(ValueError, match="IRS_TRAIN_TRUNK"):
            InfluentialNet(cfg)
        with pytest.raises(ValueError):
            SampleNet(synth.make_config("eval_tiny"))
    monkeypatch.delenv("IRS_TRAIN_TRUNK")
    net = InfluentialNet(cfg)
    with pytest.raises(ValueError):
        net.trunk = "cuda"
    assert net.trunk == "torch"


def test_cpu_module_with_the_native_trunk_raises():
    cfg = synth.make_config("tiny")
    net = InfluentialNet(cfg).train()
    net.trunk = "hip"
    seq = torch.from_numpy(synth.random_windows(2, cfg.max_len, cfg.n_item))
    with pytest.raises(IrsError, match="GPU"):
        net._decoding_autograd(seq, torch.zeros(2, dtype=torch.int64))
    snet = SampleNet(synth.make_config("eval_tiny")).train()
    snet.trunk = "hip"
    with pytest.raises(IrsError, match="GPU"):
        snet._decoding_autograd(seq)


def test_philox_known_answers():
    # Random123's published known-answer vectors for philox4x32_10
    w = philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    w = philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in w] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_dropout_generator_is_deterministic_with_the_right_keep_rate():
    n = 1 << 20
    for p in (0.05, 0.3):
        a = drop_mult(0x123456789ABCDEF, p, 1, 3, (n,))
        b = drop_mult(0x123456789ABCDEF, p, 1, 3, (n,))
        assert np.array_equal(a, b)
        assert set(np.unique(a)) <= {0.0, 1.0 / (1.0 - float(np.float32(p)))}
        rate = float(np.mean(a > 0))
        assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), (p, rate)
    assert np.array_equal(drop_mult(5, 0.0, 2, 0, (7, 3)), np.ones((7, 3)))


def test_dropout_sites_layers_and_seeds_draw_independently():
    n, p = 1 << 18, 0.3
    base = drop_mult(11, p, 2, 0, (n,)) > 0
    for other in (drop_mult(11, p, 4, 0, (n,)), drop_mult(11, p, 2, 1, (n,)), drop_mult(12, p, 2, 0, (n,)),
                  drop_mult(11 + (1 << 32), p, 2, 0, (n,))):
        o = other > 0
        agree = float(np.mean(o == base))
        expect = p * p + (1 - p) * (1 - p)
        assert abs(agree - expect) <= 5 * math.sqrt(expect * (1 - expect) / n), agree
    # the four words of one counter block serve four consecutive elements
    e = np.arange(8, dtype=np.uint64)
    w = keep_words(3, 1, 0, e)
    blk = philox4x32_10(0, 0, 0, 1, 3, 0)
    assert [int(v) for v in w[:4]] == [int(v) for v in blk]
