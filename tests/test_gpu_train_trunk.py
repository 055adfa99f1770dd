"""-m gpu: the native training trunk (include/irs_hip.h irs_train_*; net.trunk = "hip") against the stock train-mode
nn.TransformerDecoder trunk: loss and every live parameter gradient against a float64 copy of the stock module, with the
stock float32 module's own error setting the bar; dropout masks against the numpy restatement of the generator;
determinism; the reference run's recorded losses; 20-step trajectories; inference after native training."""
import copy

import numpy as np
import pytest
import torch

from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16
from influentialrs_amd.engine import Engine
from influentialrs_amd.model import _backend
from influentialrs_amd.model.evaluator import Evaluator
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from influentialrs_amd.model.uRS import SampleNet

from train_trunk_ref import _mask, functional_trunk, stock_trunk, trunk_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _setup(name, B, Lseq=None, causal=False, seed=1234, **ov):
    cfg = synth.make_config(name, dropout=0.0, **ov)
    net = (SampleNet if causal else InfluentialNet)(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, seed, evaluator=causal).items()})
    net.to(DEV).train()
    L = Lseq or cfg.max_len
    seq = synth.random_windows(B, L, cfg.n_item, seed=B + L)  # pre-padded, target last
    if causal:  # the evaluator's post-padded rows
        seq = np.stack([np.concatenate([r[r > 0], r[r == 0]]) for r in seq])
    seq = torch.from_numpy(seq).to(DEV)
    user = None if causal else torch.from_numpy(np.arange(B) * 7 % cfg.n_user).to(DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(B * 31 + L)
    R = torch.randn((B, L, cfg.emb_dim), generator=g, device=DEV)
    return cfg, net, seq, user, R


def _run(net, fn, R):
    net.zero_grad(set_to_none=True)
    x = fn()
    loss = (x * R.to(x.dtype)).sum()
    loss.backward()
    return loss.item(), {n: p.grad.detach().double().clone() for n, p in net.named_parameters() if p.grad is not None}


def _trunk(net, seq, user):
    out = net._decoding_autograd(seq, user) if user is not None else net._decoding_autograd(seq)
    return out[0] if isinstance(out, tuple) else out


def _native(net, seq, user, R):
    net.trunk = "hip"
    try:
        return _run(net, lambda: _trunk(net, seq, user), R)
    finally:
        net.trunk = "torch"


def _check(nat, s32, s64, d, what=""):
    (ln, gn), (l32, g32), (l64, g64) = nat, s32, s64
    assert abs(ln - l64) <= max(4 * abs(l32 - l64), 2e-6 * abs(l64)), (what, ln, l32, l64)
    dead = [n for n in g64 if n.endswith("multihead_attn.in_proj_weight")]
    live = [n for n in g64 if n not in dead and (n.startswith("decoder.") or "embedder.weight" in n) and "user" not in n]
    assert set(live + dead) <= set(gn)
    big = max(float(g64[n].abs().max()) for n in live)
    for n in dead:
        assert torch.count_nonzero(gn[n]) == 0, (what, n)
        assert float(g64[n].abs().max()) <= 1e-12 * big, (what, n)
    for n in live:
        a, b, c = gn[n], g32[n], g64[n]
        if n.endswith("multihead_attn.in_proj_bias"):
            assert torch.count_nonzero(a[:2 * d]) == 0, (what, n)
            assert float(c[:2 * d].abs().max()) <= 1e-12 * big, (what, n)
            a, b, c = a[2 * d:], b[2 * d:], c[2 * d:]
        scale = float(c.abs().max())
        err, e32 = float((a - c).abs().max()), float((b - c).abs().max())
        assert err <= max(4 * e32, 2e-6 * scale), (what, n, err, e32, scale)
    # no gradient for the user tensors (r_u is detached), as with the stock trunk
    assert not [n for n in gn if n.startswith("user_")]


CASES = [
    ("tiny", 5, None, False, {}),
    ("eval_tiny", 5, 11, True, {}),
    ("default", 4, None, False, {}),
    ("c1", 3, None, False, {}),
    ("c2", 2, None, False, {}),
    ("c4d", 2, None, False, {}),
    ("c2", 2, None, False, {"n_heads": 2}),          # d = 128, head dim 64
    ("tiny", 3, None, False, {"ffn_dim": 120}),
    ("tiny", 3, None, False, {"ffn_dim": 1}),
    ("tiny", 3, None, False, {"n_layers": 1}),
    ("tiny", 3, None, False, {"n_layers": 6}),
    ("tiny", 1, None, False, {}),
    ("tiny", 70, None, False, {}),                    # 840 rows: many row tiles
    ("eval_default", 4, 40, True, {}),               # L_seq < max_len
    ("tiny", 300, None, False, {"n_item": 5}),        # 3600 tokens over 5 items: long same-token chains across chunks
]


@pytest.mark.parametrize("name,B,Lseq,causal,ov", CASES, ids=[f"{c[0]}-B{c[1]}-L{c[2]}-{c[4]}" for c in CASES])
def test_gradients_match_float64_at_p0(name, B, Lseq, causal, ov):
    cfg, net, seq, user, R = _setup(name, B, Lseq, causal, **ov)
    # the yard-stick's trunk is the model's own: same mask as _generate_square_subsequent_mask, same output in float32
    L = seq.shape[1]
    if not causal:
        pi = net.user_mask_layer(net.user_embedder(user))
        own = net._generate_square_subsequent_mask(L, pi).view(B, cfg.n_heads, L, L)[:, 0]
        ref = _mask(net, torch.full_like(seq, 1), user, torch.float32)
    else:
        own = net._generate_square_subsequent_mask(L).to(DEV).expand(B, L, L)
        ref = _mask(net, torch.full_like(seq, 1), None, torch.float32)
    assert torch.equal(own, ref)
    with torch.no_grad():
        x_ref, x_own = stock_trunk(net, seq, user, torch.float32), _trunk(net, seq, user)
        assert float((x_ref - x_own).abs().max()) <= 1e-5 * float(x_own.abs().max())
    nat = _native(net, seq, user, R)
    s32 = _run(net, lambda: _trunk(net, seq, user), R)
    net64 = copy.deepcopy(net).double()
    s64 = _run(net64, lambda: stock_trunk(net64, seq, user, torch.float64), R)
    _check(nat, s32, s64, cfg.emb_dim, name)


@pytest.mark.parametrize("name,B,Lseq,causal", [("tiny", 6, None, False), ("default", 3, None, False),
                                                 ("eval_tiny", 5, 11, True)])
def test_gradients_with_dropout_match_the_documented_masks(name, B, Lseq, causal):
    cfg, net, seq, user, R = _setup(name, B, Lseq, causal)
    L = seq.shape[1]
    dims = (B, L, cfg.emb_dim, cfg.n_heads, cfg.ffn_dim, cfg.max_len, cfg.n_layers)
    net64 = copy.deepcopy(net).double()
    # the restatement is the stock module at p = 0
    ones = trunk_masks(0, 0.0, *dims)
    f64 = _run(net64, lambda: functional_trunk(net64, seq, user, ones), R)
    s64 = _run(net64, lambda: stock_trunk(net64, seq, user, torch.float64), R)
    assert abs(f64[0] - s64[0]) <= 1e-10 * abs(s64[0])
    for n in s64[1]:
        assert float((f64[1][n] - s64[1][n]).abs().max()) <= 1e-10 * max(1.0, float(s64[1][n].abs().max())), n
    for p in (0.05, 0.3):
        net.dropout = net64.dropout = p
        torch.manual_seed(99)
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # what the trunk draws for its step
        masks = trunk_masks(seed, p, *dims)
        torch.manual_seed(99)
        nat = _native(net, seq, user, R)
        f32 = _run(net, lambda: functional_trunk(net, seq, user, masks, torch.float32), R)
        f64 = _run(net64, lambda: functional_trunk(net64, seq, user, masks), R)
        _check(nat, f32, f64, cfg.emb_dim, f"{name} p={p}")


def test_backward_is_bit_deterministic():
    cfg, net, seq, user, R = _setup("default", 8)
    eng = net._hip.get(1, 1, for_training=True)
    x, saved = eng.train_forward(seq, user, 0.05, 12345)
    g1 = eng.train_backward(seq, user, 0.05, 12345, saved, R)
    g2 = eng.train_backward(seq, user, 0.05, 12345, saved, R)
    assert torch.equal(g1, g2)
    x2, _ = eng.train_forward(seq, user, 0.05, 12345)
    assert torch.equal(x, x2)
    x3, _ = eng.train_forward(seq, user, 0.05, 12346)
    assert not torch.equal(x, x3)


def _train_run(seed, steps=3):
    cfg = synth.make_config("default", dropout=0.05)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    net.trunk = "hip"
    irn = IRSNN(cfg, net, DEV)
    torch.manual_seed(seed)
    losses = []
    for s in range(steps):
        seq = torch.from_numpy(synth.random_windows(16, cfg.max_len, cfg.n_item, seed=s)).to(DEV)
        losses.append(irn.train_batch(seq, torch.arange(16, device=DEV)))
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}


def test_native_runs_are_reproducible_from_the_torch_seed():
    l1, p1 = _train_run(5)
    l2, p2 = _train_run(5)
    assert l1 == l2
    assert all(torch.equal(p1[k], p2[k]) for k in p1)
    l3, _ = _train_run(6)
    assert l3[1:] != l1[1:]


def test_training_matches_the_reference_run_with_the_native_trunk(golden):
    """The body of test_gpu_training.py::test_training_matches_the_reference_run with trunk = "hip"."""
    g = golden("train_tiny")
    cfg = synth.make_config("tiny", dropout=0.0)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()})
    net.to(DEV)
    net.trunk = "hip"
    irn = IRSNN(cfg, net, DEV)
    seqs, users = torch.from_numpy(g["irn_seqs"]).to(DEV), torch.from_numpy(g["irn_users"]).to(DEV)
    ev0 = [irn.get_loss_on_eval_data(seqs[i:i + 1], users[i:i + 1]) for i in range(4)]
    tr = [irn.train_batch(seqs[i:i + 1], users[i:i + 1]) for i in range(4)]
    ev1 = [irn.get_loss_on_eval_data(seqs[i:i + 1], users[i:i + 1]) for i in range(4)]
    assert np.allclose(ev0, g["irn_eval_before"], rtol=2e-6, atol=0)
    assert abs(tr[0] - g["irn_train"][0]) <= 2e-6 * abs(tr[0])
    assert np.allclose(tr, g["irn_train"], rtol=2e-4, atol=0), (tr, g["irn_train"])
    assert np.allclose(ev1, g["irn_eval_after"], rtol=5e-4, atol=0), (ev1, g["irn_eval_after"])
    assert np.abs(net.project.bias.detach().cpu().numpy() - g["irn_bias_after"]).max() <= 0.35 * 4 * cfg.lr1
    assert net.user_embedder.weight.grad is None and net.user_mask_layer.weight.grad is None

    ecfg = synth.make_config("eval_tiny", dropout=0.0)
    snet = SampleNet(ecfg)
    snet.load_state_dict({k: torch.from_numpy(v) for k, v in synth.irn_state_dict(ecfg, 17, evaluator=True).items()})
    snet.to(DEV)
    snet.trunk = "hip"
    ev = Evaluator(ecfg, snet, DEV)
    t = torch.from_numpy(g["ev_target"]).to(DEV)
    assert abs(ev.get_loss_on_eval_data(t) - g["ev_eval_before"][0]) <= 2e-6 * g["ev_eval_before"][0]
    etr = [ev.train_batch(t) for _ in range(3)]
    assert np.allclose(etr, g["ev_train"], rtol=2e-4, atol=0), (etr, g["ev_train"])
    assert abs(ev.get_loss_on_eval_data(t) - g["ev_eval_after"][0]) <= 5e-4 * g["ev_eval_after"][0]


def test_twenty_step_trajectory_matches_the_stock_trunk():
    cfg = synth.make_config("default", dropout=0.0)
    sd = {k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()}
    runs = {}
    for trunk in ("torch", "hip"):
        net = InfluentialNet(cfg)
        net.load_state_dict(sd)
        net.to(DEV)
        net.trunk = trunk
        irn = IRSNN(cfg, net, DEV)
        losses = []
        for s in range(20):
            seq = torch.from_numpy(synth.random_windows(32, cfg.max_len, cfg.n_item, seed=100 + s)).to(DEV)
            losses.append(irn.train_batch(seq, torch.arange(32, device=DEV) * 5))
        runs[trunk] = (losses, {k: v.detach().clone() for k, v in net.state_dict().items()})
    (lt, pt), (lh, ph) = runs["torch"], runs["hip"]
    assert np.allclose(lh, lt, rtol=2e-4, atol=0), (lh, lt)
    for k in pt:
        if k.endswith("multihead_attn.in_proj_weight"):
            continue  # dead: no output depends on it
        a, b = ph[k], pt[k]
        if k.endswith("multihead_attn.in_proj_bias"):
            a, b = a[2 * cfg.emb_dim:], b[2 * cfg.emb_dim:]
        assert float((a - b).abs().max()) <= 0.35 * 20 * cfg.lr1, k


def test_inference_after_native_training_matches_a_fresh_engine():
    cfg, net, seq, user, _ = _setup("tiny", 6)
    net.dropout = 0.05
    net.trunk = "hip"
    irn = IRSNN(cfg, net, DEV)
    for _ in range(3):
        irn.train_batch(seq, user)
    net.eval()
    x = net.decoding(seq, user)
    pos = torch.full((seq.shape[0],), cfg.max_len - 2, dtype=torch.int32, device=DEV)
    xr = net.decode_rows(seq, user, pos)
    _, ids, _ = net._hip.engine.score_topk(xr, 10, IRS_SWEEP_BF16)
    fresh = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                   ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN,
                   device=torch.device(DEV), max_rows=64, max_seqs=8)
    fresh.bind_state_dict({k: v.detach() for k, v in net.state_dict().items()})
    fx, _, _ = fresh.decode(seq, user, want_x=True)
    _, fxr, _ = fresh.decode(seq, user, want_x=False, pos=pos)
    _, fids, _ = fresh.score_topk(fxr, 10, IRS_SWEEP_BF16)
    assert float((x - fx).abs().max()) <= 1e-5
    assert torch.equal(ids, fids)
