"""-m gpu: the fused backward of projection + cross entropy (include/irs_hip.h irs_ce_backward; net.ce_backward = "fused")
-- dx, dW, db out of two register-resident passes, no dL/dlogits buffer -- against the reference's own formulation,
nn.Linear + nn.CrossEntropyLoss under stock autograd, in float64 (the yard-stick) and float32 (whose error sets the
tolerance, as in tests/test_gpu_training.py)."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_MASK_IRN, IRS_SWEEP_BF16, IRS_SWEEP_F32
from influentialrs_amd.engine import Engine, IrsError
from influentialrs_amd.model import _backend
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIB = 1 << 20


def _reference_loss(x, W, b, labels0):
    mask = labels0.ge(0)
    return F.cross_entropy(F.linear(x, W, b)[mask], labels0[mask])


def _problem(M, d, N):
    """The construction of test_gpu_training.py::test_project_ce_loss_and_gradients_match_autograd."""
    g = torch.Generator(device=DEV)
    g.manual_seed(M + N)
    nh = d // 32 if d % 32 == 0 else 1
    cfg = synth.make_config("tiny", n_item=N, emb_dim=d, n_heads=nh, n_layers=1, max_len=4, ffn_dim=8, n_user=2)
    net = InfluentialNet(cfg).to(DEV)
    with torch.no_grad():
        net.project.weight.copy_((torch.rand((N, d), generator=g, device=DEV) * 2 - 1) * d ** -0.5)
        net.project.bias.copy_(torch.randn((N,), generator=g, device=DEV) * 0.1)
    x = torch.randn((M, d), generator=g, device=DEV, requires_grad=True)
    labels0 = torch.randint(0, N, (M,), generator=g, device=DEV)
    labels0[torch.rand((M,), generator=g, device=DEV) < 0.3] = -1  # pad targets
    labels0[0], labels0[1] = N - 1, 0
    return net, x, labels0


def _references(x, W, b, labels0):
    """((dx, dW, db) in float64, the same from the float32 formulation)."""
    out = []
    for dt in (torch.float64, torch.float32):
        xs = x.detach().to(dt).requires_grad_(True)
        Ws = W.detach().to(dt).requires_grad_(True)
        bs = b.detach().to(dt).requires_grad_(True)
        _reference_loss(xs, Ws, bs, labels0).backward()
        out.append((xs.grad, Ws.grad, bs.grad))
    return out


def _assert_close(got, r64, r32, what=""):
    for name, mine, a64, a32 in zip(("dx", "dW", "db"), got, r64, r32):
        scale = a64.abs().max().item()
        err = (mine.double() - a64).abs().max().item()
        err32 = (a32.double() - a64).abs().max().item()
        print(f"{what}{name}: err {err:.3e} err32 {err32:.3e} scale {scale:.3e}")
        assert err <= max(4 * err32, 2e-6 * scale), (what, name, err, err32, scale)


SHAPES = [(300, 64, 3415), (70, 128, 100_003), (9000, 128, 3415), (45, 40, 5000), (33, 256, 70_001), (12_736, 128, 3415)]


@pytest.mark.parametrize("M,d,N", SHAPES)
def test_fused_gradients_match_float64(M, d, N):
    net, x, labels0 = _problem(M, d, N)
    net.ce_backward = "fused"
    assert net._hip.ce_backward == "fused"
    loss = _backend.project_ce(x, net.project, labels0, net._hip)
    loss.backward()
    r64, r32 = _references(x, net.project.weight, net.project.bias, labels0)
    _assert_close((x.grad, net.project.weight.grad, net.project.bias.grad), r64, r32)
    assert (x.grad[labels0 < 0] == 0).all()  # ignored rows carry no gradient, exactly


def _engine(net, M):
    eng = net._hip.get(1, M, for_training=True)
    assert eng.max_rows >= M
    return eng


def _abi_call(eng, x, labels0, lse, scale, accumulate, dW=None, db=None):
    M, d = x.shape
    dx = torch.full((M, d), float("nan"), device=DEV)
    dW = torch.full((eng.n_local, d), float("nan"), device=DEV) if dW is None else dW
    db = torch.full((eng.n_local,), float("nan"), device=DEV) if db is None else db
    scratch = torch.empty(eng.ce_backward_scratch_bytes(M), dtype=torch.uint8, device=DEV)
    eng.ce_backward(x, labels0, lse, scale, accumulate, dx, dW, db, scratch)
    return dx, dW, db


@pytest.mark.parametrize("M,d,N", [(300, 64, 3415), (45, 40, 5000), (70, 128, 100_003)])
def test_abi_overwrites_and_accumulates(M, d, N):
    """accumulate = 0 overwrites NaN-filled outputs completely (padded tiles, n_local not a multiple of 32); accumulate = 1
    onto a known pre-fill equals pre-fill + that result."""
    net, x, labels0 = _problem(M, d, N)
    eng = _engine(net, M)
    xd = x.detach()
    lse, _, tot = eng.ce_forward(xd, labels0)
    n_valid = tot[1].item()
    scale = 1.0 / n_valid
    dx, dW, db = _abi_call(eng, xd, labels0, lse, scale, False)
    for t in (dx, dW, db):
        assert torch.isfinite(t).all()
    r64, r32 = _references(x, net.project.weight, net.project.bias, labels0)
    _assert_close((dx, dW, db), r64, r32, "overwrite ")
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    pw = torch.randn((N, d), generator=g, device=DEV) * r64[1].abs().max().item()
    pb = torch.randn((N,), generator=g, device=DEV) * r64[2].abs().max().item()
    dx2, dW2, db2 = _abi_call(eng, xd, labels0, lse, scale, True, pw.clone(), pb.clone())
    _assert_close((dx2, dW2, db2), (r64[0], r64[1] + pw.double(), r64[2] + pb.double()),
                  (r32[0], r32[1].double() + pw.double(), r32[2].double() + pb.double()), "accumulate ")
    assert torch.equal(dx2, dx)  # dx is overwritten either way


@pytest.mark.parametrize("M,d,N", [(9000, 128, 3415), (70, 128, 100_003)])
def test_two_identical_calls_give_identical_bits(M, d, N):
    """One irs_ce_backward call each: the row-split partials of the item-owned pass at the small catalog, the
    catalog-split partials of the row-owned pass at the few rows."""
    net, x, labels0 = _problem(M, d, N)
    xd = x.detach()
    eng = _engine(net, M)
    lse, _, _ = eng.ce_forward(xd, labels0)
    a = _abi_call(eng, xd, labels0, lse, 1.0 / M, False)
    b = _abi_call(eng, xd, labels0, lse, 1.0 / M, False)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_no_row_by_item_buffer():
    """At (4096, 128, 100003) the chunked route's dL/dlogits chunk is ~1.06 GB; the fused backward allocates its three
    gradients and the scratch, nothing else (8 MiB: a cap for allocator rounding, not a measurement)."""
    M, d, N = 4096, 128, 100_003
    net, x, labels0 = _problem(M, d, N)
    net.ce_backward = "fused"
    loss = _backend.project_ce(x, net.project, labels0, net._hip)
    eng = net._hip.engine
    scratch = eng.ce_backward_scratch_bytes(min(M, _backend._ProjectCE.ROWS))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    allowed = 4 * (M * d + N * d + N) + scratch + 8 * MIB
    print(f"rise {rise / MIB:.1f} MiB, allowed {allowed / MIB:.1f} MiB, scratch {scratch / MIB:.1f} MiB")
    assert rise <= allowed, (rise, allowed)
    assert allowed < (4 * M * N) // 4  # a quarter of the [M, n_item] float32 chunk this route does not allocate


@pytest.mark.parametrize("M,d,N", [(8192, 128, 3415), (8192, 128, 1_000_000), (32, 256, 10_000_000)])
def test_scratch_is_never_of_order_rows_by_items(M, d, N):
    """Pure size queries: a context of that shape without a catalog behind it."""
    from influentialrs_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    dims = _lib.IrsDims(n_item=N, n_user=2, d=d, max_len=4, n_heads=d // 32, ffn_dim=8, n_layers=1, u_dim=2, mask_mode=0,
                        max_rows=M, max_k=100, max_seqs=1)
    assert lib.irs_create(ctypes.byref(h), ctypes.byref(dims), None) == 0
    try:
        n = lib.irs_ce_backward_scratch_bytes(h, M)
        assert 0 < n <= 64 * MIB + 4 * (M * d + N * d), n
    finally:
        lib.irs_destroy(h)


def _train_pair(cfgname, n):
    cfg = synth.make_config(cfgname, dropout=0.0)
    sd = {k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()}
    net = InfluentialNet(cfg)
    net.load_state_dict(sd)
    net.to(DEV)
    hists = synth.user_histories(max(n, 8), cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:n]
    raws, seqs, users, targets, labels = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    return cfg, net, torch.from_numpy(seqs).to(DEV), torch.from_numpy(users).to(DEV)


def _stock_loss(net, seqs, users):
    out = net.project(net._decoding_autograd(seqs.clone(), users)[0])[:, :-1, :].contiguous().view(-1, net.n_item)
    tgt = seqs[:, 1:].contiguous().view(-1)
    mask = tgt.gt(0)
    return nn.CrossEntropyLoss()(out[mask], tgt[mask] - 1)


@pytest.mark.parametrize("trunk", ["torch", "hip"])
@pytest.mark.parametrize("cfgname,n", [("tiny", 6), ("default", 8)])
def test_training_step_with_the_fused_backward(cfgname, n, trunk):
    """IRSNN._masked_loss + backward against the stock formulation on a deep-copied twin, parameter by parameter; then
    three Adam steps bring the loss down.  With trunk = "hip" the step touches no torch GEMM."""
    cfg, net, seqs, users = _train_pair(cfgname, n)
    twin = copy.deepcopy(net)
    net.ce_backward = "fused"
    net.trunk = trunk
    irn = IRSNN(cfg, net, DEV)
    net.train()
    twin.train()
    l_hip = irn._masked_loss(seqs, users)
    l_hip.backward()
    l_ref = _stock_loss(twin, seqs, users)
    l_ref.backward()
    for (name, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
        if q.grad is None:
            assert p.grad is None or not p.grad.abs().max() > 0, name
            continue
        sc = q.grad.abs().max().item()
        assert (p.grad - q.grad).abs().max().item() <= 2e-4 * sc + 1e-9, name
    net.zero_grad()
    l0 = irn.train_batch(seqs, users)
    l1 = irn.train_batch(seqs, users)
    l2 = irn.train_batch(seqs, users)
    assert l2 < l1 < l0


def _tiny_engine(world=1, max_rows=8):
    cfg = synth.make_config("tiny")
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in synth.irn_state_dict(cfg, 1234).items()}
    eng = Engine(n_item=cfg.n_item, n_user=cfg.n_user, d=cfg.emb_dim, max_len=cfg.max_len, n_heads=cfg.n_heads,
                 ffn_dim=cfg.ffn_dim, n_layers=cfg.n_layers, u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV),
                 max_rows=max_rows, max_seqs=8, rank=0, world=world)
    eng.bind_state_dict(sd)
    return cfg, sd, eng


def test_contract_shards_bounds_and_staleness():
    cfg, sd, shard = _tiny_engine(world=2)
    x = torch.randn(8, cfg.emb_dim, device=DEV)
    lab = torch.arange(8, dtype=torch.int64, device=DEV)
    lse = torch.zeros(8, device=DEV)
    dx = torch.empty(8, cfg.emb_dim, device=DEV)
    sdw, sdb = torch.empty(shard.n_local, cfg.emb_dim, device=DEV), torch.empty(shard.n_local, device=DEV)
    with pytest.raises(IrsError, match="whole catalog"):
        shard.ce_backward(x, lab, lse, 1.0, False, dx, sdw, sdb, torch.empty(1 << 16, dtype=torch.uint8, device=DEV))

    cfg, sd, eng = _tiny_engine()
    lse, _, _ = eng.ce_forward(x, lab)
    eng.finalize()
    v0, i0, _ = eng.score_topk(x, 10, IRS_SWEEP_BF16)
    dw, db = torch.empty(cfg.n_item, cfg.emb_dim, device=DEV), torch.empty(cfg.n_item, device=DEV)
    need = eng.ce_backward_scratch_bytes(8)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(IrsError):  # M > max_rows
        eng.ce_backward_scratch_bytes(9)
    x9 = torch.randn(9, cfg.emb_dim, device=DEV)
    with pytest.raises(IrsError, match="max_rows"):
        eng.ce_backward(x9, torch.zeros(9, dtype=torch.int64, device=DEV), torch.zeros(9, device=DEV), 1.0, False,
                        torch.empty(9, cfg.emb_dim, device=DEV), dw, db, scratch)
    with pytest.raises(IrsError, match="scratch"):  # one byte short
        eng.ce_backward(x, lab, lse, 1.0, False, dx, dw, db, scratch[:need - 1])
    lib, p = eng.lib, lambda t: ctypes.c_void_p(t.data_ptr())
    for null in range(3):  # a null output
        outs = [p(dx), p(dw), p(db)]
        outs[null] = None
        assert lib.irs_ce_backward(eng.h, p(x), p(lab), p(lse), 8, 1.0, 0, *outs, p(scratch), need, None) == -1
    eng.score_topk(x, 10, IRS_SWEEP_BF16)  # none of the refused calls touched the state
    eng.ce_backward(x, lab, lse, 1.0, False, dx, dw, db, scratch)
    with pytest.raises(IrsError, match="irs_finalize_weights"):
        eng.score_topk(x, 10, IRS_SWEEP_BF16)
    eng.score_topk(x, 10, IRS_SWEEP_F32)
    eng.finalize()
    v1, i1, _ = eng.score_topk(x, 10, IRS_SWEEP_BF16)
    torch.cuda.synchronize()
    assert torch.equal(i0, i1) and torch.equal(v0, v1)


def test_label_equal_to_n_item_matches_no_column():
    """Such a row's G is scale * softmax with no -1 anywhere: it adds +scale to db.sum() where a valid row adds 0.
    Bound 1e-5 of the largest magnitude: an entry of G carries the fast exp's few ulp plus |lse| 2^-24 from the float32
    log-sum-exp (together < 1e-6 relative), and 8 rows / 257 items of like magnitude are summed in float32."""
    cfg, sd, eng = _tiny_engine()
    N, d = cfg.n_item, cfg.emb_dim
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.randn(8, d, generator=g, device=DEV)
    lab = torch.randint(0, N, (8,), generator=g, device=DEV)
    lab[2] = N
    lab[5] = -1
    lse, _, _ = eng.ce_forward(x, lab)
    scale = 0.25
    dx = torch.empty(8, d, device=DEV)
    dw, db = torch.empty(N, d, device=DEV), torch.empty(N, device=DEV)
    eng.ce_backward(x, lab, lse, scale, False, dx, dw, db, torch.empty(eng.ce_backward_scratch_bytes(8), dtype=torch.uint8, device=DEV))
    W, b = sd["project.weight"].double(), sd["project.bias"].double()
    G = torch.softmax(x.double() @ W.t() + b, dim=1)
    for m in range(8):
        if 0 <= lab[m].item() < N:
            G[m, lab[m]] -= 1.0
    G[5] = 0
    G *= scale
    assert abs(db.double().sum().item() - scale) <= 1e-5 * scale
    for mine, ref in ((dx, G @ W), (dw, G.t() @ x.double()), (db, G.sum(0))):
        assert (mine.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (dx[5] == 0).all()
