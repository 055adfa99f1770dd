"""-m gpu: projection + cross entropy over an item-sharded catalog (include/irs_hip.h irs_ce_forward_sharded /
irs_ce_backward_sharded; the front ends' project_ce_sharded) against the reference's own formulation on ONE device holding
everything -- nn.Linear + nn.CrossEntropyLoss under stock autograd, in float64 (the yard-stick) and float32 (whose error
sets the tolerance, the rule of tests/test_gpu_ce_backward.py::_assert_close).

`world` ranks are spawned processes on the one GPU of the test box, gloo through the library's callback communicator
(the worker pattern of tests/test_gpu_multirank.py; at most 3 processes).  The full W, b, rows and labels are the same
on every rank; each rank binds its shard of the catalog and owns its slice of the rows."""
import copy
import math
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = [(16, 64, 101), (45, 40, 5000), (33, 128, 3415)]  # (rows per rank, d, n_item)


# ---------------------------------------------------------------- the problem and its references (same on every rank)
def _reference_loss(x, W, b, labels0):
    mask = labels0.ge(0)
    return F.cross_entropy(F.linear(x, W, b)[mask], labels0[mask])


def _problem(world, B, d, N, all_ignored_rank=None):
    """The construction of tests/test_gpu_ce_backward.py::_problem at M = world * B rows, then: labels forced onto every
    shard's first and last item, and one rank's rows all ignored."""
    from influentialrs_amd.engine import shard_bounds
    M = world * B
    g = torch.Generator(device=DEV)
    g.manual_seed(M + N)
    W = (torch.rand((N, d), generator=g, device=DEV) * 2 - 1) * d ** -0.5
    b = torch.randn((N,), generator=g, device=DEV) * 0.1
    x = torch.randn((M, d), generator=g, device=DEV)
    labels0 = torch.randint(0, N, (M,), generator=g, device=DEV)
    labels0[torch.rand((M,), generator=g, device=DEV) < 0.3] = -1  # pad targets
    own = world - 1 if all_ignored_rank is None else all_ignored_rank
    slots = [i for i in range(M) if not own * B <= i < (own + 1) * B]
    edges = [e for r in range(world) for e in (shard_bounds(N, world, r)[0], shard_bounds(N, world, r)[1] - 1)]
    assert len(slots) >= len(edges)
    for i, e in zip(slots, edges):
        labels0[i] = e
    labels0[own * B:(own + 1) * B] = -1
    return W, b, x, labels0


def _references(x, W, b, labels0):
    """[(loss, dx, dW, db) in float64, the same from the float32 formulation]."""
    out = []
    for dt in (torch.float64, torch.float32):
        xs = x.detach().to(dt).requires_grad_(True)
        Ws = W.detach().to(dt).requires_grad_(True)
        bs = b.detach().to(dt).requires_grad_(True)
        loss = _reference_loss(xs, Ws, bs, labels0)
        loss.backward()
        out.append((loss.item(), xs.grad, Ws.grad, bs.grad))
    return out


def _assert_loss(loss, l64, l32, what=""):
    bound = max(4 * abs(l32 - l64), 2e-6 * abs(l64))
    print(f"{what}loss {loss!r} loss64 {l64!r} loss32 {l32!r}: err {abs(loss - l64):.3e} bound {bound:.3e}")
    assert abs(loss - l64) <= bound, (what, loss, l64, l32)


def _assert_close(got, r64, r32, what=""):
    for name, mine, a64, a32 in zip(("dx", "dW", "db"), got, r64, r32):
        scale = a64.abs().max().item()
        err = (mine.double() - a64).abs().max().item()
        err32 = (a32.double() - a64).abs().max().item()
        print(f"{what}{name}: err {err:.3e} err32 {err32:.3e} scale {scale:.3e}")
        assert err <= max(4 * err32, 2e-6 * scale), (what, name, err, err32, scale)


def _engine(N, d, W, b, rank, world, max_rows):
    from influentialrs_amd import synth
    from influentialrs_amd._lib import IRS_MASK_IRN
    from influentialrs_amd.engine import Engine
    nh = d // 32 if d % 32 == 0 else 1
    cfg = synth.make_config("tiny", n_item=N, emb_dim=d, n_heads=nh, n_layers=1, max_len=4, ffn_dim=8, n_user=2)
    eng = Engine(n_item=N, n_user=cfg.n_user, d=d, max_len=cfg.max_len, n_heads=nh, ffn_dim=cfg.ffn_dim, n_layers=1,
                 u_dim=cfg.u_emb_dim, mask_mode=IRS_MASK_IRN, device=torch.device(DEV), max_rows=max_rows, max_seqs=1, rank=rank,
                 world=world)
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in synth.irn_state_dict(cfg, seed=1).items()}
    sd["project.weight"], sd["project.bias"] = W, b
    eng.bind_state_dict(sd)
    return eng


def _sharded_call(eng, comm, x, labels0, scale=None, blocks=None):
    """Forward + backward of this rank's rows through the two entry points: (tot, lse, dx, dW, db).  scale None = 1 / the
    world's n_valid.  blocks: row ranges walked with `accumulate`."""
    B, d = x.shape
    lse, ls, tot = eng.ce_forward_sharded(comm, x, labels0)
    if scale is None:
        scale = 1.0 / tot[1].item()
    dx = torch.full((B, d), float("nan"), device=DEV)
    dW = torch.full((eng.n_local, d), float("nan"), device=DEV)
    db = torch.full((eng.n_local,), float("nan"), device=DEV)
    for i, (c0, c1) in enumerate(blocks or [(0, B)]):
        scratch = torch.empty(eng.ce_backward_sharded_scratch_bytes(c1 - c0), dtype=torch.uint8, device=DEV)
        eng.ce_backward_sharded(comm, x[c0:c1], labels0[c0:c1], lse[c0:c1], scale, i > 0, dx[c0:c1], dW, db, scratch)
    torch.cuda.synchronize()
    return tot, lse, ls, dx, dW, db


def _same_on_all_ranks(t, world, what):
    import torch.distributed as dist
    box = [None] * world
    dist.all_gather_object(box, t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    assert all(v == box[0] for v in box), f"{what} differs between ranks"


# ---------------------------------------------------------------- the cases (run inside a rank process)
def _case_float64(rank, world):
    """Case 1: loss, dx (own rows), dW / db (own shard) against float64 on the full problem; uneven shards at world 3."""
    from influentialrs_amd.engine import Comm
    comm = Comm(torch.device(DEV))
    assert comm.world == world and not comm.is_rccl
    for B, d, N in SHAPES:
        W, b, x, labels0 = _problem(world, B, d, N)
        (l64, *r64), (l32, *r32) = _references(x, W, b, labels0)
        eng = _engine(N, d, W, b, rank, world, world * B)
        assert eng.n_local < N or world == 1
        sl = slice(rank * B, (rank + 1) * B)
        tot, lse, ls, dx, dW, db = _sharded_call(eng, comm, x[sl].contiguous(), labels0[sl].contiguous())
        what = f"[world {world} rank {rank} {(B, d, N)}] "
        assert tot[1].item() == labels0.ge(0).sum().item() and tot[2].item() == 0
        _assert_loss((tot[0] / tot[1]).item(), l64, l32, what)
        _same_on_all_ranks(tot, world, "the loss triple")
        lo, hi = eng.item_lo, eng.item_hi
        _assert_close((dx, dW, db), (r64[0][sl], r64[1][lo:hi], r64[2][lo:hi]), (r32[0][sl], r32[1][lo:hi], r32[2][lo:hi]), what)
        assert (dx[labels0[sl] < 0] == 0).all()  # ignored rows carry no gradient, exactly
        if rank == world - 1:
            assert (dx == 0).all()  # this rank's rows are all ignored; its shard still gets the world's dW / db
        # the global lse of the own rows, and the label score (exact fma chain on whichever shard holds the label): float32
        # values below 16 in magnitude, whose ulp is at most 9.5e-7 -- four of them
        logits = F.linear(x[sl].double(), W.double(), b.double())
        assert (lse.double() - torch.logsumexp(logits, 1)).abs().max().item() <= 4e-6
        valid = labels0[sl] >= 0
        want = logits[valid].gather(1, labels0[sl][valid].view(-1, 1))[:, 0]
        assert (ls[valid].double() - want).abs().max().item() <= 4e-6 if valid.any() else True
        assert torch.isinf(ls[~valid]).all()


def _case_world1(rank, world):
    """Case 2: with one rank the two entry points equal irs_ce_forward / irs_ce_backward bit for bit."""
    from influentialrs_amd.engine import Comm
    assert world == 1
    comm = Comm(torch.device(DEV))
    for B, d, N in SHAPES + [(300, 64, 3415)]:
        W, b, x, labels0 = _problem(1, B, d, N, all_ignored_rank=5)  # (no rank is ignored as a whole)
        eng = _engine(N, d, W, b, 0, 1, B)
        tot, lse, ls, dx, dW, db = _sharded_call(eng, comm, x, labels0, scale=1.0 / B)
        lse1, ls1, tot1 = eng.ce_forward(x, labels0)
        dx1, dW1, db1 = torch.empty_like(dx), torch.empty_like(dW), torch.empty_like(db)
        scratch = torch.empty(eng.ce_backward_scratch_bytes(B), dtype=torch.uint8, device=DEV)
        eng.ce_backward(x, labels0, lse1, 1.0 / B, False, dx1, dW1, db1, scratch)
        torch.cuda.synchronize()
        for name, u, v in (("lse", lse, lse1), ("label score", ls, ls1), ("dx", dx, dx1), ("dW", dW, dW1), ("db", db, db1)):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (name, B, d, N)
        assert torch.equal(tot.view(torch.int64), tot1.view(torch.int64)), (tot, tot1)


def _case_edges(rank, world):
    """Cases 3 and 4 at world 2: determinism, accumulate over two row blocks, a label >= n_item, all rows ignored."""
    from influentialrs_amd import synth
    from influentialrs_amd.engine import Comm
    from influentialrs_amd.model import _backend
    from influentialrs_amd.model.influentialRS import InfluentialNet
    comm = Comm(torch.device(DEV))
    B, d, N = 45, 40, 5000
    W, b, x, labels0 = _problem(world, B, d, N)
    (l64, *r64), (l32, *r32) = _references(x, W, b, labels0)
    eng = _engine(N, d, W, b, rank, world, world * B)
    sl = slice(rank * B, (rank + 1) * B)
    xl, ll = x[sl].contiguous(), labels0[sl].contiguous()
    lo, hi = eng.item_lo, eng.item_hi
    ref64 = (r64[0][sl], r64[1][lo:hi], r64[2][lo:hi])
    ref32 = (r32[0][sl], r32[1][lo:hi], r32[2][lo:hi])
    # two identical calls give identical bits
    a = _sharded_call(eng, comm, xl, ll)
    c = _sharded_call(eng, comm, xl, ll)
    for u, v in zip(a, c):
        assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
    # accumulate across two row blocks equals one call (same tolerance against float64)
    two = _sharded_call(eng, comm, xl, ll, blocks=[(0, 32), (32, B)])
    _assert_close(two[3:], ref64, ref32, f"[two blocks, rank {rank}] ")
    assert torch.equal(two[1], a[1])  # the forward was one call either way
    # a label >= n_item: counted in loss[2] on every rank, in neither sum (the same bits as if the row were ignored)
    bad, ign = labels0.clone(), labels0.clone()
    bad[3], ign[3] = N + 5, -1
    tb = eng.ce_forward_sharded(comm, xl, bad[sl].contiguous())[2]
    ti = eng.ce_forward_sharded(comm, xl, ign[sl].contiguous())[2]
    torch.cuda.synchronize()
    assert tb[2].item() == 1 and ti[2].item() == 0
    assert torch.equal(tb[:2].view(torch.int64), ti[:2].view(torch.int64)) and tb[1].item() == a[0][1].item() - 1
    # ---- through the front end: IndexError on every rank; all rows ignored on all ranks -> nan loss, zero gradients
    cfg = synth.make_config("tiny", n_item=N, emb_dim=d, n_heads=1, n_layers=1, max_len=4, ffn_dim=8, n_user=2)
    net = InfluentialNet(cfg).to(DEV)
    with torch.no_grad():
        net.project.weight.copy_(W)
        net.project.bias.copy_(b)
    net.shard_items(rank, world)
    assert net._hip.holds_shard() and net.project.weight.shape[0] == hi - lo
    with pytest.raises(IndexError):
        _backend.project_ce_sharded(xl, net.project, bad[sl].contiguous(), net._hip)
    for setting in ("chunked", "fused"):
        net.ce_backward = setting
        net.zero_grad()
        xr = xl.clone().requires_grad_(True)
        loss = _backend.project_ce_sharded(xr, net.project, ll, net._hip)
        loss.backward()
        _assert_loss(loss.item(), l64, l32, f"[front end {setting}, rank {rank}] ")
        _assert_close((xr.grad, net.project.weight.grad, net.project.bias.grad), ref64, ref32, f"[front end {setting}, rank {rank}] ")
    net.zero_grad()
    xr = xl.clone().requires_grad_(True)
    loss = _backend.project_ce_sharded(xr, net.project, torch.full_like(ll, -1), net._hip)
    assert math.isnan(loss.item())
    loss.backward()
    assert (xr.grad == 0).all() and (net.project.weight.grad == 0).all() and (net.project.bias.grad == 0).all()


def _stock_irn_loss(net, seqs, users, dtype):
    """The reference's train_batch body (influentialRS.py:157-200, 292-303) on `net` in `dtype`, all torch."""
    B, L = seqs.shape
    pad = seqs.eq(0)
    enc = torch.zeros(net.max_len, B, net.embed_dim, device=seqs.device, dtype=dtype)
    x = (net.item_embedder(seqs) * math.sqrt(net.embed_dim) + net.pos_embedder(seqs)).transpose(0, 1)
    pi = net.user_mask_layer(net.user_embedder(users)).detach()
    tril = torch.ones(L, L, device=seqs.device).tril().bool()
    m = torch.full((B, L, L), float("-inf"), device=seqs.device, dtype=dtype)
    m = torch.where(tril.unsqueeze(0), pi.view(B, 1, 1).expand(B, L, L).to(dtype), m)
    m[:, :, -1] = 1.0
    padf = torch.zeros_like(pad, dtype=dtype).masked_fill(pad, float("-inf"))
    out = net.decoder(tgt=x, memory=enc, tgt_mask=torch.repeat_interleave(m, net.n_heads, dim=0), tgt_key_padding_mask=padf)
    logits = net.project(out.transpose(0, 1))[:, :-1, :].reshape(-1, net.n_item)
    tgt = seqs[:, 1:].reshape(-1)
    return F.cross_entropy(logits[tgt.gt(0)], tgt[tgt.gt(0)] - 1)


def _stock_eval_loss(net, target, dtype):
    """Evaluator.train_batch's body (evaluator.py:53-68; SampleNet.decoding, uRS.py:52-64) in `dtype`, all torch."""
    seq = target[:, :-1]
    B, L = seq.shape
    pad = seq.eq(0)
    enc = torch.zeros(net.max_len, B, net.embed_dim, device=seq.device, dtype=dtype)
    x = (net.word_embedder(seq) * math.sqrt(net.embed_dim) + net.pos_embedder(seq)).transpose(0, 1)
    mask = net._generate_square_subsequent_mask(L).to(seq.device).to(dtype)
    padf = torch.zeros_like(pad, dtype=dtype).masked_fill(pad, float("-inf"))
    out = net.decoder(tgt=x, memory=enc, tgt_mask=mask, tgt_key_padding_mask=padf).transpose(0, 1)
    logits = net.project(out).reshape(-1, net.n_item)
    tgt = target[:, 1:].reshape(-1)
    return F.cross_entropy(logits[tgt.gt(0)], tgt[tgt.gt(0)] - 1)


def _stock_run(net, lr, loss_fn, steps, dtype):
    """`steps` Adam steps of the handlers' optimizer on a copy of `net` in `dtype`: (losses, the copy)."""
    twin = copy.deepcopy(net).to(dtype).train()
    opt = torch.optim.Adam(twin.parameters(), betas=(0.9, 0.98), eps=1e-09, lr=lr)
    losses = []
    for _ in range(steps):
        loss = loss_fn(twin, dtype)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses, twin


def _check_training(handler_s, handler_1, net_s, net_1, step_s, step_1, stock, steps, rank, world, what):
    import torch.distributed as dist
    l64, n64 = _stock_run(net_1, handler_1.optimizer.param_groups[0]["lr"], stock, steps, torch.float64)
    l32, n32 = _stock_run(net_1, handler_1.optimizer.param_groups[0]["lr"], stock, steps, torch.float32)
    got_s = [step_s() for _ in range(steps)]
    got_1 = [step_1() for _ in range(steps)]
    for i in range(steps):
        bound = max(4 * abs(l32[i] - l64[i]), 2e-6 * abs(l64[i]))
        print(f"{what} step {i}: sharded {got_s[i]!r} unsharded {got_1[i]!r} f32 {l32[i]!r} f64 {l64[i]!r} bound {bound:.3e}")
        assert abs(got_s[i] - got_1[i]) <= bound, (what, i, got_s[i], got_1[i], bound)
    assert steps == 1 or got_s[-1] < got_s[0]  # Adam steps bring the loss down
    # the replicas stay equal: every parameter but project.* is bit-identical on all ranks
    flat = torch.cat([p.detach().reshape(-1) for n, p in net_s.named_parameters() if not n.startswith("project.")])
    _same_on_all_ranks(flat, world, f"{what}: the replicated parameters")
    # each rank's project.* against the matching rows of the unsharded model's; yard-stick: stock float32 vs float64
    eng = net_s._hip.engine
    lo, hi = eng.item_lo, eng.item_hi
    for name in ("weight", "bias"):
        w64 = getattr(n64.project, name).detach()
        err32 = (getattr(n32.project, name).detach().double() - w64).abs().max().item()
        scale = w64.abs().max().item()
        mine, full = getattr(net_s.project, name).detach(), getattr(net_1.project, name).detach()
        assert mine.shape[0] == hi - lo
        err = (mine.double() - full[lo:hi].double()).abs().max().item()
        print(f"{what} project.{name}: err {err:.3e} err32 {err32:.3e} scale {scale:.3e}")
        assert err <= max(4 * err32, 2e-6 * scale), (what, name, err, err32, scale)
    dist.barrier()


def _case_front_end(rank, world):
    """Case 5: IRSNN and Evaluator on a module that holds only its shard, each rank feeding its half of the batch,
    against the same handlers on one device holding the whole catalog and the whole batch."""
    from influentialrs_amd import synth
    from influentialrs_amd.model.evaluator import Evaluator
    from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
    from influentialrs_amd.model.uRS import SampleNet
    cfg = synth.make_config("tiny", dropout=0.0)
    sd = {k: torch.from_numpy(v) for k, v in synth.irn_state_dict(cfg, 1234).items()}
    n = 6
    rows = synth.eval_rows(synth.user_histories(8, cfg.n_item, seed=7), cfg.n_item, seed=11)[:n]
    _, seqs, users, _, _ = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    seqs, users = torch.from_numpy(seqs).to(DEV), torch.from_numpy(users).to(DEV)
    nets = []
    for _ in range(2):
        net = InfluentialNet(cfg)
        net.load_state_dict(sd)
        nets.append(net.to(DEV))
    net_s, net_1 = nets
    net_s.shard_items(rank, world)
    irn_s, irn_1 = IRSNN(cfg, net_s, DEV), IRSNN(cfg, net_1, DEV)
    per = n // world
    sl = slice(rank * per, (rank + 1) * per)
    my_seqs, my_users = seqs[sl].contiguous(), users[sl].contiguous()
    # eval loss: the same global number on every rank, equal to the unsharded handler's on the full batch
    with torch.no_grad():
        l64 = _stock_irn_loss(copy.deepcopy(net_1).double().train(), seqs, users, torch.float64).item()
        l32 = _stock_irn_loss(copy.deepcopy(net_1).train(), seqs, users, torch.float32).item()
    le_s = irn_s.get_loss_on_eval_data(my_seqs, my_users)
    le_1 = irn_1.get_loss_on_eval_data(seqs, users)
    bound = max(4 * abs(l32 - l64), 2e-6 * abs(l64))
    print(f"IRSNN eval loss: sharded {le_s!r} unsharded {le_1!r} f32 {l32!r} f64 {l64!r} bound {bound:.3e}")
    assert abs(le_s - le_1) <= bound
    _same_on_all_ranks(torch.tensor([le_s], dtype=torch.float64), world, "the eval loss")
    _check_training(irn_s, irn_1, net_s, net_1, lambda: irn_s.train_batch(my_seqs, my_users),
                    lambda: irn_1.train_batch(seqs, users), lambda m, dt: _stock_irn_loss(m, seqs, users, dt), 3, rank, world,
                    "IRSNN")
    # ---- Evaluator / SampleNet, one step
    g = np.load(os.path.join(REPO, "tests", "golden", "train_tiny.npz"))
    ecfg = synth.make_config("eval_tiny", dropout=0.0)
    esd = {k: torch.from_numpy(v) for k, v in synth.irn_state_dict(ecfg, 17, evaluator=True).items()}
    target = torch.from_numpy(g["ev_target"]).to(DEV)
    assert target.shape[0] % world == 0
    nets = []
    for _ in range(2):
        net = SampleNet(ecfg)
        net.load_state_dict(esd)
        nets.append(net.to(DEV))
    snet_s, snet_1 = nets
    snet_s.shard_items(rank, world)
    ev_s, ev_1 = Evaluator(ecfg, snet_s, DEV), Evaluator(ecfg, snet_1, DEV)
    per = target.shape[0] // world
    mine = target[rank * per:(rank + 1) * per].contiguous()
    with torch.no_grad():
        l64 = _stock_eval_loss(copy.deepcopy(snet_1).double().train(), target, torch.float64).item()
        l32 = _stock_eval_loss(copy.deepcopy(snet_1).train(), target, torch.float32).item()
    le_s, le_1 = ev_s.get_loss_on_eval_data(mine), ev_1.get_loss_on_eval_data(target)
    bound = max(4 * abs(l32 - l64), 2e-6 * abs(l64))
    print(f"Evaluator eval loss: sharded {le_s!r} unsharded {le_1!r} f32 {l32!r} f64 {l64!r} bound {bound:.3e}")
    assert abs(le_s - le_1) <= bound
    _check_training(ev_s, ev_1, snet_s, snet_1, lambda: ev_s.train_batch(mine), lambda: ev_1.train_batch(target),
                    lambda m, dt: _stock_eval_loss(m, target, dt), 1, rank, world, "Evaluator")


CASES = {"float64": _case_float64, "world1": _case_world1, "edges": _case_edges, "front_end": _case_front_end}


def _worker(rank, world, port, ret, case):
    import faulthandler
    import sys
    faulthandler.dump_traceback_later(100, exit=True)  # a stuck rank reports where, and dies
    sys.path.insert(0, REPO)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(torch.device(DEV))
        CASES[case](rank, world)
        torch.cuda.synchronize()
        ret[rank] = 1
    finally:
        dist.destroy_process_group()


def _run(world, case, limit=110):
    """Spawn the ranks; stop at the first failure: a rank that exits non-zero (or the time limit) ends the others."""
    assert world <= 3
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret, case)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        t_end = time.monotonic() + limit
        live = list(procs)
        while live and time.monotonic() < t_end:
            live[0].join(0.2)
            codes = [p.exitcode for p in procs]
            assert not [c for c in codes if c not in (None, 0)], f"rank exit codes {codes}"
            live = [p for p in procs if p.exitcode is None]
        assert not live, f"ranks still running after {limit} s: exit codes {[p.exitcode for p in procs]}"
    finally:
        for p in procs:  # never leave a rank behind
            if p.is_alive():
                p.kill()
            p.join(10)
    assert sorted(ret.keys()) == list(range(world))


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_loss_and_gradients_match_float64(world):
    _run(world, "float64")


def test_world1_equals_the_single_device_entry_points_bit_for_bit():
    _run(1, "world1")


def test_determinism_accumulate_bad_labels_and_all_ignored_world2():
    _run(2, "edges")


def test_front_end_world2_tracks_the_unsharded_handlers():
    _run(2, "front_end")
