"""-m gpu: the captured steps of the search loops (irs_replay_steps, irs_drop_graphs in csrc/capi.hip).

A captured step bakes in every argument of its call, the workspace addresses and the kernel choices.  These tests change
one of them at a time between two use_graph=True calls and compare with the same call on plain stream launches: a cache
key that misses a field, or a setter that forgets to drop the caches, replays the previous call's step and shows up as a
different result or as a write into the previous call's buffers.  Every comparison is torch.equal: no tolerance."""
import numpy as np
import pytest
import torch

from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_GEMM_F32, IRS_PROF_LINEAR, IRS_PROF_NONE, IRS_SWEEP_BF16
from influentialrs_amd.engine import _ptr
from gpu_util import make_engine

pytestmark = pytest.mark.gpu

N_USERS = 4
PATH_CAP = 8        # floats per user in a greedy `paths` allocation: every path length used below fits
F_SENTINEL = -7.0   # no item id, no window entry and no status word has these values
I_SENTINEL = -7


@pytest.fixture(scope="module")
def tiny():
    cfg = synth.make_config("tiny")
    sd = synth.irn_state_dict(cfg, 1234)
    hists = synth.user_histories(8, cfg.n_item, seed=7)
    rows = synth.eval_rows(hists, cfg.n_item, seed=11)[:N_USERS]
    _, seqs, users, targets, _ = synth.collate_eval_irs(rows, cfg.max_len, gap_len=0)
    return cfg, sd, seqs, users, targets


def _engine(tiny):
    cfg, sd = tiny[:2]
    return make_engine(cfg, sd, max_rows=16, max_seqs=16)


class GreedyBufs:
    """The caller's five buffers of irs_generate_paths, allocated once so that a test decides which address changes."""
    NAMES = ("seq", "users", "hep", "paths", "status")

    def __init__(self, tiny):
        cfg, _, seqs, users, _ = tiny
        self.L = cfg.max_len
        self.seq0 = torch.from_numpy(seqs).cuda()
        self.users0 = torch.from_numpy(users).cuda()
        for name in self.NAMES:
            self.fresh(name)

    def fresh(self, name):
        """Replaces one buffer by a new allocation (the old one stays alive with the caller) and returns the old one."""
        old = getattr(self, name, None)
        new = {"seq": lambda: torch.empty_like(self.seq0), "users": lambda: self.users0.clone(),
               "hep": lambda: torch.empty(N_USERS, dtype=torch.int32, device="cuda"),
               "paths": lambda: torch.empty(N_USERS * PATH_CAP, dtype=torch.float32, device="cuda"),
               "status": lambda: torch.empty(N_USERS, dtype=torch.int32, device="cuda")}[name]()
        assert old is None or new.data_ptr() != old.data_ptr()
        setattr(self, name, new)
        return old

    def run(self, eng, use_graph, B=N_USERS, P=5, **kw):
        """One search from the initial windows.  Returns clones of (paths, status, windows, history ends) and, last, of
        whatever lies behind the call's share of the paths / status allocations (it must keep its sentinel)."""
        self.seq.copy_(self.seq0)
        self.hep.fill_(self.L - 2)
        self.paths.fill_(F_SENTINEL)
        self.status.fill_(I_SENTINEL)
        paths = self.paths[:B * P].view(B, P)
        eng.generate_paths(self.seq[:B], self.users[:B], self.hep[:B], P, use_graph=use_graph, paths=paths,
                           status=self.status[:B], **kw)
        return (paths.clone(), self.status[:B].clone(), self.seq[:B].clone(), self.hep[:B].clone(),
                self.paths[B * P:].clone(), self.status[B:].clone())


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), (g, w)


def _poison(t):
    t.fill_(F_SENTINEL if t.is_floating_point() else I_SENTINEL)
    return t.clone()


def test_greedy_key_holds_every_argument(tiny):
    eng = _engine(tiny)
    g, s = GreedyBufs(tiny), GreedyBufs(tiny)  # the graph calls' buffers, the stream calls'
    _same(g.run(eng, True), s.run(eng, False))
    _same(g.run(eng, True), s.run(eng, False))  # (the same key again: a replay of the cached step)
    for name in ("paths", "status", "seq", "hep", "users"):  # one other address: the previous call's buffer stays as it is
        old = g.fresh(name)
        was = _poison(old)
        _same(g.run(eng, True), s.run(eng, False))
        assert torch.equal(old, was), name
    # other counts behind the SAME addresses.  (B = 3: the fourth user's share of paths / status keeps its sentinel, which
    # the comparison of the tails in run() checks; a replay of the four-user step would fill it.)
    for kw in (dict(B=3), dict(P=7), dict(P=5), dict(k=50), dict(sample=True, seed=1), dict(sample=True, seed=2),
               dict(sample=True, sample_k=2, seed=2), dict()):
        _same(g.run(eng, True, **kw), s.run(eng, False, **kw))


def _beam(eng, seqs, users, hep, W, P, k, use_graph, status):
    """Engine.beam_search with the caller's `status` buffer (the one caller pointer a captured beam step bakes in)."""
    B = seqs.shape[0]
    paths = torch.zeros((B, W, P), dtype=torch.float32, device="cuda")
    scores = torch.zeros((B, W), dtype=torch.float64, device="cuda")
    fin = torch.empty((B, W, eng.L), dtype=torch.int64, device="cuda")
    status.fill_(I_SENTINEL)
    eng._call(eng.lib.irs_beam_search, _ptr(seqs), _ptr(users), _ptr(hep), B, W, P, k, IRS_SWEEP_BF16, int(use_graph),
              _ptr(paths), _ptr(scores), _ptr(fin), _ptr(status))
    return paths, scores, fin, status.clone()


def _beam_inputs(tiny):
    cfg, _, seqs, users, _ = tiny
    hep = torch.full((N_USERS,), cfg.max_len - 2, dtype=torch.int32, device="cuda")
    return torch.from_numpy(seqs).cuda(), torch.from_numpy(users).cuda(), hep


def test_beam_key_holds_every_argument(tiny):
    eng = _engine(tiny)
    seqs, users, hep = _beam_inputs(tiny)
    st_g = torch.empty(N_USERS, dtype=torch.int32, device="cuda")
    st_s = torch.empty_like(st_g)

    def both(W, P, k, status=st_g):
        _same(_beam(eng, seqs, users, hep, W, P, k, True, status), _beam(eng, seqs, users, hep, W, P, k, False, st_s))

    both(2, 4, 100)
    both(2, 4, 100)  # (the same key again)
    st_new = torch.empty_like(st_g)
    assert st_new.data_ptr() != st_g.data_ptr()
    st_g.fill_(I_SENTINEL)
    both(2, 4, 100, st_new)
    assert bool((st_g == I_SENTINEL).all())  # (the previous call's status buffer: a replay of its step would put its flags there)
    both(3, 4, 100)
    for P in (1, 2, 5, 4):  # no graph; one replay; two replays and an odd last step on the stream; back
        both(3, P, 100)
    both(3, 4, 50)
    both(2, 4, 100)


def test_setters_drop_the_captured_steps(tiny, oracle):
    cfg, sd, seqs, users, targets = tiny
    eng = _engine(tiny)
    g, s = GreedyBufs(tiny), GreedyBufs(tiny)
    bseq, busers, bhep = _beam_inputs(tiny)
    st_g = torch.empty(N_USERS, dtype=torch.int32, device="cuda")
    st_s = torch.empty_like(st_g)

    def check():
        got = g.run(eng, True)
        _same(got, s.run(eng, False))
        _same(_beam(eng, bseq, busers, bhep, 2, 4, 100, True, st_g), _beam(eng, bseq, busers, bhep, 2, 4, 100, False, st_s))
        return got

    before = check()
    # 1. another workspace; the old one stays allocated and is poisoned: a stale step would compute on NaN
    old_ws = eng._ws
    eng._ws = torch.empty_like(old_ws)
    eng._check(eng.lib.irs_bind_workspace(eng.h, _ptr(eng._ws), eng._ws.numel()))
    old_ws[:old_ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    _same(check(), before)
    # 2. another weight, in place (the addresses stay): the last layer's output norm negated turns the ranking over
    name = f"decoder.layers.{cfg.n_layers - 1}.norm3.weight"
    sd2 = dict(sd)
    sd2[name] = -sd[name]
    want, want2 = (oracle.get_seq(w, cfg, seqs, users, targets, max_path_len=5)[0] for w in (sd, sd2))
    assert not np.array_equal(want, want2)  # (on the CPU oracle: the perturbation changes path ids)
    eng._weights[name].neg_()
    eng.finalize()
    after = check()
    assert not torch.equal(after[0], before[0])
    # 3, 4. another decoder arithmetic, another layer-kernel choice
    eng.decoder_gemm = IRS_GEMM_F32
    assert eng.decoder_gemm == IRS_GEMM_F32
    check()
    eng.decoder_seq = 0 if eng.decoder_seq else 1
    check()


def test_greedy_and_beam_caches_are_independent(tiny):
    eng = _engine(tiny)
    g, s = GreedyBufs(tiny), GreedyBufs(tiny)
    seqs, users, hep = _beam_inputs(tiny)
    st_g = torch.empty(N_USERS, dtype=torch.int32, device="cuda")
    st_s = torch.empty_like(st_g)
    want_g = s.run(eng, False)
    want_b = _beam(eng, seqs, users, hep, 2, 4, 100, False, st_s)
    for _ in range(2):  # greedy, beam, greedy, beam: each with its first call's arguments
        _same(g.run(eng, True), want_g)
        _same(_beam(eng, seqs, users, hep, 2, 4, 100, True, st_g), want_b)


def test_profiling_runs_the_steps_on_the_stream(tiny):
    eng = _engine(tiny)
    g, s = GreedyBufs(tiny), GreedyBufs(tiny)
    want = s.run(eng, False)
    _same(g.run(eng, True), want)  # (a captured step exists before profiling is switched on)
    eng.prof_enable(IRS_PROF_LINEAR)
    _same(g.run(eng, True), want)
    launches = eng.prof_read()[0]
    assert launches > 0  # the use_graph call recorded its brackets: it ran on the stream
    eng.prof_enable(IRS_PROF_NONE)
    _same(g.run(eng, True), want)
