"""Round 6: the sequence-resident decoder's plan with its tail rule (k_plan_seq) and the idle path of empty waves (k_block_x6).

One workgroup fits a CU, so the launch runs in rounds of n_cu workgroups.  When the last round is short the plan opens
half-live workgroups for it (at most 8 blocks, live tiles on waves 4 .. 7 only).  The batches here put the last round at about
0.1 / 0.25 / 0.4 / 0.6 / 0.9 of a round of THIS device's CU count, one has windows of 1 .. L tokens, one has only sequences too long
for the tail.  For each of them:
  * the plan's decision and its counts of full and half-live workgroups equal a host replica of the rule (so a plan that never
    takes the rule fails), and the 0.1 and 0.25 batches do take it;
  * the plan read back through irs_debug_ptr places every block of every sequence exactly once, keeps sequences of more than
    8 blocks out of the half-live workgroups, keeps their live tiles on one wave per SIMD, gives them the highest ids, and stays
    inside the launch's grid (one workgroup per sequence);
  * two decodes of the batch give the same bits;
  * the two-kernel path (irs_set_decoder_seq off) gives rows within X_TOL[IRS_GEMM_H3] of test_gpu_throughput_goldens.py -- the
    bound both paths meet there against the reference.
"""
import numpy as np
import pytest
import torch

import bench
from gpu_util import make_engine
from influentialrs_amd import synth
from influentialrs_amd._lib import IRS_GEMM_H3
from test_gpu_throughput_goldens import X_TOL

pytestmark = pytest.mark.gpu

C, CT = 16, 8  # half tiles (blocks of 16 tokens) of a workgroup; of a half-live one
B_MAX = 2048


def count_plan(nb, cap=None):
    """Host replica of the plan's counting: best fit, largest class first, on the counts of workgroups per free-block number.
    Full workgroups (16 blocks) are opened while fewer than `cap` exist (None: always), half-live ones (8 blocks) behind it.
    Returns (workgroups, those opened by the classes of more than 8 blocks, half-live ones)."""
    hist = np.bincount(nb, minlength=C + 1)
    cnt, n, nbig, ntail = [0] * C, 0, 0, 0
    for T in range(C, 0, -1):
        left = int(hist[T])
        for f in range(T, C):
            if left == 0:
                break
            q = f // T
            used = min(left, cnt[f] * q)
            left -= used
            fl, pa = divmod(used, q)
            cnt[f] -= fl + (1 if pa else 0)
            cnt[f - T * q] += fl
            if pa:
                cnt[f - T * pa] += 1
        q = C // T
        if cap is not None and T <= CT and max(cap - n, 0) * q < left:
            room, qt = max(cap - n, 0), CT // T
            fl, pa = divmod(left - room * q, qt)
            left = room * q
            cnt[CT - T * qt] += fl
            n += fl + (1 if pa else 0)
            ntail += fl + (1 if pa else 0)
            if pa:
                cnt[CT - T * pa] += 1
        fl, pa = divmod(left, q)
        cnt[C - T * q] += fl
        n += fl + (1 if pa else 0)
        if pa:
            cnt[C - T * pa] += 1
        if T == CT + 1:
            nbig = n
    return n, nbig, ntail


def plain_workgroups(nb):
    return count_plan(nb)[0]


def expected_plan(nb, n_cu):
    """The rule as the issue and k_plan_seq's comment state it: (full workgroups, half-live workgroups)."""
    n, nbig, _ = count_plan(nb)
    rounds, rem = divmod(n, n_cu)
    if rem > 0 and 2 * rem <= n_cu and nbig <= rounds * n_cu:
        n2, _, ntail = count_plan(nb, rounds * n_cu)
        if ntail <= n_cu:
            return n2 - ntail, ntail
    return n, 0


@pytest.fixture(scope="module")
def rig():
    dev = torch.device("cuda:0")
    cfg = synth.make_config("c2", n_layers=2)
    sd = synth.irn_state_dict(cfg, 1234)
    eng = make_engine(cfg, sd, max_rows=B_MAX, max_seqs=B_MAX)
    eng.decoder_gemm = IRS_GEMM_H3
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    yield cfg, eng, dev, n_cu
    eng.decoder_seq = None


def _windows(cfg, dev, kind):
    L = cfg.max_len
    seqs = bench.gpu_windows(B_MAX, L, cfg.n_item, dev, seed=5)
    if kind in ("ramp", "long"):
        full = seqs.clone()
        full[full == 0] = 7
        col = torch.arange(L, device=dev)[None, :]
        i = torch.arange(B_MAX, device=dev)
        n = (1 + i % L) if kind == "ramp" else (L - i % (L - 16 * CT - 1))  # 1 .. L tokens; more than 8 blocks each
        seqs = torch.where(col >= L - n[:, None], full, torch.zeros_like(full))
    return seqs


def _decode(eng, seqs, users, pos, on):
    eng.decoder_seq = on
    xr = eng.decode(seqs, users, want_x=False, pos=pos)[1].clone()
    torch.cuda.synchronize()
    assert eng.decoder_seq_last == bool(on)
    return xr


def _check(rig, kind, frac):
    cfg, eng, dev, n_cu = rig
    L = cfg.max_len
    seqs = _windows(cfg, dev, kind)
    users = torch.randint(0, cfg.n_user, (B_MAX,), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pos = torch.full((B_MAX,), L - 2, dtype=torch.int32, device=dev)
    # token counts of the plan (one decode of everything), then the prefix of the batch whose last round is nearest `frac`
    _decode(eng, seqs, users, pos, 1)
    cnt_all = eng.debug_buffer(8, B_MAX, torch.int32).clone().cpu().numpy()
    nb_all = np.clip((cnt_all + 15) // 16, 1, C)
    B = B_MAX
    if frac is not None:
        best = None
        for b in range(384, B_MAX + 1, 8):
            n = plain_workgroups(nb_all[:b])
            if n < 2 * n_cu:  # (from two whole rounds up the bench windows' long sequences leave the rule room)
                continue
            d = abs((n % n_cu) / n_cu - frac)
            if best is None or d < best[0]:
                best = (d, b, n)
        assert best is not None and best[0] < 0.05, best
        B = best[1]
    seqs, users, pos = seqs[:B].contiguous(), users[:B].contiguous(), pos[:B].contiguous()
    a = _decode(eng, seqs, users, pos, 1)
    # ---- the plan
    nwg, tail0 = (int(v) for v in eng.debug_buffer(6, 2, torch.int32).cpu().numpy())
    cnt = eng.debug_buffer(8, B, torch.int32).clone().cpu().numpy()
    nb = np.clip((cnt + 15) // 16, 1, C)
    tseq = eng.debug_buffer(2, B * 16, torch.int32).clone().cpu().numpy()
    tqb = eng.debug_buffer(3, B * 16, torch.int32).clone().cpu().numpy()
    n_plain = plain_workgroups(nb)
    print(f"{kind} frac={frac}: {B} sequences, {int(nb.sum())} blocks, plain plan {n_plain} workgroups = {n_plain / n_cu:.2f} rounds of "
          f"{n_cu}; plan: {tail0} full + {nwg - tail0} half-live")
    want_full, want_tail = expected_plan(nb, n_cu)
    print(f"  expected: {want_full} full + {want_tail} half-live")
    assert (tail0, nwg - tail0) == (want_full, want_tail), "the rule's decision and its counts"
    assert 0 < nwg <= B, "the launch's grid is one workgroup per sequence"
    assert 0 <= tail0 <= nwg
    assert (tseq[16 * nwg:] < 0).all(), "nothing is placed behind the workgroups in use"
    used = np.nonzero(tseq[:16 * nwg] >= 0)[0]
    seen = np.zeros((B, C), dtype=np.int32)
    np.add.at(seen, (tseq[used], tqb[used]), 1)
    want = (np.arange(C)[None, :] < nb[:, None]).astype(np.int32)
    assert np.array_equal(seen, want), "every block of every sequence exactly once"
    wg_of = used // 16
    first = np.full(B, -1)
    first[tseq[used]] = wg_of
    assert np.array_equal(first[tseq[used]], wg_of), "a sequence sits in one workgroup"
    live = np.zeros((nwg, 8), dtype=bool)
    live[wg_of, (used % 16) // 2] = True
    assert live.any(1).all(), "no empty workgroup"
    for w in range(tail0, nwg):  # half-live workgroups: the highest ids by construction of tail0; what they may hold
        assert not (live[w, :4] & live[w, 4:]).any(), "two live waves on one SIMD (waves w and w + 4 share one)"
        assert live[w].sum() <= 4
        assert nb[tseq[16 * w:16 * w + 16][tseq[16 * w:16 * w + 16] >= 0]].max() <= CT
    if tail0 < nwg:
        assert (live[:tail0].sum(1) > 0).all() and tail0 % n_cu == 0, "full workgroups fill whole rounds in front of the tail"
    if kind == "long":
        assert tail0 == nwg, "nothing is eligible for the tail"
    # ---- the rows
    b2 = _decode(eng, seqs, users, pos, 1)
    assert torch.equal(a.view(torch.int32), b2.view(torch.int32)), "two runs of one batch: the same bits"
    ref = _decode(eng, seqs, users, pos, 0)
    assert not torch.isnan(a).any() and not torch.isnan(ref).any()
    err = float((a - ref).abs().max())
    print(f"  sequence-resident vs two-kernel rows: max {err:.3g} (bound {X_TOL[IRS_GEMM_H3]:.3g})")
    assert err < X_TOL[IRS_GEMM_H3], err
    return tail0, nwg


@pytest.mark.parametrize("frac", [0.1, 0.25, 0.4, 0.6, 0.9])
def test_last_round_fraction(rig, frac):
    tail0, nwg = _check(rig, "bench", frac)
    if frac > 0.5:
        assert tail0 == nwg, "a last round above half a round stays as it was"
    if frac <= 0.25:
        assert tail0 < nwg, "a short last round behind two whole ones: the rule applies"


def test_windows_of_every_length(rig):
    _check(rig, "ramp", None)


def test_only_long_sequences(rig):
    _check(rig, "long", None)
