"""-m gpu: training and the front end behind a long window (max_len = 272).

The native trunk (irs_train_forward / irs_train_backward) tiles keys by 64 with a log-sum-exp and is not sized by the window: at
L = 272 its loss and every live gradient are compared with train_trunk_ref.functional_trunk in float64, at p = 0 and at p = 0.1 with
the documented dropout masks, by the tolerances of tests/test_gpu_train_trunk.py (its _check: 4 x the float32 restatement's own error,
or 2e-6 relative).  The front end builds its engines through irs_create_ex: IRSNN with config.max_len = 272 searches the paths of
oracle.get_seq, trains a batch and evaluates a finite loss."""
import copy

import numpy as np
import pytest
import torch

from influentialrs_amd import synth
from influentialrs_amd.engine import IrsError
from influentialrs_amd.model.influentialRS import IRSNN, InfluentialNet
from test_gpu_train_trunk import _check, _native, _run, _setup
from train_trunk_ref import functional_trunk, trunk_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 272


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_native_trunk_gradients_at_272(p):
    cfg, net, seq, user, R = _setup("tiny", 3, max_len=L)
    assert seq.shape == (3, L)
    dims = (3, L, cfg.emb_dim, cfg.n_heads, cfg.ffn_dim, cfg.max_len, cfg.n_layers)
    net64 = copy.deepcopy(net).double()
    net.dropout = net64.dropout = p
    torch.manual_seed(99)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())  # what the trunk draws for its step
    masks = trunk_masks(seed, p, *dims)
    torch.manual_seed(99)
    nat = _native(net, seq, user, R)
    f32 = _run(net, lambda: functional_trunk(net, seq, user, masks, torch.float32), R)
    f64 = _run(net64, lambda: functional_trunk(net64, seq, user, masks), R)
    _check(nat, f32, f64, cfg.emb_dim, f"tiny L={L} p={p}")


def _irsnn(max_len, n_item=2000):
    cfg = synth.make_config("tiny", max_len=max_len, n_item=n_item, dropout=0.0)
    sd = synth.irn_state_dict(cfg, 1234)
    net = InfluentialNet(cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.to(DEV)
    return cfg, sd, net, IRSNN(cfg, net, DEV)


def test_frontend_searches_trains_and_evaluates_at_272(oracle):
    cfg, sd, net, irn = _irsnn(L)
    B, P = 6, 5
    seqs = synth.random_windows(B, L, cfg.n_item, seed=5, min_hist=200)
    seqs[0, :L - 1] = np.random.default_rng(6).permutation(cfg.n_item)[:L - 1] + 1  # a full window
    users = (np.arange(B) * 7 % cfg.n_user).astype(np.int64)
    targets = seqs[:, L - 1].copy()
    irn.eval()
    with torch.no_grad():
        paths, tt, hh, early = irn.get_seq_in_batch(torch.from_numpy(seqs).to(DEV), torch.from_numpy(users).to(DEV),
                                                    torch.from_numpy(targets).to(DEV), P, 0, False, 3)
    ref, _, ref_h, ref_early = oracle.get_seq(sd, cfg, seqs, users, targets, max_path_len=P)
    assert np.array_equal(paths, ref) and early == ref_early
    assert all(np.array_equal(a, b) for a, b in zip(hh, ref_h))
    net.trunk = "hip"
    seq_t, usr_t = torch.from_numpy(seqs).to(DEV), torch.from_numpy(users).to(DEV)
    loss = irn.train_batch(seq_t, usr_t)
    ev = irn.get_loss_on_eval_data(seq_t, usr_t)
    assert np.isfinite(loss) and np.isfinite(ev) and loss > 0 and ev > 0


def test_beyond_1024_the_librarys_message_surfaces():
    cfg, sd, net, irn = _irsnn(1025, n_item=300)
    seqs = torch.from_numpy(synth.random_windows(1, 1025, cfg.n_item, seed=1)).to(DEV)
    with pytest.raises(IrsError, match=r"max_len must be in \[2, 1024\]"), torch.no_grad():
        irn.eval()
        irn.get_seq_in_batch(seqs, torch.zeros(1, dtype=torch.int64, device=DEV), seqs[:, -1].clone(), 2, 0, False, 3)
