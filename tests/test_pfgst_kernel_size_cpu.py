"""PFGSTLoss kernel_size 5 / 7 and the full top_k range (1 .. kernel_size^2 - 1), CPU side: the module accepts exactly the
reference's reachable domain and refuses the rest, and the CPU oracle matches the executed reference's vectors
(tests/golden/make_golden_kernel_size.py -> pfgst_kernel_size.npz)."""
import os

import numpy as np
import pytest
import torch

from oracle import pfst_oracle as O

G = os.path.join(os.path.dirname(__file__), 'golden')
W6 = {k: 0.1 for k in ('src_pos', 'src_neg', 'sim_pos', 'sim_neg', 'src_pos_std', 'src_neg_std')}

# tests/golden/make_golden_kernel_size.py:KERNEL_SIZE_VARIANTS (PFGSTLoss config overrides)
KERNEL_SIZE_VARIANTS = {
    'k5_d1_top3': dict(kernel_size=5, dilation=1, top_k=3),
    'k5_d1_top16_gaussian': dict(kernel_size=5, dilation=1, top_k=16, sim_type='gaussian', sigma=8.0),
    'k7_d1_all_unfold_margin2': dict(kernel_size=7, dilation=1, top_k=None, detach_unfold=False, src_loss_type='margin2',
                                     margin=(0.6, 0.0)),
    'k5_d2_full_res': dict(kernel_size=5, dilation=2, top_k=3, downscale=None),
    'k3_top6': dict(kernel_size=3, top_k=6),
    'k5_d1_src_perc_proj': dict(kernel_size=5, dilation=1, top_k=8, src_perc=0.6, proj_net_cfg=dict(in_channels=32, out_channels=16)),
}


def module_cfg(name):
    """the PFGSTLoss config of a variant (the shipped loss config + the overrides)"""
    cfg = dict(kernel_size=3, dilation=2, top_k=3, weights=dict(W6), sim_type='cosine', feat_level=None, detach_unfold=True,
               downscale=0.5)
    cfg.update(KERNEL_SIZE_VARIANTS[name])
    return cfg


def oracle_opts(name):
    """the same variant as keyword arguments of oracle.pfst_oracle.pfgst_loss (which names the knobs k / dil)"""
    cfg = module_cfg(name)
    opts = dict(k=cfg['kernel_size'], dil=cfg['dilation'], top_k=cfg['top_k'], downscale=cfg['downscale'], sim_type=cfg['sim_type'],
                detach_unfold=cfg['detach_unfold'])
    for key in ('sigma', 'src_loss_type', 'margin', 'src_perc'):
        if key in cfg:
            opts[key] = cfg[key]
    return opts


def _close(a, b, rtol=1e-4, atol=1e-5):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert np.allclose(a, b, rtol=rtol, atol=atol), f'max abs err {err}'


@pytest.mark.parametrize('ks,top_k', [(3, 1), (3, 5), (3, 8), (3, None), (5, 1), (5, 12), (5, 24), (5, None), (7, 3), (7, 48), (7, None)])
def test_kernel_size_and_top_k_domain_is_accepted(ks, top_k):
    from pfst_amd.uda import PFGSTLoss
    for sim_type in ('cosine', 'gaussian'):
        loss = PFGSTLoss(top_k, 2, ks, dict(W6), sim_type=sim_type, detach_unfold=True, downscale=0.5)
        assert loss.kernel_size == ks and loss.top_k == top_k


@pytest.mark.parametrize('over', [dict(kernel_size=4), dict(kernel_size=9), dict(kernel_size=1), dict(kernel_size=3, top_k=9),
                                  dict(kernel_size=5, top_k=25), dict(kernel_size=7, top_k=49), dict(kernel_size=5, top_k=0),
                                  dict(kernel_size=5, cross_prob_type='ema')])
def test_outside_the_domain_fails_loudly(over):
    from pfst_amd.uda import PFGSTLoss
    cfg = dict(top_k=3, dilation=2, kernel_size=3, weights=dict(W6), sim_type='cosine')
    cfg.update(over)
    with pytest.raises(NotImplementedError):
        PFGSTLoss(**cfg)


@pytest.mark.parametrize('name', list(KERNEL_SIZE_VARIANTS))
def test_oracle_matches_the_reference_at_every_kernel_size(name):
    z = np.load(os.path.join(G, 'pfgst_kernel_size.npz'))
    assert name in list(z['variants'])
    assert int(z[name + '|n_valid']) > 1
    lt = torch.from_numpy(z['logits_trg']).requires_grad_()
    xs = torch.from_numpy(z['x_src']).requires_grad_()
    proj = None
    if name + '|proj_weight' in z:
        proj = (torch.from_numpy(z[name + '|proj_weight']).requires_grad_(), torch.from_numpy(z[name + '|proj_bias']).requires_grad_())
    losses, ex = O.pfgst_loss(lt, torch.from_numpy(z['x_ema']), xs, torch.from_numpy(z['gt_src']), torch.from_numpy(z['mix_masks']),
                              O.DEFAULT_LOSS_W, proj=proj, **oracle_opts(name))
    assert list(losses) == list(z[name + '|names'])
    _close(np.array([float(v.detach().sum()) for v in losses.values()]), z[name + '|losses'], 1e-5, 1e-7)
    sum(v.sum() for v in losses.values()).backward()
    _close(lt.grad, z[name + '|grad_logits'], 1e-4, 1e-9)
    _close(xs.grad, z[name + '|grad_xsrc'], 1e-4, 1e-9)
    _close(ex['density'], z[name + '|density'], 1e-5)
    if proj is not None:
        _close(proj[0].grad, z[name + '|grad_proj_weight'], 1e-4, 1e-9)
        _close(proj[1].grad, z[name + '|grad_proj_bias'], 1e-4, 1e-9)
