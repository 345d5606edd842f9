"""The sigmoid loss terms inside the train steps: the supervised step with [CrossEntropyLoss, FocalLoss] in both heads (shape and settings of
tests/test_dice_step_gpu.py: b = 2, 128 x 128, six classes, dropout 0), one PFGST step, and a CrossEntropyLoss(use_sigmoid=True) head.

Linearity needs no oracle: at fixed batch statistics the network is linear in dL/dlogits, so the gradient arena of the [CE, Focal] step is
arena(CE only) + arena(Focal only), norm-wise within 1e-3 (the `north_star` tolerance).  Measured on an MI355X: 7.6e-6.

Unlike Dice, the sigmoid terms honour the pixel weights: on the PFGST mixed pass the Focal gradient follows the pseudo-label confidence and is
exactly 0 in every low-resolution cell whose whole footprint has weight 0."""
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from helpers import model_cfg, seeded_pfgst_state, to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SGD = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005)
CE = lambda w: dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=w)
BCE = lambda w: dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=w, class_weight=[1.0, 1.0, 1.0, 1.0, 2.0, 1.5])
FOCAL = lambda w: dict(type='FocalLoss', loss_weight=w, gamma=2.0, alpha=[0.25, 0.25, 0.25, 0.25, 0.75, 0.5])
# the Focal term's mean runs over N C H W elements: weights that keep it beside the CE term
HEADS = {'ce': (CE(1.0), CE(0.4)), 'focal': (FOCAL(20.0), FOCAL(8.0)), 'both': ([CE(1.0), FOCAL(20.0)], [CE(0.4), FOCAL(8.0)]),
         'bce': (BCE(1.0), BCE(0.4))}
KEYS = ['decode.loss_ce', 'decode.loss_focal', 'decode.acc_seg', 'aux.loss_ce', 'aux.loss_focal', 'aux.acc_seg', 'loss']


def cfg_with(heads):
    cfg = model_cfg(dropout=0.0)
    cfg['decode_head']['loss_decode'], cfg['auxiliary_head']['loss_decode'] = heads
    return cfg


def sup_batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return {k: v for k, v in synth_batch(2, 128, 6, seed=seed).items() if not k.startswith('target_')}


def sup_step(heads, batch):
    """a fresh segmentor from the seeded state, one train_step -> (log_vars, the gradient arena, how far the step moved conv_seg's weight)"""
    import pfst_amd  # noqa: F401
    from oracle import pfst_oracle as O
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import fill_state_dict
    model = build_segmentor(cfg_with(heads))
    res = model.load_state_dict(fill_state_dict(O.init_state_dict(6, 3), 9), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    before = model.decode_head.conv_seg.weight.detach().clone()
    out = model.train_step(to_dev(batch, DEV), build_optimizer(model, dict(SGD)))
    torch.cuda.synchronize()
    assert out['loss'] == out['log_vars']['loss']
    moved = float((model.decode_head.conv_seg.weight.detach() - before).abs().max())
    return out['log_vars'], model.param_arena.grad.clone(), moved


@pytest.fixture(scope='module')
def runs():
    """every configuration once (and the list twice), in deterministic mode"""
    from pfst_amd import hip_ops
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        batch = sup_batch()
        return {name: sup_step(HEADS[name.split('_')[0]], batch) for name in ('ce', 'focal', 'both', 'both_again')}
    finally:
        hip_ops.set_deterministic(was)


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_log_vars_hold_the_focal_terms_and_loss_counts_them(runs):
    log = runs['both'][0]
    assert list(log) == KEYS
    assert all(np.isfinite(v) for v in log.values()), log
    assert log['decode.loss_focal'] > 0 and log['aux.loss_focal'] > 0
    total = sum(log[k] for k in KEYS if 'loss' in k and k != 'loss')
    assert abs(log['loss'] - total) <= 1e-6 * total
    # each term is what the one-term heads report for the same forward pass
    assert list(runs['ce'][0]) == [k for k in KEYS if 'loss_focal' not in k] and list(runs['focal'][0]) == [k for k in KEYS if 'loss_ce' not in k]
    for k in ('decode.loss_ce', 'aux.loss_ce', 'decode.acc_seg', 'aux.acc_seg'):
        assert log[k] == runs['ce'][0][k], k
    for k in ('decode.loss_focal', 'aux.loss_focal', 'decode.acc_seg', 'aux.acc_seg'):
        assert log[k] == runs['focal'][0][k], k


def test_gradient_is_the_sum_of_the_terms_gradients(runs):
    both, ce, focal = runs['both'][1], runs['ce'][1], runs['focal'][1]
    err = rel(both, ce.double() + focal.double())
    print(f'arena([CE, Focal]) vs arena(CE) + arena(Focal): norm-wise {err:.3e} (bound 1e-3); |CE| {float(ce.norm()):.3e} |Focal| {float(focal.norm()):.3e}')
    assert float(focal.norm()) > 1e-3 * float(ce.norm()) and float(ce.norm()) > 1e-3 * float(focal.norm()), 'both terms carry weight'
    assert err <= 1e-3


def test_deterministic_mode_is_bit_identical_run_to_run(runs):
    assert torch.equal(runs['both'][1], runs['both_again'][1])
    assert runs['both'][0] == runs['both_again'][0]


def test_out_of_range_label_raises_after_the_step():
    bad = sup_batch(56)
    bad['gt_semantic_seg'][0, 0, 40:44, 40:44] = 7
    for name in ('focal', 'both', 'bce'):
        with pytest.raises(ValueError, match='outside'):
            sup_step(HEADS[name], bad)


def test_a_sigmoid_ce_head_trains_one_step():
    log, grad, moved = sup_step(HEADS['bce'], sup_batch())
    assert list(log) == ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss']
    assert all(np.isfinite(v) for v in log.values()) and log['decode.loss_ce'] > 0 and log['aux.loss_ce'] > 0
    assert abs(log['loss'] - (log['decode.loss_ce'] + log['aux.loss_ce'])) <= 1e-6 * log['loss']
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    assert moved > 0, 'the optimizer moved the parameters'


def pfgst_step(threshold, batch, both):
    """one PFGST step with [CE, Focal] heads; records the Focal gradients (each term alone, into a buffer of its own) and the pixel weights
    they were given, in the order the backward sweep runs the closures"""
    import pfst_amd  # noqa: F401
    from oracle import pfst_oracle as O  # noqa: F401
    from pfst_amd import models
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import UDA
    cfg = uda_cfg(threshold=threshold)
    cfg['model']['decode_head']['loss_decode'], cfg['model']['auxiliary_head']['loss_decode'] = HEADS['both']
    model = UDA.build(cfg)
    model.load_state_dict(both, strict=False)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    seen, real = [], models.ops.sigloss_upsample_bwd

    def recording(ld, l8, coef, scale, gamma, weight, ign, out=None, accumulate=False):
        seen.append((real(ld, l8, coef, scale, gamma, weight, ign).clone(), None if weight is None else weight.clone()))
        return real(ld, l8, coef, scale, gamma, weight, ign, out=out, accumulate=accumulate)
    models.ops.sigloss_upsample_bwd = recording
    try:
        random.seed(0); np.random.seed(0); torch.manual_seed(0)
        log = model.train_step(to_dev(batch, DEV), opt)['log_vars']
        torch.cuda.synchronize()
    finally:
        models.ops.sigloss_upsample_bwd = real
    return log, seen


def untouched_cells(weight, hw):
    """bool [N, h, w]: the low-resolution cells whose whole bilinear footprint has pixel weight 0 (the resize's adjoint of the weight map is 0)"""
    z = torch.zeros(weight.shape[0], 1, *hw, dtype=torch.float64, requires_grad=True)
    up = torch.nn.functional.interpolate(z, size=weight.shape[-2:], mode='bilinear', align_corners=False)
    (t,) = torch.autograd.grad(up, z, grad_outputs=weight.double().cpu().unsqueeze(1))
    return t[:, 0] == 0


def test_pfgst_step_with_loss_lists_and_focal_follows_the_pseudo_weights():
    from oracle import pfst_oracle as O
    from pfst_amd import hip_ops
    from pfst_amd.synthetic import synth_batch
    both, _, _ = seeded_pfgst_state(O, 9)
    batch = synth_batch(2, 128, 6, seed=1234)
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        # thre_type='all': the threshold sets the scalar pseudo-weight q of the target pixels and nothing else (labels are the arg-max):
        # every pixel confident (q = 1) against none (q = 0)
        log_a, g_a = pfgst_step(0.0, batch, OrderedDict((k, v.clone()) for k, v in both.items()))
        log_b, g_b = pfgst_step(1.01, batch, OrderedDict((k, v.clone()) for k, v in both.items()))
    finally:
        hip_ops.set_deterministic(was)
    for k in ('decode.loss_focal', 'aux.loss_focal', 'mix.decode.loss_focal', 'mix.aux.loss_focal', 'mix.decode.loss_ce'):
        assert k in log_a and np.isfinite(log_a[k]), k
    print('mixed-pass Focal under the two thresholds:', log_a['mix.decode.loss_focal'], log_b['mix.decode.loss_focal'])
    assert log_a['mix.decode.loss_focal'] != log_b['mix.decode.loss_focal'] and log_a['mix.aux.loss_focal'] != log_b['mix.aux.loss_focal']
    assert log_a['decode.loss_focal'] == log_b['decode.loss_focal'], 'the source pass carries no pseudo-weights'
    assert len(g_a) == len(g_b) == 4                       # the backward sweep runs the mixed pass's closures first: aux, decode
    for i in (0, 1):
        (ga, wa), (gb, wb) = g_a[i], g_b[i]
        assert wa is not None and wb is not None and float(wa.min()) == 1.0 and float(wb.min()) == 0.0 and float(wb.max()) == 1.0
        assert float(ga.abs().max()) > 0 and not torch.equal(ga, gb), i
        dead = untouched_cells(wb, gb.shape[-2:]).to(DEV)
        assert 0 < int(dead.sum()) < dead.numel(), 'the class mix leaves both kinds of cells'
        dead = dead.unsqueeze(1).expand_as(gb)
        assert not gb[dead].any(), 'exactly 0 where every weight of the footprint is 0'
        assert gb[~dead].any()
    for i in (2, 3):
        assert g_a[i][1] is None and torch.equal(g_a[i][0], g_b[i][0]), 'the source pass is the same under both thresholds'
