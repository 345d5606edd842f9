"""Loss lists inside the train steps: the supervised step with [CrossEntropyLoss, DiceLoss] in both heads (shape and settings of
tests/test_supervised_gpu.py's step test: b = 2, 128 x 128, six classes, dropout 0) and one PFGST step.

Linearity needs no oracle: at fixed batch statistics the network is linear in dL/dlogits, so the gradient arena of the [CE, Dice] step is
arena(CE only) + arena(Dice only), norm-wise within 1e-3 (the `north_star` tolerance).  Measured on an MI355X: 7.6e-6."""
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
DICE = lambda w: dict(type='DiceLoss', loss_weight=w)
HEADS = {'ce': (CE(1.0), CE(0.4)), 'dice': (DICE(3.0), DICE(1.2)), 'both': ([CE(1.0), DICE(3.0)], [CE(0.4), DICE(1.2)])}
KEYS = ['decode.loss_ce', 'decode.loss_dice', 'decode.acc_seg', 'aux.loss_ce', 'aux.loss_dice', 'aux.acc_seg', 'loss']


def cfg_with(heads):
    cfg = model_cfg(dropout=0.0)
    cfg['decode_head']['loss_decode'], cfg['auxiliary_head']['loss_decode'] = heads
    return cfg


def sup_batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return {k: v for k, v in synth_batch(2, 128, 6, seed=seed).items() if not k.startswith('target_')}


def sup_step(heads, batch):
    """a fresh segmentor from the seeded state, one train_step -> (log_vars, the gradient arena)"""
    import pfst_amd  # noqa: F401
    from oracle import pfst_oracle as O
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import fill_state_dict
    model = build_segmentor(cfg_with(heads))
    res = model.load_state_dict(fill_state_dict(O.init_state_dict(6, 3), 9), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    out = model.train_step(to_dev(batch, DEV), build_optimizer(model, dict(SGD)))
    torch.cuda.synchronize()
    assert out['loss'] == out['log_vars']['loss']
    return out['log_vars'], model.param_arena.grad.clone()


@pytest.fixture(scope='module')
def runs():
    """every configuration once (and the list twice), in deterministic mode"""
    from pfst_amd import hip_ops
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        batch = sup_batch()
        return {name: sup_step(HEADS[name.split('_')[0]], batch) for name in ('ce', 'dice', 'both', 'both_again')}
    finally:
        hip_ops.set_deterministic(was)


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_log_vars_hold_the_dice_terms_and_loss_counts_them(runs):
    log = runs['both'][0]
    assert list(log) == KEYS
    assert all(np.isfinite(v) for v in log.values()), log
    assert log['decode.loss_dice'] > 0 and log['aux.loss_dice'] > 0
    total = sum(log[k] for k in KEYS if 'loss' in k and k != 'loss')
    assert abs(log['loss'] - total) <= 1e-6 * total
    # each term is what the one-term heads report for the same forward pass
    assert list(runs['ce'][0]) == [k for k in KEYS if 'loss_dice' not in k] and list(runs['dice'][0]) == [k for k in KEYS if 'loss_ce' not in k]
    for k in ('decode.loss_ce', 'aux.loss_ce', 'decode.acc_seg', 'aux.acc_seg'):
        assert log[k] == runs['ce'][0][k], k
    for k in ('decode.loss_dice', 'aux.loss_dice', 'decode.acc_seg', 'aux.acc_seg'):
        assert log[k] == runs['dice'][0][k], k


def test_gradient_is_the_sum_of_the_terms_gradients(runs):
    both, ce, dice = runs['both'][1], runs['ce'][1], runs['dice'][1]
    err = rel(both, ce.double() + dice.double())
    print(f'arena([CE, Dice]) vs arena(CE) + arena(Dice): norm-wise {err:.3e} (bound 1e-3); |CE| {float(ce.norm()):.3e} |Dice| {float(dice.norm()):.3e}')
    assert float(dice.norm()) > 1e-3 * float(ce.norm()) and float(ce.norm()) > 1e-3 * float(dice.norm()), 'both terms carry weight'
    assert err <= 1e-3


def test_deterministic_mode_is_bit_identical_run_to_run(runs):
    assert torch.equal(runs['both'][1], runs['both_again'][1])
    assert runs['both'][0] == runs['both_again'][0]


def test_out_of_range_label_raises_after_the_step():
    bad = sup_batch(56)
    bad['gt_semantic_seg'][0, 0, 40:44, 40:44] = 7
    for name in ('dice', 'both'):
        with pytest.raises(ValueError, match='outside'):
            sup_step(HEADS[name], bad)


def pfgst_step(threshold, batch, both):
    """one PFGST step with [CE, Dice] heads; records the mixed pass's Dice gradients (the first two Dice closures the backward sweep runs)"""
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
    grads, real = [], models.ops.dice_upsample_bwd

    def recording(ld, l8, lse, coef, scale, ign, e, out=None, accumulate=False):
        grads.append(real(ld, l8, lse, coef, scale, ign, e).clone())        # the term alone, into a buffer of its own
        return real(ld, l8, lse, coef, scale, ign, e, out=out, accumulate=accumulate)
    models.ops.dice_upsample_bwd = recording
    try:
        random.seed(0); np.random.seed(0); torch.manual_seed(0)
        log = model.train_step(to_dev(batch, DEV), opt)['log_vars']
        torch.cuda.synchronize()
    finally:
        models.ops.dice_upsample_bwd = real
    return log, grads


def test_pfgst_step_with_loss_lists_and_dice_ignores_the_pseudo_weights():
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
    for k in ('decode.loss_dice', 'aux.loss_dice', 'mix.decode.loss_dice', 'mix.aux.loss_dice', 'mix.decode.loss_ce'):
        assert k in log_a and np.isfinite(log_a[k]), k
    print('mixed-pass CE under the two thresholds:', log_a['mix.decode.loss_ce'], log_b['mix.decode.loss_ce'])
    assert log_a['mix.decode.loss_ce'] != log_b['mix.decode.loss_ce'], 'the pseudo-weights did change'
    assert log_a['mix.decode.loss_dice'] == log_b['mix.decode.loss_dice'] and log_a['mix.aux.loss_dice'] == log_b['mix.aux.loss_dice']
    assert len(g_a) == len(g_b) == 4                       # the backward sweep runs the mixed pass's closures first: aux, decode
    for i in (0, 1):
        assert float(g_a[i].abs().max()) > 0 and torch.equal(g_a[i], g_b[i]), i
