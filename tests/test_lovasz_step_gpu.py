"""LovaszLoss inside the train steps: the supervised step at b = 2, 64 x 64 (six classes, dropout 0) with [CrossEntropyLoss, LovaszLoss] on the
decode head (logits at 1/4: the x4 block route) and [CrossEntropyLoss] on the auxiliary head, and one PFGST step with the term listed in both
heads.  The network's other reductions run in deterministic mode, as in tests/test_dice_step_gpu.py; the Lovasz term is bit-identical in
either mode (tests/test_lovasz_loss_gpu.py)."""
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
LV = lambda w: dict(type='LovaszLoss', loss_weight=w, reduction='none')
HEADS = {'ce': (CE(1.0), CE(0.4)), 'both': ([CE(1.0), LV(1.0)], CE(0.4))}


def sup_step(heads, batch):
    """a fresh segmentor from the seeded state, one train_step -> (log_vars, the gradient arena)"""
    import pfst_amd  # noqa: F401
    from oracle import pfst_oracle as O
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import fill_state_dict
    cfg = model_cfg(dropout=0.0)
    cfg['decode_head']['loss_decode'], cfg['auxiliary_head']['loss_decode'] = heads
    model = build_segmentor(cfg)
    res = model.load_state_dict(fill_state_dict(O.init_state_dict(6, 3), 9), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    out = model.train_step(to_dev(batch, DEV), build_optimizer(model, dict(SGD)))
    torch.cuda.synchronize()
    assert out['loss'] == out['log_vars']['loss']
    return out['log_vars'], model.param_arena.grad.clone()


@pytest.fixture(scope='module')
def runs():
    from pfst_amd import hip_ops
    from pfst_amd.synthetic import synth_batch
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        batch = {k: v for k, v in synth_batch(2, 64, 6, seed=1234).items() if not k.startswith('target_')}
        return {name: sup_step(HEADS[name.split('_')[0]], batch) for name in ('ce', 'both', 'both_again')}
    finally:
        hip_ops.set_deterministic(was)


def test_supervised_step_logs_the_term_beside_ce(runs):
    log, ce = runs['both'][0], runs['ce'][0]
    assert list(log) == ['decode.loss_ce', 'decode.loss_lovasz', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss']
    assert all(np.isfinite(v) for v in log.values()), log
    assert 0.0 < log['decode.loss_lovasz'] <= 1.0               # a mean of Lovasz extensions of the Jaccard loss: in (0, 1]
    total = sum(log[k] for k in log if 'loss' in k and k != 'loss')
    assert abs(log['loss'] - total) <= 1e-6 * total
    # the CE values and acc_seg are what the [CE]-only step reports for the same forward pass, bit for bit
    for k in ('decode.loss_ce', 'aux.loss_ce', 'decode.acc_seg', 'aux.acc_seg'):
        assert log[k] == ce[k], k


def test_supervised_step_gradients_carry_the_term_and_repeat_bit_for_bit(runs):
    both, ce = runs['both'][1], runs['ce'][1]
    diff = float((both.double() - ce.double()).norm() / ce.double().norm())
    print(f'|arena([CE, Lovasz]) - arena([CE])| / |arena([CE])| = {diff:.3e}')
    assert bool(torch.isfinite(both).all()) and diff > 1e-3
    assert torch.equal(both, runs['both_again'][1]) and runs['both'][0] == runs['both_again'][0]


def pfgst_step(threshold, batch, both):
    import pfst_amd  # noqa: F401
    from oracle import pfst_oracle as O  # noqa: F401
    from pfst_amd import models
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import UDA
    cfg = uda_cfg(threshold=threshold)
    cfg['model']['decode_head']['loss_decode'], cfg['model']['auxiliary_head']['loss_decode'] = [CE(1.0), LV(1.0)], [CE(0.4), LV(0.4)]
    model = UDA.build(cfg)
    model.load_state_dict(both, strict=False)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    grads, real = [], models.ops.lovasz_upsample_bwd

    def recording(ld, l8, slot, cls, lse, cmap, blk, scale, ign, out=None, accumulate=False):
        grads.append(real(ld, l8, slot, cls, lse, cmap, blk, scale, ign).clone())        # the term alone, into a buffer of its own
        return real(ld, l8, slot, cls, lse, cmap, blk, scale, ign, out=out, accumulate=accumulate)
    models.ops.lovasz_upsample_bwd = recording
    try:
        random.seed(0); np.random.seed(0); torch.manual_seed(0)
        log = model.train_step(to_dev(batch, DEV), opt)['log_vars']
        torch.cuda.synchronize()
    finally:
        models.ops.lovasz_upsample_bwd = real
    return log, grads


def test_pfgst_step_with_the_term_listed_ignores_the_pseudo_weights():
    from oracle import pfst_oracle as O
    from pfst_amd import hip_ops
    from pfst_amd.synthetic import synth_batch
    both, _, _ = seeded_pfgst_state(O, 9)
    batch = synth_batch(2, 128, 6, seed=1234)
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        # thre_type='all': the threshold sets the scalar pseudo-weight q of the target pixels and nothing else (labels are the arg-max):
        # every weight replaced by one (q = 1) against every weight zero (q = 0)
        log_a, g_a = pfgst_step(0.0, batch, OrderedDict((k, v.clone()) for k, v in both.items()))
        log_b, g_b = pfgst_step(1.01, batch, OrderedDict((k, v.clone()) for k, v in both.items()))
    finally:
        hip_ops.set_deterministic(was)
    for k in ('decode.loss_lovasz', 'aux.loss_lovasz', 'mix.decode.loss_lovasz', 'mix.aux.loss_lovasz', 'mix.decode.loss_ce'):
        assert k in log_a and np.isfinite(log_a[k]), k
    print('mixed-pass CE under the two thresholds:', log_a['mix.decode.loss_ce'], log_b['mix.decode.loss_ce'])
    assert log_a['mix.decode.loss_ce'] != log_b['mix.decode.loss_ce'], 'the pseudo-weights did change'
    assert log_a['mix.decode.loss_lovasz'] == log_b['mix.decode.loss_lovasz'] and log_a['mix.aux.loss_lovasz'] == log_b['mix.aux.loss_lovasz']
    assert len(g_a) == len(g_b) == 4                       # the backward sweep runs the mixed pass's closures first: aux, decode
    for i in (0, 1):
        assert float(g_a[i].abs().max()) > 0 and torch.equal(g_a[i], g_b[i]), i
