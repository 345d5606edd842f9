"""The self-training baselines inside whole train steps (b = 2, 128 x 128, six classes, dropout 0, the seeded state of the other step tests):
DACS against the PFGST step it is built on, and PFGST with an EntropyLoss among its auxiliary losses.

All steps run in deterministic mode from identical weights, seeds and an injected class choice, so two steps that launch the same kernels on
the same values agree bit for bit.  Bounds: a logged EntropyLoss value within 1e-5 relative of the fp64 oracle (tests/entropy_oracle.py)
evaluated on the step's captured mixed-pass logits; gradient arenas, taken as one tensor, per element within the per-link bound
1e-4 max|ref| + 1e-3 |ref|.

The weight W = 16 is chosen for the linearity test, whose subject is a DIFFERENCE of arenas.  Two steps that differ only in the order of two
fp32 additions into the logit gradient (the order test below) give arenas 1.3e-5 apart, 3.4e-6 of the arena's largest element: that is the
rounding of one backward sweep through some fifty layers, and every minuend carries it.  A difference of arenas is therefore known to about
1e-5 x max|arena| absolute, and the bound 1e-4 x max|difference| resolves it only where the term's share of the gradient is a tenth of the
arena's largest element or more.  At W = 1 the term moves the arena by 0.06 (W) and 0.12 (2W) of a maximum of 3.86 -- 3 % -- and the
comparison measured 3.4e-5 against a bound of 1.2e-5: rounding of the minuends, not a non-linearity.  At W = 16 the shares are 1 and 2 of 3.86.

The step's single blocking host read is not asserted here: tests/helpers.py has no reusable assertion for it; tests/test_entropy_cpu.py reads
the EntropyLoss path for host reads instead."""
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from entropy_oracle import entropy_loss, per_link_excess
from helpers import seeded_pfgst_state, to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
W = 16.0
PFGST_LOSS = uda_cfg()['aux_losses'][0]
ENT = lambda w: dict(type='EntropyLoss', loss_type='entropy', weights={'loss_ent': w})
MSQ = dict(type='EntropyLoss', loss_type='max_square', weights={'loss_max_square': W})
AUX_KEYS = ['loss_src_pos_mean', 'loss_src_neg_mean', 'loss_src_pos_std', 'loss_src_neg_std', 'loss_sim_pos', 'loss_sim_neg']
STEP_KEYS = ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'mix.decode.loss_ce', 'mix.decode.acc_seg', 'mix.aux.loss_ce',
             'mix.aux.acc_seg']


def step(kind, aux, batch, state, classes, through_train_step=False):
    """a fresh wrapper from the seeded state, one step with colour jitter and blur drawn (seeds reset) -> (out, gradient arena, debug dict)"""
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import UDA
    cfg = uda_cfg(blur=True, jitter_p=0.2)
    cfg['type'] = kind
    cfg['aux_losses'] = aux
    if kind == 'DACS':
        cfg.pop('aux_losses')
        cfg['debug_img_interval'] = 1000
    model = UDA.build(cfg)
    model.load_state_dict(OrderedDict((k, v.clone()) for k, v in state.items()), strict=False)
    model.cuda()
    model.injected_mix_classes = classes
    dbg = model.debug = {}
    random.seed(0); np.random.seed(0); torch.manual_seed(0); torch.cuda.manual_seed_all(0)
    if through_train_step:
        opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
        out = model.train_step(to_dev(batch, DEV), opt)
    else:
        out = model(**to_dev(batch, DEV))[0]            # forward_train's log_vars, `loss` included (train_step pops it)
    torch.cuda.synchronize()
    assert model.local_iter == 1
    return out, model.student_arena.grad.clone(), dbg


@pytest.fixture(scope='module')
def runs():
    from oracle import pfst_oracle as O
    from pfst_amd import hip_ops
    from pfst_amd.synthetic import synth_batch
    state, _, _ = seeded_pfgst_state(O, 9)
    batch = synth_batch(2, 128, 6, seed=1234)
    gt = batch['gt_semantic_seg']
    classes = np.array([[int(gt[i, 0, 100, 20]), int(gt[i, 0, 20, 100])] for i in range(2)], dtype=np.int32)
    assert classes.min() >= 0 and classes.max() < 6
    same_trg = dict(batch, target_img_strong_aug=batch['target_img'])
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        r = dict(
            dacs=step('DACS', None, batch, state, classes, through_train_step=True),          # the batch WITH its strong-aug entry: ignored
            pfgst_plain=step('PFGST', None, same_trg, state, classes, through_train_step=True),
            none=step('PFGST', [PFGST_LOSS], batch, state, classes),
            pe=step('PFGST', [PFGST_LOSS, ENT(W)], batch, state, classes),
            ep=step('PFGST', [ENT(W), PFGST_LOSS], batch, state, classes),
            pe2=step('PFGST', [PFGST_LOSS, ENT(2 * W)], batch, state, classes),
            msq=step('PFGST', [PFGST_LOSS, MSQ], batch, state, classes))
    finally:
        hip_ops.set_deterministic(was)
    r['batch'] = batch
    return r


def test_dacs_step_is_the_pfgst_step_without_auxiliary_losses(runs):
    (out_d, arena_d, dbg_d), (out_p, arena_p, dbg_p) = runs['dacs'], runs['pfgst_plain']
    assert sorted(out_d) == ['log_vars', 'num_samples'] and out_d['num_samples'] == 2           # dacs.py:147-149: no `states`
    assert sorted(out_p) == ['log_vars', 'num_samples', 'states']
    assert sorted(out_d['log_vars']) == sorted(STEP_KEYS)         # PFGST's keys without the auxiliary ones (and without `loss`)
    assert all(np.isfinite(v) for v in out_d['log_vars'].values())
    assert out_d['log_vars'] == out_p['log_vars']
    assert float(arena_d.abs().max()) > 0 and torch.equal(arena_d, arena_p)
    # the mix was pasted onto target_img (not its strongly augmented copy), then jittered and blurred: the two mixed images are the same
    assert torch.equal(dbg_d['mixed_img'], dbg_p['mixed_img'])
    own = runs['none'][2]['mixed_img']                       # PFGST on the unchanged batch pastes onto the strongly augmented copy
    assert not torch.equal(dbg_d['mixed_img'], own)
    # ... and neither is the plain paste: the colour jitter and the blur did run behind it
    b = to_dev(runs['batch'], DEV)
    m = dbg_d['mix_masks'].bool()
    pasted = torch.where(m, b['img'], b['target_img'])
    assert not torch.allclose(dbg_d['mixed_img'], pasted, atol=1e-3)


def test_entropy_term_is_logged_counted_and_order_independent(runs):
    (log_a, arena_a, dbg_a), (log_b, arena_b, _) = runs['pe'], runs['ep']
    step_keys = [k for k in runs['none'][0] if k not in AUX_KEYS + ['loss']]
    assert sorted(step_keys) == sorted(STEP_KEYS)
    assert list(log_a) == step_keys + AUX_KEYS + ['loss_ent', 'loss'] and list(log_b) == step_keys + ['loss_ent'] + AUX_KEYS + ['loss']
    want, _ = entropy_loss(dbg_a['mix_logits'].cpu().numpy(), 'entropy', W)
    rel = abs(log_a['loss_ent'] - want) / abs(want)
    print(f'loss_ent {log_a["loss_ent"]:.8g}, fp64 oracle on the captured logits {want:.8g}: rel {rel:.2e} (bound 1e-5)')
    assert rel <= 1e-5 and log_a['loss_ent'] > 0
    total = sum(v for k, v in log_a.items() if 'loss' in k and k != 'loss')
    assert abs(log_a['loss'] - total) <= 1e-12 * abs(total)
    none = runs['none'][0]
    assert abs((log_a['loss'] - none['loss']) - log_a['loss_ent']) <= 1e-9 * abs(log_a['loss'])       # every other term is unchanged ...
    assert {k: v for k, v in log_a.items() if k not in ('loss', 'loss_ent')} == {k: v for k, v in none.items() if k != 'loss'}
    # both orders: the same forward values (the python sum of `loss` runs in another order)
    assert {k: v for k, v in log_a.items() if k != 'loss'} == {k: v for k, v in log_b.items() if k != 'loss'}
    assert abs(log_a['loss'] - log_b['loss']) <= 1e-12 * abs(log_a['loss'])
    ex = per_link_excess(arena_b.cpu().numpy(), arena_a.cpu().numpy())
    print(f'arena [EntropyLoss, PFGSTLoss] vs [PFGSTLoss, EntropyLoss]: max |diff| {float((arena_a - arena_b).abs().max()):.2e} of max '
          f'{float(arena_a.abs().max()):.2e}, excess over the per-link bound {ex:.2e}')
    assert ex <= 0


def test_entropy_gradient_reaches_the_parameters_linearly_in_its_weight(runs):
    a0, a1, a2 = (runs[k][1].double().cpu().numpy() for k in ('none', 'pe', 'pe2'))
    assert not np.array_equal(a1, a0)
    d1, d2 = a1 - a0, a2 - a0
    ex = per_link_excess(2 * d1, d2)
    print(f'arena(2W) - arena(0): max {np.abs(d2).max():.3e} beside max |arena(0)| {np.abs(a0).max():.3e}; against 2 (arena(W) - arena(0)): '
          f'max |diff| {np.abs(2 * d1 - d2).max():.2e}, excess over the per-link bound {ex:.2e}')
    assert np.abs(d2).max() > 0.1 * np.abs(a0).max(), 'the term\'s share is large enough for the bound to resolve the difference (module docstring)'
    assert ex <= 0
    assert runs['pe2'][0]['loss_ent'] == pytest.approx(2 * runs['pe'][0]['loss_ent'], rel=1e-6)


def test_max_square_step(runs):
    log, arena, dbg = runs['msq']
    assert list(log)[-2:] == ['loss_max_square', 'loss'] and len(log) == len(STEP_KEYS) + len(AUX_KEYS) + 2
    want, _ = entropy_loss(dbg['mix_logits'].cpu().numpy(), 'max_square', W)
    rel = abs(log['loss_max_square'] - want) / abs(want)
    print(f'loss_max_square {log["loss_max_square"]:.8g}, fp64 oracle {want:.8g}: rel {rel:.2e} (bound 1e-5)')
    assert rel <= 1e-5 and log['loss_max_square'] < 0
    assert bool(torch.isfinite(arena).all()) and not torch.equal(arena, runs['none'][1])
