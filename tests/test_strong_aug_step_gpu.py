"""pfst_amd.strong_aug.apply_strong_aug and its call site in the train step (uda.py, PFGST.forward_train) against the float64 reference of
tests/strong_aug_oracle.py with the parameters RE-DRAWN on the host from snapshots of the generator states: the entry point must consume
torch's CPU generator (four uniform_ and one randperm(4) per image) and NumPy's (one uniform(0.15, 1.15) per image) exactly as
rsiseg/models/uda/pfgst.py:212-222,287-294 and dacs_transforms.py:93 do, and nothing when a draw stays below its threshold.

Bounds: those of tests/test_strong_aug_edges_gpu.py -- the jitter bound (its largest value per channel: the blur mixes neighbours with
unit-sum weights, so it passes unchanged) plus the blur bound 2^-24 A (nx + ny + 2) on the jittered image.  Images are uint8-derived and
in gamut, normalised with the metas' mean and std.

The steps (b = 2, 128 x 128, six classes, dropout 0, pseudo threshold 0.3, blur on, colour_jitter_probability 0 so the jitter fires) wrap the
module attribute `apply_strong_aug` (forward_train imports it per call): the wrapper clones the class-mixed image it receives and snapshots
both generator states.  After the step debug['mixed_img'] -- what the student's mixed pass read -- must be the reference's image, the clone
must be the plain paste mask * img + (1 - mask) * target_img_strong_aug (target_img for DACS), and Python's `random` stream must have
advanced by exactly the step's two draws.  A further step with neither draw firing must hand the paste to the student bit for bit without
calling the entry point.

Worst ratio to the bound measured on the MI355X:
  entry point   scalar jitter_s 0.16 (64 x 64) and 0.19 (100 x 90), dict-valued 0.038 and 0.051 (its gain max(1, c) max(1, f) is larger),
                jitter only 0.22, blur only 0.25
  train step    PFGST 0.094, DACS 0.094; Python's generator advanced by exactly the two draws in every step"""
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

import strong_aug_oracle as SO
from helpers import note, report, seeded_pfgst_state, to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DICT_S = dict(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.5)


def metas(n):
    return [dict(img_norm_cfg=dict(mean=list(SO.MEAN), std=list(SO.STD))) for _ in range(n)]


def states():
    return torch.get_rng_state(), np.random.get_state()


def same_states(before):
    ts, ns = states()
    return torch.equal(ts, before[0]) and all(np.array_equal(a, b) for a, b in zip(ns, before[1]))


def same_numpy(before):
    return all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), before[1]))


# ------------------------------------------------------------------------------------------------------------------------------ the entry point
@pytest.mark.parametrize('shape', [(64, 64), (100, 90)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('jitter_s', [0.2, DICT_S], ids=['scalar', 'dict'])
def test_entry_point_draws_and_result(jitter_s, shape):
    from pfst_amd.strong_aug import apply_strong_aug
    img = SO.jitter_input(3, *shape, True, seed=3)
    torch.manual_seed(11), np.random.seed(11)
    before = states()
    x = img.to(DEV)
    y = apply_strong_aug(x, metas(3), 0.9, 0.2, jitter_s, 0.9)
    assert y.shape == x.shape and y.data_ptr() != x.data_ptr() and not same_states(before)
    want, bound = SO.strong_aug(img, metas(3), jitter_s, *before)
    ratio = float(((y.cpu().double() - want).abs() / bound).max())
    note('entry point', f'{"dict" if isinstance(jitter_s, dict) else "scalar"} {shape[0]}x{shape[1]}', ratio)
    report('entry point')
    assert bool(torch.isfinite(y).all()) and ratio < 1.0
    # the generators stand where the reference's draws leave them: the next draws agree with a replay that draws the same
    after = states()
    assert torch.equal(SO.draw_params(3, jitter_s, before[0], end_state=True)[1], after[0])
    assert all(np.array_equal(a, b) for a, b in zip(SO.draw_sigmas(3, before[1], end_state=True)[2], after[1]))


def test_entry_point_below_both_thresholds_draws_nothing():
    from pfst_amd.strong_aug import apply_strong_aug
    x = SO.jitter_input(2, 64, 64, True, seed=4).to(DEV)
    keep = x.clone()
    torch.manual_seed(12), np.random.seed(12)
    before = states()
    assert apply_strong_aug(x, metas(2), 0.1, 0.2, 0.2, 0.5) is x             # the blur needs draw > 0.5, the jitter draw > p
    assert apply_strong_aug(x, metas(2), 0.2, 0.2, DICT_S, 0.3) is x
    assert torch.equal(x, keep) and same_states(before)
    ten = torch.randn(2, 10, 32, 32, device=DEV)
    keep10 = ten.clone()
    assert apply_strong_aug(ten, metas(2), 0.9, 0.2, 0.2, 0.9) is ten         # not 3 channels: returned, nothing drawn
    assert torch.equal(ten, keep10) and same_states(before)


def test_each_transform_consumes_only_its_own_stream():
    from pfst_amd.strong_aug import apply_strong_aug
    img = SO.jitter_input(2, 64, 64, True, seed=5)
    torch.manual_seed(13), np.random.seed(13)
    before = states()
    x = img.to(DEV)
    y = apply_strong_aug(x, metas(2), 0.9, 0.2, 0.2, 0.3)                      # jitter only: in place, torch's stream
    assert y is x and same_numpy(before) and not torch.equal(torch.get_rng_state(), before[0])
    want, bound = SO.strong_aug(img, metas(2), 0.2, before[0], None)
    r_j = float(((y.cpu().double() - want).abs() / bound).max())
    mid = states()
    x = img.to(DEV)
    z = apply_strong_aug(x, metas(2), 0.1, 0.2, 0.2, 0.9)                      # blur only: a new tensor, NumPy's stream
    assert z is not x and torch.equal(x.cpu(), img) and torch.equal(torch.get_rng_state(), mid[0]) and not same_numpy(mid)
    want, bound = SO.strong_aug(img, metas(2), 0.2, None, mid[1])
    r_b = float(((z.cpu().double() - want).abs() / bound).max())
    note('entry point', 'jitter only', r_j), note('entry point', 'blur only', r_b)
    report('entry point')
    assert r_j < 1.0 and r_b < 1.0


# ------------------------------------------------------------------------------------------------------------------------------ the train step
def py_seed(fires):
    """the first seed of Python's generator whose second uniform(0, 1) is above 0.5 (fires) or not -> (seed, the state after the two draws)"""
    for seed in range(64):
        random.seed(seed)
        random.uniform(0, 1)
        if (random.uniform(0, 1) > 0.5) == fires:
            return seed, random.getstate()
    raise AssertionError


@pytest.fixture(scope='module')
def setup():
    from oracle import pfst_oracle as O
    from pfst_amd.synthetic import NORM_CFG, synth_batch
    assert tuple(NORM_CFG['mean']) == SO.MEAN and tuple(NORM_CFG['std']) == SO.STD
    state, _, _ = seeded_pfgst_state(O, 9)
    batch = synth_batch(2, 128, 6, seed=1234)
    for i, k in enumerate(('img', 'target_img', 'target_img_strong_aug')):
        batch[k] = SO.jitter_input(2, 128, 128, True, seed=20 + i)
    return state, batch


def run_step(kind, state, batch, monkeypatch, fires):
    import pfst_amd  # noqa: F401
    import pfst_amd.strong_aug as sa
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import UDA
    cfg = uda_cfg(threshold=0.3, blur=True, jitter_p=0.0 if fires else 2.0, dropout=0.0)
    cfg['type'] = kind
    if kind == 'DACS':
        cfg.pop('aux_losses')
    model = UDA.build(cfg)
    model.load_state_dict(OrderedDict((k, v.clone()) for k, v in state.items()), strict=False)
    model.cuda()
    dbg = model.debug = {}
    calls, real = [], sa.apply_strong_aug

    def wrapper(mixed_img, *args, **kw):
        calls.append((mixed_img.clone(),) + states())
        return real(mixed_img, *args, **kw)

    monkeypatch.setattr(sa, 'apply_strong_aug', wrapper)
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    seed, py_after = py_seed(fires)
    np.random.seed(0), torch.manual_seed(0), torch.cuda.manual_seed_all(0)
    random.seed(seed)
    out = model.train_step(to_dev(batch, DEV), opt)
    torch.cuda.synchronize()
    assert random.getstate() == py_after, 'the step drew from Python\'s generator other than its two strong-augmentation draws'
    assert all(np.isfinite(v) for v in out['log_vars'].values()), out['log_vars']
    b = to_dev(batch, DEV)
    paste = torch.where(dbg['mix_masks'].bool(), b['img'], b['target_img' if kind == 'DACS' else 'target_img_strong_aug'])
    frac = float(dbg['mix_masks'].float().mean())
    assert 0.05 < frac < 0.95, 'both operands of the paste are present'
    return dbg, calls, paste


@pytest.mark.parametrize('kind', ['PFGST', 'DACS'])
def test_step_feeds_the_student_the_augmented_mix(setup, monkeypatch, kind):
    state, batch = setup
    dbg, calls, paste = run_step(kind, state, batch, monkeypatch, fires=True)
    assert len(calls) == 1
    given, ts, ns = calls[0]
    assert torch.equal(given, paste), 'the entry point received the plain paste'
    got = dbg['mixed_img']
    assert got.shape == given.shape and not torch.equal(got, given)
    want, bound = SO.strong_aug(given.cpu(), batch['img_metas'], 0.2, ts, ns)
    ratio = float(((got.cpu().double() - want).abs() / bound).max())
    moved = float((want - given.cpu().double()).abs().max())
    note('train step', kind, ratio)
    print(f'{kind}: {ratio:.3g} of the bound; the augmentation moved the image by up to {moved:.3g}')
    report('train step')
    assert ratio < 1.0 and moved > 0.1


def test_step_without_a_firing_draw_hands_over_the_paste(setup, monkeypatch):
    state, batch = setup
    dbg, calls, paste = run_step('PFGST', state, batch, monkeypatch, fires=False)
    assert calls == []
    assert torch.equal(dbg['mixed_img'].view(torch.int32), paste.view(torch.int32))
