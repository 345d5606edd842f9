"""LovaszLoss without a GPU: the registry and constructor, and tests/lovasz_oracle.py -- the fp64 restatement the GPU tests compare with --
against the executed reference (tests/golden/lovasz_loss.npz, written by tests/golden/make_golden_lovasz.py).

Bounds, fp32 reference against the fp64 oracle: the loss within 1e-6 relative (about 1e4 terms of fp32 rounding 6e-8 each, added in fp32 by
torch.dot: measured 7e-9 .. 5e-8), the gradient within the per-link bound of tests/test_dice_loss_gpu.py, |ref - oracle| <= 1e-4 max|oracle| +
1e-3 |oracle| per element (measured worst ratio 0.17, case x4), outside the oracle's mask of undetermined cells -- which is empty at the
fixture's seeds and must cover at most 5 % of the cells."""
import os

import numpy as np
import pytest
import torch

import lovasz_oracle as O

CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
# name: (inputs, LovaszLoss / oracle options)      -- the options of tests/golden/make_golden_lovasz.py's CASES
CASES = {
    'x4': ('x4', dict()),
    'x4_all': ('x4', dict(classes='all', class_weight=CW6)),
    'x4_img': ('x4', dict(per_image=True, reduction='mean')),
    'x4_img_sum': ('x4', dict(per_image=True, reduction='sum')),
    'x8': ('x8', dict(classes=[1, 4])),
    'g11': ('g11', dict()),
}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'lovasz_loss.npz'))


def test_the_registry_builds_the_term_from_a_dict_and_inside_a_list():
    import pfst_amd  # noqa: F401
    from pfst_amd.models import LovaszLoss
    from pfst_amd.registry import build_loss
    term = build_loss(dict(type='LovaszLoss', reduction='none', loss_weight=2.0, classes=[1, 4]))
    assert isinstance(term, LovaszLoss) and term.loss_name == 'loss_lovasz' and term.loss_weight == 2.0 and term.classes == [1, 4]
    assert not term.per_image and term.class_weight is None
    both = [build_loss(c) for c in (dict(type='CrossEntropyLoss'), dict(type='LovaszLoss', per_image=True, loss_name='loss_lv'))]
    assert isinstance(both[1], LovaszLoss) and both[1].per_image and both[1].reduction == 'mean' and both[1].loss_name == 'loss_lv'
    assert hasattr(term, 'fused')


def test_the_constructor_refuses_what_is_not_built_or_not_valid():
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_loss
    with pytest.raises(NotImplementedError, match='binary'):
        build_loss(dict(type='LovaszLoss', loss_type='binary', reduction='none'))
    with pytest.raises(ValueError, match='loss_type'):
        build_loss(dict(type='LovaszLoss', loss_type='hinge', reduction='none'))
    with pytest.raises(ValueError, match="reduction should be 'none' when per_image is False"):
        build_loss(dict(type='LovaszLoss', per_image=False, reduction='mean'))
    with pytest.raises(ValueError, match="reduction should be 'none'") as err:
        build_loss(dict(type='LovaszLoss'))                # the reference's defaults contradict each other in the same way (its assert)
    # ... and a config that names the term and nothing else fails with a KeyError too, as it did while the registry lacked the type
    assert isinstance(err.value, KeyError) and str(err.value) == "LovaszLoss: reduction should be 'none' when per_image is False"
    for bad in ('some', [], [1.5], [True], 3):
        with pytest.raises(ValueError, match='classes'):
            build_loss(dict(type='LovaszLoss', reduction='none', classes=bad))
    with pytest.raises(ValueError, match='reduction'):
        build_loss(dict(type='LovaszLoss', per_image=True, reduction='avg'))


def test_class_tables_and_class_weight_are_checked_at_first_use():
    import pfst_amd  # noqa: F401
    from pfst_amd import hip_ops
    from pfst_amd.registry import build_loss
    slot, cls = hip_ops.lovasz_class_tables([4, 1], 6, 'cpu')
    assert slot.tolist() == [-1, 1, -1, -1, 0, -1] and cls.tolist() == [4, 1]
    slot, cls = hip_ops.lovasz_class_tables('present', 3, 'cpu')
    assert slot.tolist() == [0, 1, 2] and cls.tolist() == [0, 1, 2]
    for bad in ([6], [-1], [1, 1]):
        with pytest.raises(ValueError, match='distinct class indices'):
            hip_ops.lovasz_class_tables(bad, 6, 'cpu')
    term = build_loss(dict(type='LovaszLoss', reduction='none', class_weight=[1.0, 2.0, 3.0]))
    with pytest.raises(ValueError, match='class_weight has 3 entries for 6 classes'):
        term._class_tables(6, torch.device('cpu'))


def test_a_sampled_head_refuses_a_lovasz_term():
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head
    cfg = dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36), c1_in_channels=8,
               c1_channels=4, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
               sampler=dict(type='OHEMPixelSampler', thresh=0.7, min_kept=1000))
    with pytest.raises(NotImplementedError, match='LovaszLoss'):
        build_head(dict(cfg, loss_decode=[dict(type='CrossEntropyLoss'), dict(type='LovaszLoss', reduction='none')]))
    build_head(dict(cfg, loss_decode=dict(type='CrossEntropyLoss')))


@pytest.mark.parametrize('name', list(CASES))
def test_the_oracle_reproduces_the_executed_reference(golden, name):
    src, opts = CASES[name]
    logits, label = torch.from_numpy(golden[src + '|logits']), torch.from_numpy(golden[src + '|label'])
    r = O.lovasz_oracle(logits, label, tuple(label.shape[-2:]), **opts)
    want = float(golden[name + '|loss'])
    e_loss = abs(r['loss'] - want) / abs(r['loss'])
    frac = float(r['mask'].float().mean())
    ratio = O.link_ratio(torch.from_numpy(golden[name + '|grad']), r['grad'], ~r['mask'].unsqueeze(1))
    print(f'{name}: loss oracle {r["loss"]!r} reference {want!r} rel err {e_loss:.2e} (bound 1e-6); masked cells {int(r["mask"].sum())} of '
          f'{r["mask"].numel()}; reference fp32 gradient vs the oracle: worst ratio to the per-link bound {ratio:.2e}')
    assert e_loss <= 1e-6
    assert frac <= O.MASK_CAP
    assert ratio <= 1.0
    assert r['bad'] == (16 if name == 'x8' else 0)


def test_the_closed_form_of_the_uniform_case(golden):
    label = torch.from_numpy(golden['x4|label'])
    logits = torch.zeros(2, 6, 19, 17)
    r = O.lovasz_oracle(logits, label, (76, 68))
    assert abs(r['loss'] - O.closed_form_uniform(label, 6)) <= 1e-12 and O.closed_form_uniform(label, 6) == 1.0 - 1.0 / 6
    assert O.closed_form_uniform(torch.full_like(label, 255), 6) == 0.0


def test_the_head_case_of_the_fixture_ignores_the_pixel_weights(golden):
    assert list(golden['head|names']) == ['loss_ce', 'loss_lovasz', 'acc_seg']
    a, b = golden['head|values'], golden['head_half|values']
    assert a[1] == b[1] and a[0] != b[0] and a[2] == b[2]
    # loss_weight 2: twice the standalone x4 value (fp32: one rounding of the product)
    assert abs(a[1] - 2.0 * float(golden['x4|loss'])) <= 1e-6 * a[1]
