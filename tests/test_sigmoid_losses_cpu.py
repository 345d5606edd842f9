"""FocalLoss and CrossEntropyLoss(use_sigmoid=True), the parts that need no GPU: the fp64 closed-form oracle of the GPU tests
(tests/sigmoid_loss_oracle.py) against fp64 autograd of the reference's literal formulas and against the numbers the reference itself returned
(tests/golden/sigmoid_losses.npz, written by tests/golden/make_golden_focal.py), the reference's defaults, every refused option, configs and
--cfg-options, the C ABI of the three entry points, and the OHEMPixelSampler rule for sigmoid terms.

Measured here (the reference's fp32 against the fp64 oracle): loss <= 1.2e-7 relative, gradients <= 1.7e-3 of the per-link bound."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import pfst_amd  # noqa: F401
import sigmoid_loss_oracle as O
from helpers import model_cfg
from pfst_amd.registry import build_head, build_loss, build_segmentor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'sigmoid_losses.npz')
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
BCE = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)
FOCAL = dict(type='FocalLoss', loss_weight=2.0)
CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
ALPHA6 = [0.25, 0.5, 0.75, 0.1, 0.9, 0.4]
SIZES = {'x4': (76, 68), 'x8': (136, 144), 'g11': (30, 37), 'g2': (30, 37)}
# what make_golden_focal.py ran: name -> (inputs, oracle arguments, pixel weights?)
FIXTURE_CASES = {
    'x4_focal': ('x4', dict(coef=O.focal_coef(6), gamma=2.0), True),
    'x4_bce': ('x4', dict(coef=O.bce_coef(6), gamma=0.0), True),
    'x8_focal': ('x8', dict(coef=O.focal_coef(6, ALPHA6, CW6), gamma=3.0), True),
    'g11_focal': ('g11', dict(coef=O.focal_coef(11, 0.25), gamma=0.5, reduction='none'), True),
    'g2_focal': ('g2', dict(coef=O.focal_coef(2, [0.3, 0.6]), gamma=0.0, reduction='sum'), False),
    'g2_bce': ('g2', dict(coef=O.bce_coef(2), gamma=0.0, loss_weight=0.5), False),
}


def head_cfg(which, loss_decode, **over):
    cfg = dict(model_cfg()[which], loss_decode=loss_decode)
    cfg.update(over)
    return cfg


@pytest.fixture(scope='module')
def gold():
    return O.load_fixture(GOLD)


def fixture_inputs(gold, src, weighted):
    z, lab = torch.from_numpy(gold[src + '|logits']), torch.from_numpy(gold[src + '|label'])
    w = O.expand_blocks(torch.from_numpy(gold[src + '|weight_blocks']), SIZES[src]) if weighted else None
    return z, lab, w


def test_closed_form_equals_fp64_autograd_of_the_literal_formulas(gold):
    z, lab, w = fixture_inputs(gold, 'x4', True)
    z11, lab11, w11 = fixture_inputs(gold, 'g11', True)
    worst = 0.0
    for gamma in (0.0, 0.5, 2.0, 3.0):
        for alpha, cw, red in ((0.5, None, 'mean'), (ALPHA6, CW6, 'sum')):
            got = O.sigmoid_loss(z, lab, SIZES['x4'], O.focal_coef(6, alpha, cw), gamma, w, reduction=red, loss_weight=1.5)
            loss, dz = O.literal_loss(z, lab, SIZES['x4'], 'focal', gamma, alpha, cw, w, reduction=red, loss_weight=1.5)
            assert abs(got['loss'] - loss) <= 1e-12 * abs(loss), (gamma, alpha)
            err = np.abs(got['grad'] - dz).max() / np.abs(dz).max()
            worst = max(worst, err)
            assert err <= 1e-12, (gamma, alpha, err)
    for cw in (None, CW6):
        got = O.sigmoid_loss(z, lab, SIZES['x4'], O.bce_coef(6, cw), 0.0, w)
        loss, dz = O.literal_loss(z, lab, SIZES['x4'], 'bce', class_weight=cw, weight=w)
        assert abs(got['loss'] - loss) <= 1e-12 * abs(loss)
        assert np.abs(got['grad'] - dz).max() <= 1e-12 * np.abs(dz).max()
    got = O.sigmoid_loss(z11, lab11, SIZES['g11'], O.focal_coef(11, 0.25), 0.5, w11, reduction='none')
    loss, dz = O.literal_loss(z11, lab11, SIZES['g11'], 'focal', 0.5, 0.25, None, w11, reduction='none')
    assert abs(got['loss'] - loss) <= 1e-12 * abs(loss) and np.abs(got['grad'] - dz).max() <= 1e-12 * np.abs(dz).max()
    assert not got['grad'][1].any() and not got['sums'][1].any(), 'image 1 of g11 is entirely 255'
    print('worst relative gradient difference to fp64 autograd', worst)


def test_the_literal_formula_breaks_where_the_closed_form_does_not(gold):
    """gamma = 0.5 on saturated logits: pow(0, 0.5) has an infinite derivative that autograd multiplies by 0 -- NaN in fp32 (and in fp64 once
    sigmoid rounds to 1).  The closed form has no negative power and stays finite: what the kernels implement."""
    z, lab, w = fixture_inputs(gold, 'x4', True)
    _, dz = O.literal_loss(z * 40, lab, SIZES['x4'], 'focal', 0.5, 0.5, None, w, dtype=torch.float32)
    assert np.isnan(dz).any()
    for gamma in (0.5, 2.0):
        got = O.sigmoid_loss(z * 40, lab, SIZES['x4'], O.focal_coef(6), gamma, w)
        assert np.isfinite(got['grad']).all() and np.isfinite(got['sums']).all() and np.isfinite(got['loss'])


def test_oracle_against_the_executed_reference(gold):
    assert list(gold['cases']) == list(FIXTURE_CASES)
    worst_loss = worst_grad = 0.0
    for name, (src, kw, weighted) in FIXTURE_CASES.items():
        z, lab, w = fixture_inputs(gold, src, weighted)
        got = O.sigmoid_loss(z, lab, SIZES[src], weight=w, **kw)
        rel = abs(got['loss'] - float(gold[name + '|loss'])) / abs(got['loss'])
        ratio = O.worst_ratio(gold[name + '|grad'], got['grad'])
        print(f'{name}: loss rel {rel:.2e}, worst gradient ratio to the per-link bound {ratio:.2e}')
        worst_loss, worst_grad = max(worst_loss, rel), max(worst_grad, ratio)
        assert rel <= 1e-5, name
        assert ratio <= 1.0, name
    # the head: [CE(1.0), Focal(2.0, alpha 0.25, CW6)] without weights, and the two modules with weights
    z, lab, w = fixture_inputs(gold, 'x4', True)
    for key, weight in (('head', None), ('head_w', w)):
        focal = O.sigmoid_loss(z, lab, SIZES['x4'], O.focal_coef(6, 0.25, CW6), 2.0, weight, loss_weight=2.0)
        z64 = z.double().requires_grad_()
        per = torch.nn.functional.cross_entropy(O.upsample(z64, SIZES['x4']), lab.long(), ignore_index=255, reduction='none')
        ce = (per if weight is None else per * weight.double()).mean()
        (dce,) = torch.autograd.grad(ce, z64)
        vals = gold[key + '|values']
        assert abs(float(ce) - vals[0]) <= 1e-5 * abs(float(ce)) and abs(focal['loss'] - vals[1]) <= 1e-5 * abs(focal['loss']), key
        assert O.worst_ratio(gold[key + '|grad'], dce.numpy() + focal['grad']) <= 1.0, key
    assert list(gold['head|names']) == ['loss_ce', 'loss_focal', 'acc_seg']
    print('worst over the fixture: loss', worst_loss, 'gradient ratio', worst_grad)


def test_defaults_are_the_references():
    from pfst_amd.models import CrossEntropyLoss, FocalLoss
    f = build_loss(dict(type='FocalLoss'))
    assert isinstance(f, FocalLoss)
    assert (f.use_sigmoid, f.gamma, f.alpha, f.reduction, f.class_weight, f.loss_weight, f.loss_name) == (True, 2.0, 0.5, 'mean', None, 1.0, 'loss_focal')
    b = build_loss(dict(type='CrossEntropyLoss', use_sigmoid=True))
    assert isinstance(b, CrossEntropyLoss) and b.use_sigmoid and (b.class_weight, b.loss_weight, b.loss_name) == (None, 1.0, 'loss_ce')
    assert build_loss(CE).use_sigmoid is False
    assert hasattr(f, 'fused') and hasattr(b, 'fused')


def test_alpha_as_float_and_as_list():
    f = build_loss(dict(type='FocalLoss', alpha=0.25, class_weight=[1.0, 2.0, 4.0]))
    assert f.coef_rows(3) == [[0.25, 0.75], [0.5, 1.5], [1.0, 3.0]]
    f = build_loss(dict(type='FocalLoss', alpha=[0.0, 1.0, 0.5]))
    assert f.coef_rows(3) == [[0.0, 1.0], [1.0, 0.0], [0.5, 0.5]]
    assert f.coef_rows(3) == O.focal_coef(3, [0.0, 1.0, 0.5])
    b = build_loss(dict(type='CrossEntropyLoss', use_sigmoid=True, class_weight=[3.0, 0.5]))
    assert b.sigmoid_coef(2) == [[3.0, 1.0], [0.5, 1.0]] == O.bce_coef(2, [3.0, 0.5])
    assert build_loss(BCE).sigmoid_coef(4) == [[1.0, 1.0]] * 4


def test_refused_options_fail_loudly():
    with pytest.raises(NotImplementedError, match='sigmoid'):
        build_loss(dict(type='FocalLoss', use_sigmoid=False))
    for gamma in (-0.5, float('nan'), 'two', None):
        with pytest.raises(ValueError, match='gamma'):
            build_loss(dict(type='FocalLoss', gamma=gamma))
    for gamma in (0, 0.0, 0.5, 2, 3.0):
        assert build_loss(dict(type='FocalLoss', gamma=gamma)).gamma == gamma
    for alpha in (-0.1, 1.5, float('nan'), [0.5, 1.2], [], 'half'):
        with pytest.raises(ValueError, match='alpha'):
            build_loss(dict(type='FocalLoss', alpha=alpha))
    with pytest.raises(ValueError, match='reduction'):
        build_loss(dict(type='FocalLoss', reduction='batchmean'))
    for reduction in ('mean', 'sum', 'none'):
        assert build_loss(dict(type='FocalLoss', reduction=reduction)).reduction == reduction
    # list lengths are checked against C at the first call, the message names both numbers
    with pytest.raises(ValueError, match=r'alpha has 3 entries for 6 classes'):
        build_loss(dict(type='FocalLoss', alpha=[0.1, 0.2, 0.3])).coef_rows(6)
    with pytest.raises(ValueError, match=r'class_weight has 2 entries for 6 classes'):
        build_loss(dict(type='FocalLoss', class_weight=[1.0, 2.0])).coef_rows(6)
    with pytest.raises(ValueError, match=r'class_weight has 2 entries for 6 classes'):
        build_loss(dict(type='CrossEntropyLoss', use_sigmoid=True, class_weight=[1.0, 2.0])).sigmoid_coef(6)
    # what stays out
    for over in (dict(avg_non_ignore=True), dict(use_mask=True), dict(reduction='sum'), dict(use_sigmoid=True, avg_non_ignore=True),
                 dict(use_sigmoid=True, reduction='none')):
        with pytest.raises(NotImplementedError):
            build_loss(dict(type='CrossEntropyLoss', **over))
    with pytest.raises(NotImplementedError, match='num_classes >= 2'):
        build_loss(BCE).sigmoid_coef(1)
    with pytest.raises(NotImplementedError, match='num_classes >= 2'):
        build_loss(dict(type='FocalLoss')).coef_rows(1)
    with pytest.raises(KeyError):
        build_loss(dict(type='LovaszLoss'))


def test_configs_build_and_cfg_options_round_trip():
    import torch.nn as nn
    from pfst_amd.models import CrossEntropyLoss, FocalLoss
    head = build_head(head_cfg('auxiliary_head', [CE, FOCAL]))
    assert isinstance(head.loss_decode, nn.ModuleList) and [type(l) for l in head.loss_decode] == [CrossEntropyLoss, FocalLoss]
    assert [l.loss_name for l in head.loss_decode] == ['loss_ce', 'loss_focal'] and head.loss_decode[1].loss_weight == 2.0
    assert isinstance(build_head(head_cfg('decode_head', FOCAL)).loss_decode, FocalLoss)
    assert build_head(head_cfg('decode_head', BCE)).loss_decode.use_sigmoid
    cfg = model_cfg()
    cfg['decode_head']['loss_decode'] = [CE, FOCAL]
    cfg['auxiliary_head']['loss_decode'] = [dict(CE, loss_weight=0.4), dict(FOCAL, loss_weight=0.8, loss_name='loss_focal_aux')]
    model = build_segmentor(cfg)
    assert model.auxiliary_head.loss_decode[1].loss_name == 'loss_focal_aux'
    assert not [k for k in model.state_dict() if 'loss_decode' in k], 'a loss list adds no parameters or buffers'
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.registry import build_train_model
    name = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
    losses = "[{'type':'CrossEntropyLoss','loss_weight':1.0},{'type':'FocalLoss','loss_weight':2.0,'gamma':2.0,'alpha':[0.25,0.25,0.25,0.25,0.75,0.5]}]"
    cfg = train_cli.load_cfg(train_cli.parse_args([name, '--supervised', '--cfg-options', 'model.decode_head.loss_decode=' + losses,
                                                   "model.auxiliary_head.loss_decode={'type':'CrossEntropyLoss','use_sigmoid':True,'loss_weight':0.4}"]))
    got = cfg.model['decode_head']['loss_decode']
    assert [dict(l) for l in got] == [dict(type='CrossEntropyLoss', loss_weight=1.0),
                                      dict(type='FocalLoss', loss_weight=2.0, gamma=2.0, alpha=[0.25, 0.25, 0.25, 0.25, 0.75, 0.5])]
    model = build_train_model(cfg)
    assert [type(l).__name__ for l in model.decode_head.loss_decode] == ['CrossEntropyLoss', 'FocalLoss']
    assert model.decode_head.loss_decode[1].alpha == [0.25, 0.25, 0.25, 0.25, 0.75, 0.5] and model.auxiliary_head.loss_decode.use_sigmoid
    uda = build_train_model(train_cli.load_cfg(train_cli.parse_args([name, '--cfg-options', 'model.decode_head.loss_decode=' + losses])))
    assert [type(l).__name__ for l in uda.get_model().decode_head.loss_decode] == ['CrossEntropyLoss', 'FocalLoss']


def test_the_three_entry_points_are_declared_and_validate_on_the_host():
    """every refusal below returns -1 before any launch: no device is touched"""
    from pfst_amd import _lib, hip_ops
    decls = _lib.parse_header()
    want = {'pfst_sigloss_upsample_fwd': 17, 'pfst_sigloss_finalize': 10, 'pfst_sigloss_upsample_bwd': 17}
    text = open(_lib.HEADER).read()
    src = open(os.path.join(ROOT, 'pfst_amd', 'csrc', 'sigmoid_loss.hip')).read()
    for name, nargs in want.items():
        restype, args = decls[name]
        assert restype is ctypes.c_int and len(args) == nargs, (name, len(args))
        assert args[-1] == (ctypes.c_void_p, 'stream')
        norm = lambda s: ' '.join(re.search(name + r'\s*\(([^)]*)\)', s).group(1).split())
        assert norm(text) == norm(src[src.index('extern "C" int ' + name):]), name
        assert hasattr(_lib.lib(), name)
    kinds = dict((a, k) for k, a in decls['pfst_sigloss_finalize'][1])
    assert kinds['divisor'] is ctypes.c_double and kinds['loss_weight'] is ctypes.c_double and kinds['slab'] is ctypes.c_void_p
    kinds = dict((a, k) for k, a in decls['pfst_sigloss_upsample_fwd'][1])
    assert kinds['gamma'] is ctypes.c_float and kinds['form'] is ctypes.c_int and kinds['coef'] is ctypes.c_void_p
    from pfst_amd.build import NO_SLP, SOURCES
    assert 'sigmoid_loss.hip' in SOURCES and 'sigmoid_loss.hip' in NO_SLP and '#pragma clang fp contract(off)' in src
    assert 'atomicAdd' not in src, 'the kernels use no atomics'
    assert 'powf' not in src.replace('no powf', '')

    P = 1 << 12                                  # a non-null, 8-byte aligned stand-in for a pointer that is never dereferenced
    N, C, h, w, H, W = 2, 6, 19, 17, 76, 68
    blocks4 = ((w + 16) // 16) * ((h + 32) // 32)

    def fwd(logits=P, N=N, C=C, h=h, w=w, label=P, pw=P, H=H, W=W, ign=255, coef=P, gamma=2.0, form=4, slab=P, counts=P, blocks=blocks4):
        return _lib.lib().pfst_sigloss_upsample_fwd(logits, N, C, h, w, label, pw, H, W, ign, coef, gamma, form, slab, counts, blocks, None)

    def bwd(logits=P, N=N, C=C, h=h, w=w, label=P, pw=P, H=H, W=W, ign=255, coef=P, gamma=2.0, form=4, scale=1.0, dlogits=P, acc=0):
        return _lib.lib().pfst_sigloss_upsample_bwd(logits, N, C, h, w, label, pw, H, W, ign, coef, gamma, form, scale, dlogits, acc, None)

    def fin(slab=P, counts=P, N=N, C=C, blocks=4, divisor=1.0, lw=1.0, sums=P, out=P):
        return _lib.lib().pfst_sigloss_finalize(slab, counts, N, C, blocks, divisor, lw, sums, out, None)

    for f in (fwd, bwd):
        for bad in (dict(logits=None), dict(label=None), dict(coef=None), dict(C=0), dict(C=256), dict(N=0), dict(h=0), dict(gamma=-1.0),
                    dict(gamma=float('nan')), dict(form=3), dict(form=8), dict(form=4, C=9), dict(form=4, H=H + 1), dict(form=4, W=W - 4),
                    dict(form=4, pw=P + 4), dict(form=4, label=P + 1), dict(form=8, H=8 * h, W=4 * w)):
            assert f(**bad) == -1, (f.__name__, bad)
        assert 'sigmoid_loss.hip' in _lib.lib().pfst_last_error().decode()
    for bad in (dict(slab=None), dict(counts=None), dict(blocks=blocks4 + 1), dict(form=0, blocks=blocks4)):
        assert fwd(**bad) == -1, bad
    assert bwd(dlogits=None) == -1
    for bad in (dict(slab=None), dict(counts=None), dict(sums=None), dict(out=None), dict(C=0), dict(C=256), dict(N=0), dict(blocks=0),
                dict(divisor=0.0), dict(divisor=float('nan'))):
        assert fin(**bad) == -1, bad
    with pytest.raises(TypeError, match='takes 17 arguments'):
        _lib.call('pfst_sigloss_upsample_fwd', *([0] * 16))
    with pytest.raises(RuntimeError, match='GPU only'):
        hip_ops.sigloss_upsample_fwd(torch.zeros(1, 2, 4, 4), torch.zeros(1, 16, 16, dtype=torch.uint8), torch.ones(2, 2))
    # the caller's choice of form follows dice_form's rules
    class Fake:
        def __init__(self, shape, ptr=P):
            self.shape, self._ptr = shape, ptr

        def data_ptr(self):
            return self._ptr
    assert hip_ops.sigloss_form(Fake((2, 6, 19, 17)), Fake((2, 76, 68))) == (4, blocks4)
    assert hip_ops.sigloss_form(Fake((2, 6, 17, 18)), Fake((2, 136, 144)), Fake((2, 136, 144))) == (8, 2 * 2)
    assert hip_ops.sigloss_form(Fake((2, 6, 19, 17)), Fake((2, 76, 68)), generic=True) == (0, (76 * 68 + 1023) // 1024)
    assert hip_ops.sigloss_form(Fake((2, 33, 17, 18)), Fake((2, 136, 144)))[0] == 0
    assert hip_ops.sigloss_form(Fake((2, 6, 19, 17)), Fake((2, 76, 68)), Fake((2, 76, 68), P + 4))[0] == 0
    assert hip_ops.sigloss_form(Fake((2, 2, 7, 9)), Fake((2, 30, 37)))[0] == 0


def test_the_sampler_rule_for_sigmoid_terms():
    from pfst_amd.models import OHEMPixelSampler
    head = build_head(head_cfg('decode_head', BCE, sampler=dict(type='OHEMPixelSampler', thresh=0.7, min_kept=1000)))
    assert isinstance(head.sampler, OHEMPixelSampler) and head.sampler.thresh == 0.7
    build_head(head_cfg('auxiliary_head', [CE, BCE], sampler=dict(type='OHEMPixelSampler', thresh=0.5)))
    for losses in (BCE, [CE, BCE]):
        with pytest.raises(NotImplementedError, match='use_sigmoid=True'):
            build_head(head_cfg('decode_head', losses, sampler=dict(type='OHEMPixelSampler', min_kept=1000)))
    for sampler in (dict(type='OHEMPixelSampler', thresh=0.7), dict(type='OHEMPixelSampler')):
        for losses in (FOCAL, [CE, FOCAL]):
            with pytest.raises(NotImplementedError, match=r'FocalLoss \(loss_focal\)'):
                build_head(head_cfg('decode_head', losses, sampler=sampler))
