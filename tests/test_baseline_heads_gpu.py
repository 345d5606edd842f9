"""PSPHead, ASPPHead and the general FCNHead on the GPU against what the reference's own heads returned (tests/golden/decode_heads.npz, made by
tests/golden/make_golden_heads.py: in_channels 32, channels 16, six classes, N = 2, a 19 x 17 grid, labels 76 x 68 with a 255 region), under
each of the three convolution arithmetics.  Logits, features, the input gradient and every parameter gradient are held to the project's
per-link bound |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref| (tests/test_layer_backward_gpu.py), the losses to 1e-4 max(|v|, 1e-3)."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
COMMON = dict(in_channels=32, in_index=0, channels=16, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True),
              align_corners=False)
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
HEADS = {'psp': dict(type='PSPHead', pool_scales=(1, 2, 3, 6)), 'aspp': dict(type='ASPPHead', dilations=(1, 2, 3, 5)),
         'fcn': dict(type='FCNHead', num_convs=2, kernel_size=3, concat_input=True)}


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'decode_heads.npz'))


@pytest.fixture(params=['f32', 'bf16x6', 'f16x3'])
def conv_math(request):
    from pfst_amd import layers
    prev, layers.CONV_MATH = layers.CONV_MATH, request.param
    yield request.param
    layers.CONV_MATH = prev


def link_ratio(got, ref):
    """max over the elements of |got - ref| / (1e-4 max|ref| + 1e-3 |ref|): within the per-link bound iff <= 1"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (1e-4 * ref.abs().max() + 1e-3 * ref.abs())).max())


def build_head(golden, name, loss_decode=CE, **extra):
    """the head with the golden's parameters: fill_state_dict over the reference's key order (what the generator loaded into the reference)"""
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    from pfst_amd.synthetic import fill_state_dict
    head = build(dict(HEADS[name], loss_decode=loss_decode, **COMMON, **extra))
    sd = OrderedDict((str(k), torch.zeros([int(d) for d in str(s).split(',')] if str(s) else [], dtype=torch.int64 if str(k).endswith('num_batches_tracked') else torch.float32))
                     for k, s in zip(golden[name + '|keys'], golden[name + '|shapes']))
    fill_state_dict(sd, int(golden['seed']))
    res = head.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return head.to(DEV)


def run_head(head, golden):
    from pfst_amd.engine import Tape, Var
    for p in head.parameters():
        p.grad = torch.zeros_like(p)
    for m in head.modules():
        if hasattr(m, 'repack'):
            m.repack(True)
    x = Var(torch.from_numpy(golden['x'].astype(np.float32)).to(DEV), True)
    label = torch.from_numpy(golden['label']).to(DEV)
    tape = Tape()
    logits, feats = head.forward([x], return_features=True, tape=tape, training=True)
    res = head.losses(logits, label, None, tape)
    tape.backward()
    torch.cuda.synchronize()
    return logits, feats, res, x.grad


@pytest.mark.parametrize('name', list(HEADS))
def test_head_matches_the_reference(golden, conv_math, name):
    head = build_head(golden, name)
    logits, feats, res, dx = run_head(head, golden)
    worst = {}
    worst['logits'] = link_ratio(logits.data, torch.from_numpy(golden[name + '|logits']))
    worst['feats'] = link_ratio(feats.data, torch.from_numpy(golden[name + '|feats']))
    worst['dx'] = link_ratio(dx, torch.from_numpy(golden[name + '|dx']))
    for k, p in head.named_parameters():
        worst['grad ' + k] = link_ratio(p.grad, torch.from_numpy(golden[name + '|grad|' + k]))
    for k, v in worst.items():
        print(f'{name} {conv_math} {k}: {v:.3f} of the per-link bound')
    for k, want in zip(golden[name + '|loss_names'], golden[name + '|loss_values']):
        got = float(res[str(k)])
        print(f'{name} {conv_math} {k}: {got!r} reference {float(want)!r}')
        assert abs(got - want) <= 1e-4 * max(abs(want), 1e-3), (k, got, want)
    assert float(res['_bad_labels']) == 0.0
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_psp_head_with_a_loss_list_and_a_sampler(golden):
    dice = dict(type='DiceLoss', loss_weight=3.0)
    head = build_head(golden, 'psp', loss_decode=[CE, dice])
    logits, feats, res, dx = run_head(head, golden)
    assert list(res) == ['loss_ce', 'loss_dice', 'acc_seg', '_bad_labels']
    assert all(bool(torch.isfinite(v).all()) for v in res.values()) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    # the CE term alone is the golden's: the Dice term adds to the gradient, not to loss_ce
    want = dict(zip([str(k) for k in golden['psp|loss_names']], golden['psp|loss_values']))
    assert abs(float(res['loss_ce']) - want['loss_ce']) <= 1e-4 * abs(want['loss_ce'])
    head = build_head(golden, 'psp', sampler=dict(type='OHEMPixelSampler', thresh=0.7, min_kept=500))
    logits, feats, res, dx2 = run_head(head, golden)
    info = head.sampler.last_info.cpu()
    assert 500 * 2 <= int(info[2]) <= int(info[1]) and bool(torch.isfinite(dx2).all()) and float(dx2.abs().max()) > 0
    assert abs(float(res['acc_seg']) - want['acc_seg']) <= 1e-3 * want['acc_seg']           # the same forward: the sampler changes the weights only


def test_fcn_variants_run(golden):
    """num_convs 0 (with and without conv_cat), kernel 1, dilation 2: forward, losses and backward run and stay finite; the auxiliary form
    (num_convs = 1, no concat) takes its old branch"""
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    for cfg in (dict(num_convs=0, concat_input=False, channels=32), dict(num_convs=0, concat_input=True, channels=32),
                dict(num_convs=3, kernel_size=1, concat_input=True), dict(num_convs=2, kernel_size=3, dilation=2, concat_input=False),
                dict(num_convs=1, concat_input=False)):
        head = build(dict(dict(COMMON, loss_decode=CE), type='FCNHead', **cfg)).to(DEV)
        logits, feats, res, dx = run_head(head, golden)
        assert tuple(logits.data.shape) == (2, 6, 19, 17) and tuple(feats.data.shape) == (2, cfg.get('channels', 16), 19, 17)
        assert bool(torch.isfinite(res['loss_ce']).all()) and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0, cfg
        assert all(float(p.grad.abs().max()) > 0 for p in head.parameters()), cfg
