"""UPerHead and the stride-32 ResNetV1c on the GPU against what the reference's own modules returned (tests/golden/upernet.npz, made by
tests/golden/make_golden_upernet.py), under each of the three convolution arithmetics.  Head: in_channels [8, 16, 24, 32], channels 16, six
classes, N = 2, level grids 19 x 17 / 10 x 9 / 5 x 5 / 3 x 3 (no step an exact x2), labels 76 x 68 with a 255 region.  Backbone: strides
(1, 2, 2, 2) without dilation, stem 16 / base 4 channels, a 2 x 3 x 76 x 68 input, the cotangents of the generator.  Logits, features, input
gradients and parameter gradients are held to the project's per-link bound |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref|, the losses to
1e-4 max(|v|, 1e-3) (both: tests/test_baseline_heads_gpu.py).  Under f16x3 the head's forward launches no pfst_absmax: the merged maps and
the concat get their maxima from the kernels that write them."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORM = dict(type='BN', requires_grad=True)
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
HEAD = dict(type='UPerHead', in_channels=[8, 16, 24, 32], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=16, dropout_ratio=0.0,
            num_classes=6, norm_cfg=NORM, align_corners=False)
BACKBONE = dict(type='ResNetV1c', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), dilations=(1, 1, 1, 1), strides=(1, 2, 2, 2), norm_cfg=NORM,
                norm_eval=False, style='pytorch', contract_dilation=True, in_channels=3, stem_channels=16, base_channels=4)
GRAD_BLOCKS = ('layer3.0.', 'layer4.0.')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'upernet.npz'))


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


def cotangent(i, shape):
    """make_golden_upernet.cotangent: cos(0.37 k + i) over the flat index k, as fp32"""
    k = np.arange(int(np.prod(shape)), dtype=np.float64)
    return torch.from_numpy(np.cos(0.37 * k + i).astype(np.float32).reshape(tuple(shape)))


def load_golden_params(module, golden, part):
    """fill_state_dict over the reference's key order: what the generator loaded into the reference"""
    from pfst_amd.synthetic import fill_state_dict
    sd = OrderedDict((str(k), torch.zeros([int(d) for d in str(s).split(',')] if str(s) else [],
                                          dtype=torch.int64 if str(k).endswith('num_batches_tracked') else torch.float32))
                     for k, s in zip(golden[part + '|keys'], golden[part + '|shapes']))
    fill_state_dict(sd, int(golden['seed']))
    res = module.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return module.to(DEV)


def prepare(module):
    for p in module.parameters():
        p.grad = torch.zeros_like(p)
    for m in module.modules():
        if hasattr(m, 'repack'):
            m.repack(True)


def build_head(golden, loss_decode=CE, **extra):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    return load_golden_params(build(dict(HEAD, loss_decode=loss_decode, **extra)), golden, 'head')


def run_head(head, golden, count=None):
    """forward, losses, backward.  count: a list that receives the name of every library call made during the forward pass"""
    from pfst_amd import _lib, hip_ops, layers
    from pfst_amd.engine import Tape, Var
    prepare(head)
    xs = [Var(torch.from_numpy(golden[f'head|x{i}'].astype(np.float32)).to(DEV), True) for i in range(4)]
    if layers.CONV_MATH == 'f16x3':
        for x in xs:                     # as the backbone hands them over: the layer that wrote a map published its maximum
            x.amax = hip_ops.absmax(x.data)
    label = torch.from_numpy(golden['label']).to(DEV)
    tape = Tape()
    real = _lib.call
    if count is not None:
        def counting(name, *args):
            count.append(name)
            return real(name, *args)
        _lib.call = hip_ops.call = counting
    try:
        logits, feats = head.forward(xs, return_features=True, tape=tape, training=True)
    finally:
        _lib.call = hip_ops.call = real
    res = head.losses(logits, label, None, tape)
    tape.backward()
    torch.cuda.synchronize()
    return logits, feats, res, [x.grad for x in xs]


def test_head_matches_the_reference(golden, conv_math):
    head = build_head(golden)
    logits, feats, res, dxs = run_head(head, golden)
    worst = {}
    worst['logits'] = link_ratio(logits.data, torch.from_numpy(golden['head|logits']))
    worst['feats'] = link_ratio(feats.data, torch.from_numpy(golden['head|feats']))
    for i, dx in enumerate(dxs):
        worst[f'dx{i}'] = link_ratio(dx, torch.from_numpy(golden[f'head|dx{i}']))
    for k, p in head.named_parameters():
        worst['grad ' + k] = link_ratio(p.grad, torch.from_numpy(golden['head|grad|' + k]))
    for k, v in worst.items():
        print(f'upernet head {conv_math} {k}: {v:.3f} of the per-link bound')
    for k, want in zip(golden['head|loss_names'], golden['head|loss_values']):
        got = float(res[str(k)])
        print(f'upernet head {conv_math} {k}: {got!r} reference {float(want)!r}')
        assert abs(got - want) <= 1e-4 * max(abs(want), 1e-3), (k, got, want)
    assert float(res['_bad_labels']) == 0.0
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_backbone_matches_the_reference(golden, conv_math):
    import pfst_amd  # noqa: F401
    from pfst_amd.engine import Tape, Var
    from pfst_amd.registry import build_backbone
    net = load_golden_params(build_backbone(dict(BACKBONE)), golden, 'backbone')
    prepare(net)
    img = Var(torch.from_numpy(golden['img'].astype(np.float32)).to(DEV), True)
    tape = Tape()
    outs = net(img, tape)
    assert [tuple(o.data.shape) for o in outs] == [(2, 16, 19, 17), (2, 32, 10, 9), (2, 64, 5, 5), (2, 128, 3, 3)]
    for i, o in enumerate(outs):
        o._grad = cotangent(i, o.data.shape).to(DEV)
    tape.backward()
    torch.cuda.synchronize()
    worst = {f'out{i}': link_ratio(o.data, torch.from_numpy(golden[f'backbone|out{i}'])) for i, o in enumerate(outs)}
    worst['dimg'] = link_ratio(img.grad, torch.from_numpy(golden['backbone|dimg']))
    checked = 0
    for k, p in net.named_parameters():
        if k.startswith(GRAD_BLOCKS):
            worst['grad ' + k] = link_ratio(p.grad, torch.from_numpy(golden['backbone|grad|' + k]))
            checked += 1
    assert checked == 2 * 12               # three convolutions and a downsample, each with its BatchNorm's weight and bias, per block
    for k, v in worst.items():
        print(f'upernet backbone {conv_math} {k}: {v:.3f} of the per-link bound')
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_no_absmax_launch_in_the_heads_forward_under_f16x3(golden):
    from pfst_amd import layers
    prev, layers.CONV_MATH = layers.CONV_MATH, 'f16x3'
    try:
        calls = []
        run_head(build_head(golden), golden, count=calls)
        assert calls.count('pfst_topdown_merge') == 3 and calls.count('pfst_fpn_resize_concat') == 1, calls
        assert calls.count('pfst_absmax') == 0, [c for c in calls if c == 'pfst_absmax']
        # a head wide enough for every 3x3 and 1x1 layer to run on the f16x3 kernels, which scale their operands from the published maxima
        import pfst_amd  # noqa: F401
        from pfst_amd.engine import Var
        from pfst_amd import hip_ops
        from pfst_amd.registry import build_head as build
        torch.manual_seed(2)
        wide = build(dict(HEAD, in_channels=[64, 64, 128, 128], channels=128, loss_decode=CE)).to(DEV)
        prepare(wide)
        assert wide.fpn_convs[1].conv.fprop_reads_amax and wide.fpn_bottleneck.conv.fprop_reads_amax
        xs = [Var(torch.relu(torch.randn(2, c, h, w, device=DEV)), False) for c, (h, w) in zip([64, 64, 128, 128], [(32, 32), (16, 16), (8, 8), (4, 4)])]
        for x in xs:
            x.amax = hip_ops.absmax(x.data)
        sizes = []
        real = hip_ops.call

        def counting(name, *args):
            if name == 'pfst_absmax':
                sizes.append(int(args[1]) * int(args[2]))
            return real(name, *args)
        hip_ops.call = counting
        try:
            logits, feats = wide.forward(xs, return_features=True, tape=None, training=True)
        finally:
            hip_ops.call = real
        torch.cuda.synchronize()
        assert bool(torch.isfinite(logits.data).all()) and tuple(feats.data.shape) == (2, 128, 32, 32)
        # the only maxima taken by a pass of their own are those of the pyramid's pooled grids (at most 6 x 6 cells), as in PSPHead
        assert all(s <= 2 * 128 * 36 for s in sizes), sizes
    finally:
        layers.CONV_MATH = prev


def test_head_with_a_loss_list_and_a_sampler(golden):
    dice = dict(type='DiceLoss', loss_weight=3.0)
    head = build_head(golden, loss_decode=[CE, dice])
    logits, feats, res, dxs = run_head(head, golden)
    assert list(res) == ['loss_ce', 'loss_dice', 'acc_seg', '_bad_labels']
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
    assert all(bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0 for dx in dxs)
    want = dict(zip([str(k) for k in golden['head|loss_names']], golden['head|loss_values']))
    assert abs(float(res['loss_ce']) - want['loss_ce']) <= 1e-4 * abs(want['loss_ce'])          # the CE term alone is the golden's
    head = build_head(golden, sampler=dict(type='OHEMPixelSampler', thresh=0.7, min_kept=500))
    logits, feats, res, dxs = run_head(head, golden)
    info = head.sampler.last_info.cpu()
    assert 500 * 2 <= int(info[2]) <= int(info[1])
    assert all(bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0 for dx in dxs)
    assert abs(float(res['acc_seg']) - want['acc_seg']) <= 1e-3 * want['acc_seg']                # the same forward: the sampler changes the weights only
    assert all(float(p.grad.abs().max()) > 0 and bool(torch.isfinite(p.grad).all()) for p in head.parameters())
