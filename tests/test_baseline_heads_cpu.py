"""The comparison decode heads on the host: PSPHead, ASPPHead and the general FCNHead build (state-dict keys and shapes equal the reference's,
recorded in tests/golden/decode_heads.npz), the three presets and a ResNetV1c-101 build, the refusals are loud, `tools/train.py --supervised
--model` and `--cfg-options` reach the heads, and the host-built operator tables of the pyramid kernels reproduce F.adaptive_avg_pool2d and
F.interpolate in fp64."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = dict(in_channels=32, in_index=0, channels=16, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True),
              align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
HEADS = {'psp': dict(type='PSPHead', pool_scales=(1, 2, 3, 6)), 'aspp': dict(type='ASPPHead', dilations=(1, 2, 3, 5)),
         'fcn': dict(type='FCNHead', num_convs=2, kernel_size=3, concat_input=True)}


def build(cfg):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head
    return build_head(cfg)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'decode_heads.npz'))


@pytest.mark.parametrize('name', list(HEADS))
def test_state_dict_keys_and_shapes_are_the_references(golden, name):
    sd = build(dict(HEADS[name], **COMMON)).state_dict()
    assert list(sd) == list(golden[name + '|keys'])
    assert [','.join(str(d) for d in v.shape) for v in sd.values()] == list(golden[name + '|shapes'])


def test_psp_keys_follow_the_image_pool_layout():
    sd = build(dict(HEADS['psp'], **COMMON)).state_dict()
    assert 'psp_modules.3.1.conv.weight' in sd and 'psp_modules.0.1.bn.running_mean' in sd
    assert tuple(sd['bottleneck.conv.weight'].shape) == (16, 32 + 4 * 16, 3, 3)


@pytest.mark.parametrize('kind', ['pspnet', 'deeplabv3', 'fcn'])
def test_presets_build(kind):
    import pfst_amd  # noqa: F401
    from pfst_amd.presets import baseline_model_cfg, model_cfg
    from pfst_amd.registry import build_segmentor
    cfg = baseline_model_cfg(kind, 6, 3)
    assert cfg['auxiliary_head'] == model_cfg(6, 3)['auxiliary_head'] and cfg['backbone']['depth'] == 50
    model = build_segmentor(cfg)
    want = dict(pspnet='PSPHead', deeplabv3='ASPPHead', fcn='FCNHead')[kind]
    assert type(model.decode_head).__name__ == want and model.decode_head.channels == 512
    if kind == 'pspnet':
        assert model.decode_head.pool_scales == (1, 2, 3, 6) and model.decode_head.bottleneck.conv.weight.shape[1] == 2048 + 4 * 512
    if kind == 'deeplabv3':
        assert [m.conv.weight.shape[-1] for m in model.decode_head.aspp_modules] == [1, 3, 3, 3]
        assert [m.conv.dilation for m in model.decode_head.aspp_modules] == [1, 12, 24, 36]
    if kind == 'fcn':
        assert len(model.decode_head.convs) == 2 and model.decode_head.conv_cat.conv.weight.shape[1] == 2048 + 512
    with pytest.raises(ValueError):
        baseline_model_cfg('unet', 6, 3)


def test_resnet101_builds():
    import pfst_amd  # noqa: F401
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import build_backbone
    net = build_backbone(baseline_model_cfg('pspnet', 2, 14, depth=101)['backbone'])
    assert len(net.layer3) == 23 and net.stem[0].weight.shape[1] == 14


def test_refusals_are_loud():
    with pytest.raises(NotImplementedError):
        build(dict(HEADS['psp'], **dict(COMMON, align_corners=True)))
    with pytest.raises(NotImplementedError):
        build(dict(HEADS['aspp'], **dict(COMMON, align_corners=True)))
    with pytest.raises(NotImplementedError, match='scales'):
        build(dict(type='PSPHead', pool_scales=(1, 2, 9), **COMMON))
    with pytest.raises(NotImplementedError, match='scales'):
        build(dict(type='PSPHead', pool_scales=(1, 2, 3, 4, 5, 6, 7), **COMMON))
    with pytest.raises(ValueError, match='num_convs=0'):
        build(dict(type='FCNHead', num_convs=0, concat_input=False, **COMMON))
    with pytest.raises(NotImplementedError, match='kernel_size'):
        build(dict(type='FCNHead', num_convs=1, kernel_size=5, concat_input=False, **COMMON))
    build(dict(type='FCNHead', num_convs=0, concat_input=True, **dict(COMMON, channels=32)))           # in_channels == channels: builds


def test_fcn_variants_build_with_the_references_modules():
    h = build(dict(type='FCNHead', num_convs=3, kernel_size=1, concat_input=False, dilation=2, **COMMON))
    assert len(h.convs) == 3 and h.convs[0].conv.weight.shape == (16, 32, 1, 1) and not hasattr(h, 'conv_cat')
    h = build(dict(type='FCNHead', num_convs=0, concat_input=False, **dict(COMMON, channels=32)))
    assert isinstance(h.convs, torch.nn.Identity)
    aux = build(dict(type='FCNHead', num_convs=1, concat_input=False, dilation=3, **COMMON))                       # the auxiliary head, as before
    assert list(aux.state_dict())[:3] == ['conv_seg.weight', 'conv_seg.bias', 'convs.0.conv.weight'] and aux.convs[0].conv.padding == 3


def test_train_cli_model_switch_and_cfg_options_round_trip():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import build_train_model
    preset = 'pfst_inria_da_deeplabv3plus_r50-d8'
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--synthetic', '--model', 'pspnet']))
    assert 'uda' not in cfg
    assert dict(cfg.model.decode_head) == baseline_model_cfg('pspnet', 2, 3)['decode_head']
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--model', 'pspnet', '--cfg-options',
                                                   'model.decode_head.pool_scales=(1, 2, 4)', 'model.backbone.depth=101']))
    model = build_train_model(cfg)
    assert model.decode_head.pool_scales == (1, 2, 4) and len(model.backbone.layer3) == 23
    # the same model through --cfg-options alone
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--cfg-options',
                                                   "model.decode_head=dict(type='ASPPHead', in_channels=2048, in_index=3, channels=512, "
                                                   "dilations=(1, 12, 24, 36), dropout_ratio=0.1, num_classes=2, norm_cfg=dict(type='BN', "
                                                   "requires_grad=True), align_corners=False, loss_decode=dict(type='CrossEntropyLoss', "
                                                   "use_sigmoid=False, loss_weight=1.0))"]))
    with pytest.raises(ValueError, match='--supervised'):
        train_cli.load_cfg(train_cli.parse_args([preset, '--model', 'fcn']))


@pytest.mark.parametrize('h,w', [(13, 10), (5, 7), (16, 16), (128, 128)])
def test_operator_tables_reproduce_torch_in_fp64(h, w):
    from pfst_amd.hip_ops import pyramid_operator
    scales = (1, 2, 3, 6)
    x = torch.randn(2, 3, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h * w))
    tabs = {(kind, n): pyramid_operator(kind, n, scales) for kind in ('pool', 'bilinear') for n in (h, w)}
    o = 0
    for k, s in enumerate(scales):
        rh, rw = (torch.from_numpy(tabs['pool', n][0][o:o + s]) for n in (h, w))
        err = float((torch.einsum('iy,ncyx,jx->ncij', rh, x, rw) - F.adaptive_avg_pool2d(x, s)).abs().max())
        g = torch.randn(2, 3, s, s, dtype=torch.float64, generator=torch.Generator().manual_seed(s))
        ah, aw = (torch.from_numpy(tabs['bilinear', n][0][o:o + s]) for n in (h, w))
        err2 = float((torch.einsum('iy,ncij,jx->ncyx', ah, g, aw) - F.interpolate(g, (h, w), mode='bilinear', align_corners=False)).abs().max())
        print(f'{h}x{w} s={s}: pool {err:.1e} bilinear {err2:.1e}')
        assert err <= 1e-14 and err2 <= 1e-14
        o += s
    # the spans the kernels walk cover every non-zero, row-wise and pixel-wise
    for (kind, n), (dense, span, tspan) in tabs.items():
        assert dense.shape == (sum(scales), n) and span.shape == (sum(scales), 2) and tspan.shape == (len(scales), n, 2)
        cover = np.zeros_like(dense, bool)
        for i, (a, b) in enumerate(span):
            cover[i, a:b] = True
        assert not (dense[~cover] != 0).any()
        o = 0
        for k, s in enumerate(scales):
            cover = np.zeros((s, n), bool)
            for p, (a, b) in enumerate(tspan[k]):
                assert 0 <= a < b <= s
                cover[a:b, p] = True
            assert not (dense[o:o + s][~cover] != 0).any()
            o += s

