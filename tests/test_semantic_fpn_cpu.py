"""Semantic FPN on the host: the FPN neck and FPNHead build with the reference's state-dict keys and shapes (recorded in
tests/golden/semantic_fpn.npz by tests/golden/make_golden_semantic_fpn.py); EncoderDecoder(neck=...) registers the neck between backbone and
decode_head; the 'fpn' preset builds with the values of the reference's fpn_r50.py and no auxiliary head; `tools/train.py --supervised --model
fpn` reaches it and `--cfg-options model.neck...` its keys; the refusals are loud; the pseudo-feature statistics read a model with a neck;
hip_ops.nearest_src_index is torch's legacy 'nearest' rule."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM = dict(type='BN', requires_grad=True)
NECK = dict(type='FPN', in_channels=[8, 16, 24, 32], out_channels=16, num_outs=4)
HEAD = dict(type='FPNHead', in_channels=[16] * 4, in_index=[0, 1, 2, 3], feature_strides=[4, 8, 16, 32], channels=8, dropout_ratio=0.0,
            num_classes=6, norm_cfg=NORM, align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))


def build_neck(cfg):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_neck as build
    return build(cfg)


def build_head(cfg):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    return build(cfg)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'semantic_fpn.npz'))


def shapes_of(sd):
    return [','.join(str(d) for d in v.shape) for v in sd.values()]


def test_neck_and_head_state_dict_keys_and_shapes_are_the_references(golden):
    for part, module in (('neck', build_neck(dict(NECK))), ('head', build_head(dict(HEAD)))):
        sd = module.state_dict()
        assert list(sd) == list(golden[part + '|keys']), part
        assert shapes_of(sd) == list(golden[part + '|shapes']), part
    neck, head = build_neck(dict(NECK)).state_dict(), build_head(dict(HEAD)).state_dict()
    for k in ('lateral_convs.0.conv.weight', 'lateral_convs.3.conv.bias', 'fpn_convs.2.conv.bias'):
        assert k in neck, k
    assert not any('.bn.' in k for k in neck)                                   # norm_cfg=None: bare convolutions with a bias
    assert list(head)[:2] == ['conv_seg.weight', 'conv_seg.bias']
    for k in ('scale_heads.0.0.conv.weight', 'scale_heads.2.2.conv.weight', 'scale_heads.3.4.bn.running_var', 'scale_heads.3.4.conv.weight'):
        assert k in head, k
    assert not any(k.split('.')[2] in ('1', '3', '5') for k in head if k.startswith('scale_heads.'))      # the Upsample places hold nothing
    assert tuple(head['scale_heads.3.0.conv.weight'].shape) == (8, 16, 3, 3) and tuple(head['scale_heads.3.4.conv.weight'].shape) == (8, 8, 3, 3)
    # with a norm_cfg the neck's ConvModules get a bn and lose the bias; no_norm_on_lateral keeps the laterals bare
    sd = build_neck(dict(NECK, norm_cfg=NORM)).state_dict()
    assert 'lateral_convs.1.bn.running_mean' in sd and 'fpn_convs.1.bn.weight' in sd and 'fpn_convs.1.conv.bias' not in sd
    sd = build_neck(dict(NECK, norm_cfg=NORM, no_norm_on_lateral=True)).state_dict()
    assert 'lateral_convs.1.conv.bias' in sd and 'lateral_convs.1.bn.weight' not in sd and 'fpn_convs.1.bn.weight' in sd
    assert build_neck(dict(NECK, norm_cfg=NORM, act_cfg=dict(type='ReLU'))).fpn_convs[0].act and not build_neck(dict(NECK, norm_cfg=NORM)).fpn_convs[0].act


def test_encoder_decoder_registers_the_neck_between_backbone_and_head():
    import pfst_amd  # noqa: F401
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import build_segmentor
    cfg = baseline_model_cfg('pspnet', 6, 3)
    cfg['backbone'].update(stem_channels=16, base_channels=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1))
    cfg['neck'] = dict(NECK, in_channels=[16, 32, 64, 128])
    cfg['decode_head'] = dict(HEAD)
    cfg['auxiliary_head'].update(in_channels=16, channels=8)                    # reads the neck's level 2 (16 channels), as in the reference
    model = build_segmentor(cfg)
    assert list(model._modules)[:3] == ['backbone', 'neck', 'decode_head']
    names = [n for n, _ in model.named_parameters()]
    first = next(i for i, n in enumerate(names) if not n.startswith('backbone.'))
    assert names[first].startswith('neck.') and all(n.startswith('backbone.') for n in names[:first])
    assert [n.split('.')[0] for n in names[first:]] == sorted([n.split('.')[0] for n in names[first:]], key=['neck', 'decode_head', 'auxiliary_head'].index)
    # neck=None is today's model
    plain = build_segmentor(baseline_model_cfg('pspnet', 6, 3))
    assert plain.neck is None and list(plain._modules)[:2] == ['backbone', 'decode_head'] and not any(k.startswith('neck') for k in plain.state_dict())


def test_preset_builds():
    import pfst_amd  # noqa: F401
    from pfst_amd.presets import BASELINE_KINDS, baseline_model_cfg
    from pfst_amd.registry import build_segmentor
    assert 'fpn' in BASELINE_KINDS
    cfg = baseline_model_cfg('fpn', 6, 3)
    assert 'auxiliary_head' not in cfg
    assert cfg['backbone']['strides'] == (1, 2, 2, 2) and cfg['backbone']['dilations'] == (1, 1, 1, 1)
    assert cfg['neck'] == dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=4)
    head = cfg['decode_head']
    assert (head['type'], head['in_channels'], head['in_index'], head['feature_strides'], head['channels'], head['dropout_ratio']) == \
        ('FPNHead', [256] * 4, [0, 1, 2, 3], [4, 8, 16, 32], 128, 0.1)
    assert head['norm_cfg'] == NORM and cfg['backbone']['norm_cfg'] == NORM
    model = build_segmentor(cfg)
    assert not model.with_auxiliary_head and list(model._modules)[:3] == ['backbone', 'neck', 'decode_head']
    assert [m.conv.weight.shape[1] for m in model.neck.lateral_convs] == [256, 512, 1024, 2048]
    assert all(tuple(m.conv.weight.shape) == (256, 256, 3, 3) and m.conv.bias is not None and m.bn is None for m in model.neck.fpn_convs)
    assert model.neck.upsample_cfg == dict(mode='nearest')
    assert [len(s) for s in model.decode_head.scale_heads] == [1, 2, 4, 6]
    assert tuple(model.decode_head.scale_heads[0][0].conv.weight.shape) == (128, 256, 3, 3)
    # a biased layer stays off the Winograd route in every direction (open item)
    assert not any(m.conv.plan(True).wino for m in model.neck.fpn_convs) and model.decode_head.scale_heads[3][2].conv.plan(True).wino


def test_train_cli_model_switch_and_cfg_options_round_trip():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import build_train_model
    preset = 'pfst_inria_da_deeplabv3plus_r50-d8'
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--synthetic', '--model', 'fpn']))
    assert 'uda' not in cfg
    want = baseline_model_cfg('fpn', 2, 3)
    assert dict(cfg.model.decode_head) == want['decode_head'] and dict(cfg.model.neck) == want['neck'] and 'auxiliary_head' not in cfg.model
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--model', 'fpn', '--cfg-options', 'model.neck.out_channels=64',
                                                   'model.decode_head.in_channels=[64, 64, 64, 64]', 'model.decode_head.channels=32']))
    model = build_train_model(cfg)
    assert type(model.neck).__name__ == 'FPN' and type(model.decode_head).__name__ == 'FPNHead'
    assert tuple(model.neck.fpn_convs[3].conv.weight.shape) == (64, 64, 3, 3)
    assert tuple(model.decode_head.scale_heads[1][0].conv.weight.shape) == (32, 64, 3, 3)
    with pytest.raises(ValueError, match='--supervised'):
        train_cli.load_cfg(train_cli.parse_args([preset, '--model', 'fpn']))


def test_refusals_are_loud():
    for bad in (dict(add_extra_convs=True), dict(add_extra_convs='on_input'), dict(num_outs=5), dict(num_outs=3), dict(start_level=1),
                dict(end_level=3), dict(upsample_cfg=dict(mode='nearest', scale_factor=2)), dict(upsample_cfg=dict(mode='bicubic')),
                dict(upsample_cfg=dict(mode='bilinear', align_corners=True)), dict(conv_cfg=dict(type='Conv2d')),
                dict(norm_cfg=dict(type='SyncBN', requires_grad=True)), dict(act_cfg=dict(type='ReLU')),
                dict(in_channels=[8, 8, 16, 24, 32], num_outs=5)):
        with pytest.raises(NotImplementedError):
            build_neck(dict(NECK, **bad))
    build_neck(dict(NECK, upsample_cfg=dict(mode='bilinear')))                  # the existing topdown_merge
    with pytest.raises(NotImplementedError):
        build_head(dict(HEAD, align_corners=True))
    with pytest.raises(NotImplementedError):
        build_head(dict(HEAD, input_transform='multiple_select'))            # the head selects its levels itself; the argument stays refused
    with pytest.raises(NotImplementedError):
        build_head(dict(HEAD, norm_cfg=dict(type='SyncBN', requires_grad=True)))
    with pytest.raises(TypeError, match='lists'):
        build_head(dict(HEAD, in_channels=16, in_index=0))
    with pytest.raises(AssertionError):
        build_head(dict(HEAD, feature_strides=[4, 8, 16]))
    with pytest.raises(AssertionError):
        build_head(dict(HEAD, feature_strides=[8, 4, 16, 32]))
    # non-power-of-two strides follow the reference's int(log2 ...): 12 / 4 -> one stage
    assert [len(s) for s in build_head(dict(HEAD, feature_strides=[4, 12, 16, 40])).scale_heads] == [1, 2, 4, 6]
    # a single-level head builds
    assert len(build_head(dict(HEAD, in_channels=[16], in_index=[0], feature_strides=[4])).scale_heads) == 1
    # the adversarial segmentor keeps refusing a neck
    from pfst_amd.presets import advent_cfg, baseline_model_cfg
    from pfst_amd.registry import build_segmentor
    with pytest.raises(NotImplementedError, match='neck'):
        build_segmentor(advent_cfg(baseline_model_cfg('fpn', 6, 3))['model'])


def test_statistics_read_a_model_with_a_neck():
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.statistics import feature_dilation
    cfg = dict(model=baseline_model_cfg('fpn', 6, 3))
    assert feature_dilation(cfg, 'decoded', 2, None) == 2          # decoded features and logits share the stride-4 grid
    assert feature_dilation(cfg, 0, 2, None) == 2 and feature_dilation(cfg, 2, 4, None) == 1 and feature_dilation(cfg, 3, 8, None) == 1
    cfg['model']['decode_head']['feature_strides'] = [8, 16, 32, 64]
    assert feature_dilation(cfg, 'decoded', 2, None) == 1          # 'decoded' is feature_strides[0]
    with pytest.raises(NotImplementedError):
        feature_dilation(cfg, 1, 3, None)


def test_nearest_src_index_is_torchs_legacy_rule():
    from pfst_amd import hip_ops

    def torch_index(o, i):
        src = torch.arange(i, dtype=torch.float32)[None, None, :, None]
        return F.interpolate(src, size=(o, 1), mode='nearest')[0, 0, :, 0].to(torch.int64).numpy()
    pairs = [(i, o) for o in range(1, 97) for i in range(1, o + 1)] + [(125, 250), (63, 125), (32, 63), (128, 257), (86, 171)]
    for i, o in pairs:
        got = hip_ops.nearest_src_index(o, i)
        assert got.dtype == np.int64 and np.array_equal(got, torch_index(o, i)), (i, o)
