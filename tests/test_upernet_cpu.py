"""UPerNet on the host: UPerHead builds with the reference's state-dict keys and shapes (recorded in tests/golden/upernet.npz by
tests/golden/make_golden_upernet.py), so does the narrow stride-32 ResNetV1c of that golden; the 'upernet' preset builds; `tools/train.py
--supervised --model upernet` reaches it and `--cfg-options` its keys; the refusals are loud; the pseudo-feature statistics read a
multi-level `in_index`."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM = dict(type='BN', requires_grad=True)
HEAD = dict(type='UPerHead', in_channels=[8, 16, 24, 32], in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=16, dropout_ratio=0.0,
            num_classes=6, norm_cfg=NORM, align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
BACKBONE = dict(type='ResNetV1c', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), dilations=(1, 1, 1, 1), strides=(1, 2, 2, 2), norm_cfg=NORM,
                norm_eval=False, style='pytorch', contract_dilation=True, in_channels=3, stem_channels=16, base_channels=4)


def build(cfg):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head
    return build_head(cfg)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'upernet.npz'))


def shapes_of(sd):
    return [','.join(str(d) for d in v.shape) for v in sd.values()]


def test_head_state_dict_keys_and_shapes_are_the_references(golden):
    sd = build(dict(HEAD)).state_dict()
    assert list(sd) == list(golden['head|keys'])
    assert shapes_of(sd) == list(golden['head|shapes'])
    for k in ('psp_modules.3.1.conv.weight', 'bottleneck.bn.running_var', 'lateral_convs.2.conv.weight', 'fpn_convs.0.bn.weight',
              'fpn_bottleneck.conv.weight', 'conv_seg.bias'):
        assert k in sd, k
    assert not any(k.startswith(('lateral_convs.3', 'fpn_convs.3')) for k in sd)          # the top level's lateral is the PPM's bottleneck


def test_backbone_state_dict_keys_and_shapes_are_the_references(golden):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_backbone
    net = build_backbone(dict(BACKBONE))
    sd = net.state_dict()
    assert list(sd) == list(golden['backbone|keys'])
    assert shapes_of(sd) == list(golden['backbone|shapes'])
    assert [net.layer3[0].conv2.stride, net.layer4[0].conv2.stride, net.layer4[0].conv2.dilation] == [2, 2, 1]


def test_preset_builds():
    import pfst_amd  # noqa: F401
    from pfst_amd.presets import BASELINE_KINDS, baseline_model_cfg, model_cfg
    from pfst_amd.registry import build_segmentor
    assert 'upernet' in BASELINE_KINDS
    cfg = baseline_model_cfg('upernet', 6, 3)
    assert cfg['auxiliary_head'] == model_cfg(6, 3)['auxiliary_head'] and cfg['auxiliary_head']['in_index'] == 2
    assert cfg['backbone']['strides'] == (1, 2, 2, 2) and cfg['backbone']['dilations'] == (1, 1, 1, 1)
    assert cfg['backbone']['norm_cfg'] == NORM and cfg['decode_head']['norm_cfg'] == NORM
    model = build_segmentor(cfg)
    head = model.decode_head
    assert type(head).__name__ == 'UPerHead' and head.channels == 512 and head.in_channels == [256, 512, 1024, 2048]
    assert head.in_index == [0, 1, 2, 3] and head.pool_scales == (1, 2, 3, 6)
    assert head.bottleneck.conv.weight.shape[1] == 2048 + 4 * 512 and head.fpn_bottleneck.conv.weight.shape[1] == 4 * 512
    assert [m.conv.weight.shape[1] for m in head.lateral_convs] == [256, 512, 1024] and len(head.fpn_convs) == 3
    assert [model.backbone.layer3[0].conv2.stride, model.backbone.layer4[0].conv2.stride] == [2, 2]
    assert all(b.conv2.dilation == 1 for b in list(model.backbone.layer3) + list(model.backbone.layer4))


def test_train_cli_model_switch_and_cfg_options_round_trip():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import build_train_model
    preset = 'pfst_inria_da_deeplabv3plus_r50-d8'
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--synthetic', '--model', 'upernet']))
    assert 'uda' not in cfg
    want = baseline_model_cfg('upernet', 2, 3)
    assert dict(cfg.model.decode_head) == want['decode_head']
    assert tuple(cfg.model.backbone['strides']) == (1, 2, 2, 2) and tuple(cfg.model.backbone['dilations']) == (1, 1, 1, 1)
    cfg = train_cli.load_cfg(train_cli.parse_args([preset, '--supervised', '--model', 'upernet', '--cfg-options',
                                                   'model.decode_head.pool_scales=(1, 2, 4)', 'model.decode_head.channels=64']))
    model = build_train_model(cfg)
    assert type(model.decode_head).__name__ == 'UPerHead' and model.decode_head.pool_scales == (1, 2, 4)
    assert model.decode_head.fpn_bottleneck.conv.weight.shape[:2] == (64, 4 * 64)
    with pytest.raises(ValueError, match='--supervised'):
        train_cli.load_cfg(train_cli.parse_args([preset, '--model', 'upernet']))


def test_refusals_are_loud():
    with pytest.raises(NotImplementedError):
        build(dict(HEAD, align_corners=True))
    with pytest.raises(NotImplementedError):
        build(dict(HEAD, input_transform='multiple_select'))          # the head selects its levels itself; the argument stays refused
    with pytest.raises(NotImplementedError, match='scales'):
        build(dict(HEAD, pool_scales=(1, 2, 9)))
    with pytest.raises(NotImplementedError, match='scales'):
        build(dict(HEAD, pool_scales=(1, 2, 3, 4, 5, 6, 7)))
    with pytest.raises(TypeError, match='lists'):
        build(dict(HEAD, in_channels=32, in_index=3))                  # a scalar in_channels: a single-level head's
    with pytest.raises(TypeError, match='lists'):
        build(dict(HEAD, in_index=[0, 1, 2]))
    with pytest.raises(NotImplementedError, match='levels'):
        build(dict(HEAD, in_channels=[8, 8, 16, 24, 32], in_index=[0, 0, 1, 2, 3]))


def test_statistics_read_a_multi_level_in_index():
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.statistics import feature_dilation
    cfg = dict(model=baseline_model_cfg('upernet', 6, 3))
    assert feature_dilation(cfg, 'decoded', 2, None) == 2          # decoded features and logits share the stride-4 grid
    assert feature_dilation(cfg, 3, 8, None) == 1                  # level 3 is stride 32 here
    with pytest.raises(NotImplementedError):
        feature_dilation(cfg, 1, 3, None)                          # dilation 3 on a stride-8 map under the stride-4 loss grid
