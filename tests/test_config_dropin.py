"""Drop-in boundary on the CPU: the reference's own configs build the registered types with the reference's checkpoint layout.
The configs' values after `_base_` merging are pinned in tests/golden/reference_configs.json (make_golden.py); where the reference's
config files are present, loading them with Config.fromfile must give exactly those values."""
import json
import os

import numpy as np
import pytest

REF_CFG = '/root/reference/configs/pfst'
NAMES = ['pfst_pots_irrg2vaih_irrg', 'pfst_vaih_irrg2pots_irrg', 'pfst_inria_da', 'pfst_season_net_sp2fa']


def _dec(v):
    if isinstance(v, dict):
        return tuple(_dec(x) for x in v['__tuple__']) if set(v) == {'__tuple__'} else {k: _dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_dec(x) for x in v]
    return v


def reference_config(name, golden_dir):
    """Config of configs/pfst/<name>_deeplabv3plus_r50-d8.py: the pinned values, checked against the file where it exists"""
    from pfst_amd.config import Config
    with open(os.path.join(golden_dir, 'reference_configs.json')) as f:
        pinned = _dec(json.load(f)[name])
    path = os.path.join(REF_CFG, f'{name}_deeplabv3plus_r50-d8.py')
    if os.path.exists(path):
        assert Config.fromfile(path).to_dict() == pinned
    return Config(pinned, filename=path)


@pytest.mark.parametrize('name', NAMES)
def test_reference_configs_load_and_build(name, golden_dir):
    import pfst_amd  # noqa: F401
    from pfst_amd.config import parse_cfg_options
    from pfst_amd.registry import build_train_model
    cfg = reference_config(name, golden_dir)
    cfg.merge_from_dict(parse_cfg_options(['model.pretrained=None', 'runner.max_iters=123']))
    assert cfg.uda.type == 'PFGST' and cfg.uda.aux_losses[0]['type'] == 'PFGSTLoss'
    model = build_train_model(cfg)
    assert model.max_iters == 123
    keys = [k for k in model.state_dict().keys() if k != '_extra_state']
    gold = [str(k) for k in np.load(os.path.join(golden_dir, 'train_step.npz'))['keys']]
    assert keys == gold                              # the reference's 848 keys in the reference's order
    nc = cfg.model.decode_head.num_classes
    assert model.model.decode_head.conv_seg.weight.shape[0] == nc
    assert not any(p.requires_grad for p in model.ema_model.parameters())


def test_presets_match_reference_configs_when_available(golden_dir):
    from pfst_amd.presets import WORKLOADS, workload_cfg
    for name, w in WORKLOADS.items():
        cfg, _ = workload_cfg(name)
        assert cfg['model']['decode_head']['num_classes'] == w['num_classes']
        ref = reference_config(name[:-len('_deeplabv3plus_r50-d8')], golden_dir)
        assert ref.uda.pseudo_threshold == cfg['pseudo_threshold'] and ref.uda.alpha == cfg['alpha']
        assert ref.uda.aux_losses[0]['downscale'] == w['downscale']
        assert ref.model.decode_head.num_classes == w['num_classes']


def test_fromfile_merges_base_files(tmp_path):
    """`_base_` inheritance as the reference's config files use it: a list of relative paths merged in order, nested dicts merged key
    by key, `_delete_=True` replacing a dict, the file's own values last"""
    from pfst_amd.config import Config
    (tmp_path / '_base_').mkdir()
    (tmp_path / 'pfst').mkdir()
    (tmp_path / '_base_' / 'model.py').write_text("norm_cfg = dict(type='BN', requires_grad=True)\n"
                                                  "model = dict(type='EncoderDecoder', decode_head=dict(num_classes=19, dilations=(1, 12, 24, 36)),\n"
                                                  "             auxiliary_head=dict(num_classes=19, norm_cfg=norm_cfg))\n")
    (tmp_path / '_base_' / 'schedule.py').write_text("optimizer = dict(type='AdamW', lr=6e-05, paramwise_cfg=dict(custom_keys=dict(head=dict(lr_mult=10.0))))\n"
                                                     "runner = dict(type='IterBasedRunner', max_iters=40000)\n")
    (tmp_path / 'pfst' / 'cfg.py').write_text("_base_ = ['../_base_/model.py', '../_base_/schedule.py']\nseed = 0\n"
                                              "model = dict(decode_head=dict(num_classes=6), auxiliary_head=dict(num_classes=6))\n"
                                              "optimizer = dict(lr=1e-04, paramwise_cfg=dict(_delete_=True, decay_mult=0.0))\n")
    cfg = Config.fromfile(str(tmp_path / 'pfst' / 'cfg.py'))
    assert cfg.to_dict() == dict(
        norm_cfg=dict(type='BN', requires_grad=True), seed=0,
        model=dict(type='EncoderDecoder', decode_head=dict(num_classes=6, dilations=(1, 12, 24, 36)),
                   auxiliary_head=dict(num_classes=6, norm_cfg=dict(type='BN', requires_grad=True))),
        optimizer=dict(type='AdamW', lr=1e-04, paramwise_cfg=dict(decay_mult=0.0)),
        runner=dict(type='IterBasedRunner', max_iters=40000))
    assert cfg.model.decode_head.num_classes == 6 and cfg.runner.max_iters == 40000


def test_unknown_options_fail_loudly():
    import pfst_amd  # noqa: F401
    from pfst_amd.presets import uda_cfg
    from pfst_amd.registry import UDA
    cfg = uda_cfg()
    cfg['imnet_feature_dist_lambda'] = 0.005          # DAFormer feature distance: not part of the PFST configs
    with pytest.raises(NotImplementedError):
        UDA.build(cfg)
    with pytest.raises(KeyError):
        UDA.build(dict(type='DACS'))


def test_winograd_dispatch_rules():
    """Host-side dispatch of the wide stride-1 3x3 layers to the Winograd path (pfst_amd/layers.py): geometry and size rules."""
    import pfst_amd  # noqa: F401
    from pfst_amd import layers
    from pfst_amd.layers import Conv2dP
    assert layers.WINOGRAD                                            # on by default (PFST_WINOGRAD=0 disables it)
    ok = Conv2dP(512, 512, 3, 1, 4, 4)                                # layer4 conv2: same-size dilated 3x3
    assert ok._wino_eligible()
    assert Conv2dP(2560, 512, 3, 1, 1, 1)._wino_eligible()            # head bottleneck
    assert Conv2dP(256, 256, 3, 1, 2, 2)._wino_eligible()             # layer3 conv2
    assert layers.WINO_MIN_CC <= layers.WINO_MIN_CC_WGRAD <= 512 * 512
    assert Conv2dP(128, 128, 3, 1, 1, 1)._wino_eligible() == (layers.ops.WINO_TILE == 4)   # layer2 conv2: pays off with F(4x4) only
    assert not Conv2dP(64, 64, 3, 1, 1, 1)._wino_eligible()           # layer1 conv2, transform-bound: stays direct
    assert not Conv2dP(512, 512, 3, 2, 1, 1)._wino_eligible()         # stride 2
    assert not Conv2dP(512, 512, 1)._wino_eligible()                  # 1x1
    assert not Conv2dP(512, 512, 3, 1, 0, 1)._wino_eligible()         # not a 'same' convolution
    assert not Conv2dP(2048, 2048, 3, 1, 12, 12, groups=2048)._wino_eligible()   # depthwise
    assert not Conv2dP(520, 512, 3, 1, 1, 1)._wino_eligible()         # Cin not a multiple of 16: generic kernel
