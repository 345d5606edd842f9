"""HRNet without a GPU: the registry builds it from fcn_hr18.py's `extra` and from the preset, the module tree carries the reference's keys
(tests/golden/hrnet.npz holds the key list and shapes of the reference's own state_dict), the refusals are loud, FCNHead takes level lists with
'resize_concat' and nothing else, the new entry points are in the C ABI, and `--model hrnet` parses."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import pfst_amd  # noqa: F401
from pfst_amd import _lib
from pfst_amd.presets import BASELINE_KINDS, baseline_model_cfg
from pfst_amd.registry import build_backbone, build_head, build_segmentor

HERE = os.path.dirname(os.path.abspath(__file__))
NORM = dict(type='BN', requires_grad=True)
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
HR18 = dict(stage1=dict(num_modules=1, num_branches=1, block='BOTTLENECK', num_blocks=(4,), num_channels=(64,)),
            stage2=dict(num_modules=1, num_branches=2, block='BASIC', num_blocks=(4, 4), num_channels=(18, 36)),
            stage3=dict(num_modules=4, num_branches=3, block='BASIC', num_blocks=(4, 4, 4), num_channels=(18, 36, 72)),
            stage4=dict(num_modules=3, num_branches=4, block='BASIC', num_blocks=(4, 4, 4, 4), num_channels=(18, 36, 72, 144)))
NARROW = dict(stage1=dict(num_modules=1, num_branches=1, block='BOTTLENECK', num_blocks=(1,), num_channels=(8,)),
              stage2=dict(num_modules=1, num_branches=2, block='BASIC', num_blocks=(1, 1), num_channels=(6, 12)),
              stage3=dict(num_modules=1, num_branches=3, block='BASIC', num_blocks=(1, 1, 1), num_channels=(6, 12, 24)),
              stage4=dict(num_modules=2, num_branches=4, block='BASIC', num_blocks=(1, 1, 1, 1), num_channels=(6, 12, 24, 48)))
HEAD = dict(type='FCNHead', in_channels=[6, 12, 24, 48], in_index=[0, 1, 2, 3], input_transform='resize_concat', channels=90, kernel_size=1,
            num_convs=1, concat_input=False, dropout_ratio=-1, num_classes=6, norm_cfg=NORM, align_corners=False, loss_decode=CE)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'hrnet.npz'))


def keys_and_shapes(module):
    sd = module.state_dict()
    return list(sd), [','.join(str(d) for d in v.shape) for v in sd.values()]


def test_registry_builds_hr18_and_the_presets():
    net = build_backbone(dict(type='HRNet', extra=HR18, norm_cfg=NORM))
    assert [len(getattr(net, f'stage{s}')) for s in (2, 3, 4)] == [1, 4, 3]
    assert tuple(net.stage4[2].fuse_layers[3][0][2][0].weight.shape) == (144, 18, 3, 3)
    assert tuple(net.stage4[0].fuse_layers[0][3][0].weight.shape) == (18, 144, 1, 1)
    assert 'hrnet' in BASELINE_KINDS
    for width, widths in ((18, [18, 36, 72, 144]), (48, [48, 96, 192, 384])):
        cfg = baseline_model_cfg('hrnet', 6, 4, width=width)
        assert 'auxiliary_head' not in cfg and cfg['decode_head']['channels'] == sum(widths) and cfg['decode_head']['dropout_ratio'] == -1
        model = build_segmentor(cfg)
        assert model.auxiliary_head is None and model.neck is None
        assert tuple(model.backbone.conv1.weight.shape) == (64, 4, 3, 3)
        assert tuple(model.decode_head.convs[0].conv.weight.shape) == (sum(widths), sum(widths), 1, 1)
        assert model.decode_head.in_channels == sum(widths) and model.decode_head.level_channels == widths
        assert model.decode_head.dropout_mask(2, True) is None, 'a negative dropout_ratio means no dropout'
        assert [m.in_channels for m in model.backbone.stage4] == [widths] * 3


def test_state_dict_keys_and_shapes_are_the_references(golden):
    net = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM))
    keys, shapes = keys_and_shapes(net)
    assert keys == [str(k) for k in golden['backbone|keys']]
    assert shapes == [str(s) for s in golden['backbone|shapes']]
    keys, shapes = keys_and_shapes(build_head(dict(HEAD)))
    assert keys == [str(k) for k in golden['head|keys']]
    assert shapes == [str(s) for s in golden['head|shapes']]


def test_none_entries_sit_where_the_reference_has_them():
    net = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM))
    # hrnet.py:434-479: a transition entry exists where the width changes or a branch is new
    assert [t is None for t in net.transition1] == [False, False]              # 32 -> 6 (3x3), 32 -> 12 (stride 2)
    assert [t is None for t in net.transition2] == [True, True, False]
    assert [t is None for t in net.transition3] == [True, True, True, False]
    assert len(net.transition2[2]) == 1 and len(net.transition2[2][0]) == 3    # Sequential(Sequential(conv, bn, relu))
    for mod, B in ((net.stage2[0], 2), (net.stage3[0], 3), (net.stage4[0], 4), (net.stage4[1], 4)):
        assert len(mod.fuse_layers) == B
        for i in range(B):
            assert [mod.fuse_layers[i][j] is None for j in range(B)] == [j == i for j in range(B)]
            for j in range(B):
                fl = mod.fuse_layers[i][j]
                if j > i:
                    assert len(fl) == 3 and not list(fl[2].parameters()) and fl[0].stride == 1
                elif j < i:
                    assert len(fl) == i - j and [len(s) for s in fl] == [3] * (i - j - 1) + [2] and all(s[0].stride == 2 for s in fl)


def test_multiscale_output_false_builds_one_output():
    net = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM, multiscale_output=False))
    assert len(net.stage4[0].fuse_layers) == 4 and len(net.stage4[1].fuse_layers) == 1
    assert [net.stage4[1].fuse_layers[0][j] is None for j in range(4)] == [True, False, False, False]
    assert len(net.stage3[0].fuse_layers) == 3


def test_init_weights():
    import torch
    net = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM, zero_init_residual=True))
    net.init_weights()
    assert float(net.stage4[1].branches[3][0].bn2.weight.data.abs().max()) == 0.0 and float(net.layer1[0].bn3.weight.data.abs().max()) == 0.0
    assert float(net.stage4[1].branches[3][0].bn1.weight.data.min()) == 1.0 and float(net.bn1.bias.data.abs().max()) == 0.0
    assert float(net.stage2[0].fuse_layers[1][0][0][1].weight.data.min()) == 1.0
    plain = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM))
    plain.init_weights()
    assert float(plain.layer1[0].bn3.weight.data.min()) == 1.0
    assert bool(torch.isfinite(plain.conv2.weight.data).all()) and float(plain.conv2.weight.data.std()) > 0


def test_refusals_are_loud(tmp_path):
    import torch
    for bad in (dict(norm_eval=True), dict(with_cp=True), dict(frozen_stages=0), dict(conv_cfg=dict(type='Conv2d')),
                dict(norm_cfg=dict(type='SyncBN', requires_grad=True)), dict(norm_cfg=dict(type='GN', num_groups=2))):
        with pytest.raises(NotImplementedError):
            build_backbone(dict(dict(type='HRNet', extra=NARROW, norm_cfg=NORM), **bad))
    with pytest.raises(AssertionError):
        build_backbone(dict(type='HRNet', extra={k: v for k, v in NARROW.items() if k != 'stage4'}, norm_cfg=NORM))
    with pytest.raises(AssertionError):
        build_backbone(dict(type='HRNet', extra=dict(NARROW, stage3=dict(NARROW['stage3'], num_blocks=(1, 1))), norm_cfg=NORM))
    with pytest.raises(TypeError):
        build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM, pretrained=3))
    net = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM, pretrained='open-mmlab://msra/hrnetv2_w18'))
    with pytest.raises(FileNotFoundError):
        net.init_weights()
    # a local file is loaded by key, with or without the `backbone.` prefix
    src = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM))
    path = str(tmp_path / 'hr.pth')
    torch.save(dict(state_dict={'backbone.' + k: v for k, v in src.state_dict().items()}), path)
    net = build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM, pretrained=path))
    net.init_weights()
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), src.state_dict().values()))


def test_fcn_head_takes_level_lists_with_resize_concat_and_nothing_else():
    head = build_head(dict(HEAD))
    assert head.in_channels == 90 and head.level_channels == [6, 12, 24, 48] and head.in_index == [0, 1, 2, 3]
    assert tuple(head.convs[0].conv.weight.shape) == (90, 90, 1, 1) and not hasattr(head, 'conv_cat')
    refused = [dict(HEAD, input_transform='multiple_select'), dict(HEAD, in_channels=90, in_index=0), dict(HEAD, in_index=[0, 1, 2]),
               dict(HEAD, in_index=0), dict(HEAD, type='PSPHead'), dict(HEAD, type='ASPPHead'),
               dict(HEAD, type='UPerHead', kernel_size=None, num_convs=None, concat_input=None)]
    for cfg in refused:
        cfg = {k: v for k, v in cfg.items() if v is not None}
        if cfg['type'] != 'FCNHead':
            for k in ('kernel_size', 'num_convs', 'concat_input'):
                cfg.pop(k, None)
        with pytest.raises(NotImplementedError, match='outside the PFST path'):
            build_head(cfg)


def test_new_entry_points_are_in_the_c_abi():
    decls = _lib.parse_header()
    assert os.path.exists(_lib.LIB_PATH), 'run python -m pfst_amd.build'
    L = ctypes.CDLL(_lib.LIB_PATH)
    want = dict(pfst_hr_fuse=14, pfst_hr_fuse_bwd=17, pfst_hr_fuse_route=9)
    for name, n in want.items():
        assert name in decls and hasattr(L, name), name
        assert len(decls[name][1]) == n, (name, len(decls[name][1]))
    _lib.lib()
    for name, n in want.items():
        if name.endswith('_route'):
            continue
        with pytest.raises(TypeError, match='takes'):
            _lib.call(name, *([0] * (n + 1)))
        with pytest.raises(TypeError, match='takes'):
            _lib.call(name, *([0] * (n - 1)))
    # bad arguments are rejected on the host before any launch
    lib = _lib.lib()
    assert lib.pfst_hr_fuse(None, None, None, None, None, 2, None, 0, 1, 1, 4, 4, None, None) == -1
    assert b'hrnet.hip' in lib.pfst_last_error()
    assert lib.pfst_hr_fuse_bwd(None, 0, None, 0, None, 0, None, None, None, None, None, 0, 1, 1, 4, 4, None) == -1
    assert lib.pfst_hr_fuse_route(None, None, None, None, 2, None, 0, 4, 4) == 0
    from pfst_amd import build
    assert 'hrnet.hip' in build.SOURCES and 'hrnet.hip' in build.NO_SLP


def test_train_cli_parses_the_model():
    spec = importlib.util.spec_from_file_location('train_cli', os.path.join(HERE, '..', 'tools', 'train.py'))
    train_cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train_cli)
    preset = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
    args = train_cli.parse_args([preset, '--supervised', '--model', 'hrnet'])
    assert args.model == 'hrnet'
    cfg = train_cli.load_cfg(args)
    assert cfg.model['backbone']['type'] == 'HRNet' and cfg.model['decode_head']['input_transform'] == 'resize_concat'
    assert cfg.model['decode_head']['num_classes'] == 6 and 'auxiliary_head' not in cfg.model
    with pytest.raises(ValueError, match='--supervised'):
        train_cli.load_cfg(train_cli.parse_args([preset, '--model', 'hrnet']))
