"""DiceLoss and the decode head's loss lists, the parts that need no GPU: configs build, bad options fail loudly, class weights from a file,
the C ABI of the three Dice entry points, and a loss list through tools/train.py's --cfg-options."""
import json
import os
import sys

import pytest

import pfst_amd  # noqa: F401
from helpers import model_cfg
from pfst_amd.registry import build_head, build_loss, build_segmentor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
DICE = dict(type='DiceLoss', loss_weight=3.0)


def head_cfg(loss_decode, **over):
    cfg = dict(model_cfg()['auxiliary_head'], loss_decode=loss_decode)
    cfg.update(over)
    return cfg


def test_list_and_dict_configs_build():
    import torch.nn as nn
    from pfst_amd.models import CrossEntropyLoss, DiceLoss
    head = build_head(head_cfg([CE, DICE]))
    assert isinstance(head.loss_decode, nn.ModuleList) and [type(l) for l in head.loss_decode] == [CrossEntropyLoss, DiceLoss]
    assert [l.loss_name for l in head.loss_decode] == ['loss_ce', 'loss_dice'] and head.loss_decode[1].loss_weight == 3.0
    assert isinstance(build_head(head_cfg((CE, DICE))).loss_decode, nn.ModuleList)
    assert isinstance(build_head(head_cfg(DICE)).loss_decode, DiceLoss)
    assert isinstance(build_head(head_cfg(CE)).loss_decode, CrossEntropyLoss)             # today's form stays a bare module
    cfg = model_cfg()
    cfg['decode_head']['loss_decode'] = [CE, DICE]
    cfg['auxiliary_head']['loss_decode'] = [dict(CE, loss_weight=0.4), dict(DICE, loss_weight=1.2, loss_name='loss_dice_aux')]
    model = build_segmentor(cfg)
    assert model.auxiliary_head.loss_decode[1].loss_name == 'loss_dice_aux'
    assert not [k for k in model.state_dict() if 'loss_decode' in k], 'a loss list adds no parameters or buffers'
    # the reference's arguments and defaults
    d = build_loss(dict(type='DiceLoss'))
    assert (d.smooth, d.exponent, d.reduction, d.class_weight, d.loss_weight, d.ignore_index, d.loss_name) == (1, 2, 'mean', None, 1.0, 255, 'loss_dice')


def test_bad_options_fail_loudly():
    for reduction in ('mean', 'sum', 'none'):
        assert build_loss(dict(type='DiceLoss', reduction=reduction)).reduction == reduction
    with pytest.raises(ValueError, match='reduction'):
        build_loss(dict(type='DiceLoss', reduction='batchmean'))
    for exponent in (0.5, 0, -1, float('nan')):
        with pytest.raises(ValueError, match='exponent'):
            build_loss(dict(type='DiceLoss', exponent=exponent))
    assert build_loss(dict(type='DiceLoss', exponent=1)).exponent == 1 and build_loss(dict(type='DiceLoss', exponent=3.5)).exponent == 3.5
    with pytest.raises(KeyError):
        build_head(head_cfg([CE, dict(type='LovaszLoss')]))
    with pytest.raises(NotImplementedError):
        build_head(head_cfg([CE, DICE], sampler=dict(type='OHEMPixelSampler', thresh=0.7)))
    with pytest.raises(TypeError, match='loss_decode'):
        build_head(head_cfg('DiceLoss'))
    with pytest.raises(NotImplementedError, match='fused'):
        build_head(head_cfg([CE, dict(type='PFGSTLoss', top_k=3, dilation=2, kernel_size=3, weights={})]))


def test_class_weight_is_read_from_a_file(tmp_path):
    import numpy as np
    w = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
    np.save(tmp_path / 'w.npy', np.array(w))
    (tmp_path / 'w.json').write_text(json.dumps(w))
    assert build_loss(dict(type='DiceLoss', class_weight=str(tmp_path / 'w.npy'))).class_weight == w
    assert build_loss(dict(type='DiceLoss', class_weight=str(tmp_path / 'w.json'))).class_weight == w
    assert build_loss(dict(type='DiceLoss', class_weight=w)).class_weight == w
    with pytest.raises(TypeError, match='format'):
        build_loss(dict(type='DiceLoss', class_weight=str(tmp_path / 'w.txt')))


def test_the_three_entry_points_are_declared():
    """include/pfst_hip.h is what _lib.py binds from (parse_header): the three symbols, their argument counts and kinds, and the wrappers"""
    import ctypes
    import re
    from pfst_amd import _lib, hip_ops
    decls = _lib.parse_header()
    want = {'pfst_dice_upsample_fwd': 18, 'pfst_dice_finalize': 14, 'pfst_dice_upsample_bwd': 18}
    text = open(_lib.HEADER).read()
    src = open(os.path.join(ROOT, 'pfst_amd', 'csrc', 'dice_loss.hip')).read()
    for name, nargs in want.items():
        restype, args = decls[name]
        assert restype is ctypes.c_int and len(args) == nargs, (name, len(args))
        assert args[-1] == (ctypes.c_void_p, 'stream')
        # the definition's parameter list is the declaration's, token for token
        norm = lambda s: ' '.join(re.search(name + r'\s*\(([^)]*)\)', s).group(1).split())
        assert norm(text) == norm(src[src.index('extern "C" int ' + name):]), name
    kinds = dict((a, k) for k, a in decls['pfst_dice_finalize'][1])
    assert kinds['smooth'] is ctypes.c_double and kinds['N'] is ctypes.c_int and kinds['slab'] is ctypes.c_void_p
    assert decls['pfst_ce_upsample_fwd'][1][-1] == (ctypes.c_void_p, 'stream') and len(decls['pfst_ce_upsample_fwd'][1]) == 14   # unchanged
    assert len(decls['pfst_ce_upsample_bwd'][1]) == 16 and len(decls['pfst_ce_finalize'][1]) == 5
    for fn in ('dice_upsample_fwd', 'dice_finalize', 'dice_upsample_bwd'):
        assert callable(getattr(hip_ops, fn))
    from pfst_amd.build import NO_SLP, SOURCES
    assert 'dice_loss.hip' in SOURCES and 'dice_loss.hip' in NO_SLP


def test_wrappers_refuse_cpu_tensors_and_bad_exponents():
    import torch
    from pfst_amd import hip_ops
    with pytest.raises(RuntimeError, match='GPU only'):
        hip_ops.dice_upsample_fwd(torch.zeros(1, 2, 4, 4), torch.zeros(1, 16, 16, dtype=torch.uint8))


def test_cfg_options_with_a_loss_list_round_trip():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.registry import build_train_model
    name = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
    # values are Python literals (config.parse_cfg_options): dicts in braces
    losses = "[{'type':'CrossEntropyLoss','loss_weight':1.0},{'type':'DiceLoss','loss_weight':3.0,'class_weight':[1,1,1,1,2,1]}]"
    cfg = train_cli.load_cfg(train_cli.parse_args([name, '--supervised', '--cfg-options', 'model.decode_head.loss_decode=' + losses,
                                                   "model.auxiliary_head.loss_decode=[{'type':'CrossEntropyLoss','loss_weight':0.4},{'type':'DiceLoss','loss_weight':1.2}]"]))
    got = cfg.model['decode_head']['loss_decode']
    assert [dict(l) for l in got] == [dict(type='CrossEntropyLoss', loss_weight=1.0), dict(type='DiceLoss', loss_weight=3.0, class_weight=[1, 1, 1, 1, 2, 1])]
    model = build_train_model(cfg)
    assert [type(l).__name__ for l in model.decode_head.loss_decode] == ['CrossEntropyLoss', 'DiceLoss']
    assert model.decode_head.loss_decode[1].class_weight == [1, 1, 1, 1, 2, 1] and model.auxiliary_head.loss_decode[1].loss_weight == 1.2
    # the PFGST wrapper's student and teacher take the list as well
    cfg = train_cli.load_cfg(train_cli.parse_args([name, '--cfg-options', 'model.decode_head.loss_decode=' + losses]))
    uda = build_train_model(cfg)
    assert [type(l).__name__ for l in uda.get_model().decode_head.loss_decode] == ['CrossEntropyLoss', 'DiceLoss']
