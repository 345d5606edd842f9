"""CPU-side checks of the supervised training path: the SGD optimizer's construction and C ABI, the poly schedule of the reference's
schedule_40k.py, the plain (non-UDA) dataset path through build_dataset + build_loader, and the --supervised switch of tools/train.py."""
import ctypes
import os
import sys

import pytest
import torch

from test_data_loader_cpu import _first_batches, _folders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULE_40K = dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005),
                    lr_config=dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False), max_iters=40000)


def test_build_optimizer_sgd():
    from pfst_amd import optim
    model = torch.nn.Conv2d(3, 4, 3)
    opt = optim.build_optimizer(model, dict(SCHEDULE_40K['optimizer']))
    assert type(opt) is optim.SGD and isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert (g['lr'], g['momentum'], g['dampening'], g['weight_decay'], g['nesterov']) == (0.01, 0.9, 0.0, 0.0005, False)
    assert len(g['params']) == 2
    full = optim.build_optimizer(model, dict(type='SGD', lr=0.1, momentum=0.8, dampening=0.0, weight_decay=0.0, nesterov=True))
    assert full.param_groups[0]['nesterov'] is True
    with pytest.raises(NotImplementedError, match='paramwise_cfg'):
        optim.build_optimizer(model, dict(SCHEDULE_40K['optimizer'], paramwise_cfg=dict(custom_keys={'head': dict(lr_mult=10.)})))
    with pytest.raises(NotImplementedError):
        optim.build_optimizer(model, dict(type='Adam', lr=1e-3))
    # AdamW keeps its handling (a paramwise_cfg is dropped, as before)
    assert type(optim.build_optimizer(model, dict(type='AdamW', lr=6e-5, paramwise_cfg=dict()))) is optim.AdamW
    # the flat state travels through state_dict / load_state_dict
    sd = opt.state_dict()
    assert sd['pfst_flat'] == []
    opt2 = optim.build_optimizer(model, dict(SCHEDULE_40K['optimizer']))
    opt2.load_state_dict(sd)


def test_header_declares_and_library_exports_pfst_sgd_step():
    from pfst_amd import _lib
    decls = _lib.parse_header()
    assert 'pfst_sgd_step' in decls
    restype, args = decls['pfst_sgd_step']
    assert [a[1] for a in args] == ['p', 'g', 'buf', 'n', 'lr', 'momentum', 'dampening', 'weight_decay', 'nesterov', 'first_step',
                                    'grad_scale', 'stream']
    assert [a[0] for a in args] == [ctypes.c_void_p] * 3 + [ctypes.c_longlong] + [ctypes.c_float] * 4 + [ctypes.c_int] * 2 + \
        [ctypes.c_float, ctypes.c_void_p]
    L = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(L, 'pfst_sgd_step')
    # bad arguments are rejected on the host before any launch: null pointers, n = 0, a momentum without its buffer
    L = _lib.lib()
    assert L.pfst_sgd_step(None, None, None, 16, 0.1, 0.0, 0.0, 0.0, 0, 1, 1.0, None) == -1
    assert b'optim.hip' in L.pfst_last_error()
    x = ctypes.create_string_buffer(64)
    p = ctypes.cast(x, ctypes.c_void_p)
    assert L.pfst_sgd_step(p, p, None, 0, 0.1, 0.0, 0.0, 0.0, 0, 1, 1.0, None) == -1
    assert L.pfst_sgd_step(p, p, None, 4, 0.1, 0.9, 0.0, 0.0, 0, 1, 1.0, None) == -1
    assert L.pfst_sgd_step(p, p, p, 4, 0.1, 0.0, 0.0, 0.0, 0, 1, 1.0, None) == -1


def test_poly_lr_of_schedule_40k_through_the_runner():
    """mmcv PolyLrUpdaterHook: (base - min_lr) * (1 - it / max) ** power + min_lr, no warm-up -- through IterBasedRunner.current_lr, which is
    what sets param_groups[...]['lr'] before every step"""
    from pfst_amd.config import Config
    from pfst_amd.optim import build_optimizer
    from pfst_amd.runner import IterBasedRunner
    cfg = Config(dict(runner=dict(type='IterBasedRunner', max_iters=SCHEDULE_40K['max_iters']), lr_config=dict(SCHEDULE_40K['lr_config']),
                      optimizer=dict(SCHEDULE_40K['optimizer'])))
    model = torch.nn.Conv2d(3, 4, 3)
    runner = IterBasedRunner(model, build_optimizer(model, cfg.optimizer), cfg, None, log=lambda s: None)
    runner.iter = 0
    assert runner.current_lr() == [0.01]
    runner.iter = 40000
    assert abs(runner.current_lr()[0] - 1e-4) <= 1e-18
    runner.iter = 12345
    # the formula in float64 by another route than `**`: 0.0099 * exp(0.9 * log(0.691375)) + 0.0001
    want = float((torch.tensor(0.01, dtype=torch.float64) - 1e-4) * torch.exp(0.9 * torch.log(1 - torch.tensor(12345, dtype=torch.float64) / 40000))
                 + 1e-4)
    assert 1e-4 < want < 0.01
    assert abs(runner.current_lr()[0] - want) <= 1e-15


def _plain(cfg):
    """the reference's `source=` entry of pots_irrg2vaih_irrg.py moved up to data.train"""
    return dict(cfg['source'])


def test_plain_tile_folder_through_build_dataset_and_loader(tmp_path):
    from pfst_amd.data import TileFolder, UDADataset, build_dataset, build_loader
    uda_cfg = _folders(tmp_path)
    ds = build_dataset(_plain(uda_cfg))
    assert type(ds) is TileFolder and len(ds) == 4
    runs = [_first_batches(build_loader(ds, 2, device='cpu', seed=7, workers=0), 3) for _ in range(2)]
    for a, b in zip(*runs):
        assert set(a) == {'img', 'gt_semantic_seg', 'img_metas'}
        assert a['img'].shape == (2, 3, 512, 512) and a['gt_semantic_seg'].shape == (2, 1, 512, 512)
        assert len(a['img_metas']) == 2 and all('filename' in m for m in a['img_metas'])
        assert torch.equal(a['img'], b['img']) and torch.equal(a['gt_semantic_seg'], b['gt_semantic_seg'])
        assert [m['filename'] for m in a['img_metas']] == [m['filename'] for m in b['img_metas']]
    other = _first_batches(build_loader(ds, 2, device='cpu', seed=8, workers=0), 1)
    assert not torch.equal(other[0]['img'], runs[0][0]['img'])
    # a UDA config still pairs source and target: every target-side key is there
    uda = build_dataset(uda_cfg)
    assert type(uda) is UDADataset
    b = _first_batches(build_loader(uda, 2, device='cpu', seed=7, workers=0), 1)[0]
    assert set(b) == {'img', 'gt_semantic_seg', 'img_metas', 'target_img', 'target_img_strong_aug', 'target_img_metas'}
    assert len(b['target_img_metas']) == 2
    # the inline collation as well
    from pfst_amd.data import collate
    assert set(collate([ds[0], ds[1]], 'cpu')) == {'img', 'gt_semantic_seg', 'img_metas'}
    assert 'target_img_metas' in collate([uda[0], uda[1]], 'cpu')
    with pytest.raises(KeyError):
        build_dataset(dict(uda_cfg, type='ISPRSDataset'))              # source / target entries under a non-pairing type


def test_supervised_switch_on_a_preset():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.registry import build_train_model
    name = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
    cfg = train_cli.load_cfg(train_cli.parse_args([name]))
    assert 'uda' in cfg and cfg.optimizer['type'] == 'AdamW'
    cfg = train_cli.load_cfg(train_cli.parse_args([name, '--supervised']))
    assert 'uda' not in cfg
    assert dict(cfg.optimizer) == SCHEDULE_40K['optimizer'] and dict(cfg.lr_config) == SCHEDULE_40K['lr_config']
    model = build_train_model(cfg)
    assert type(model).__name__ == 'EncoderDecoder' and callable(getattr(model, 'train_step'))
    assert list(model.state_dict())[0].startswith('backbone.')          # bare keys: tools/test.py needs no key revision
    with pytest.raises(NotImplementedError, match='grad_clip'):
        train_cli.load_cfg(train_cli.parse_args([name, '--supervised', '--cfg-options', 'optimizer_config.grad_clip={"max_norm":1}']))
    # grad_clip = None is mmcv's "no clipping"
    train_cli.load_cfg(train_cli.parse_args([name, '--supervised', '--cfg-options', 'optimizer_config.grad_clip=None']))


def test_train_step_refuses_a_uda_batch():
    """extra keys a UDA loader would add are an error, before anything touches the device"""
    import pfst_amd  # noqa: F401
    from helpers import model_cfg
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import synth_batch
    model = build_segmentor(model_cfg())
    with pytest.raises(KeyError, match='target_img'):
        model.train_step(synth_batch(2, 64, 6), None)
    with pytest.raises(KeyError, match='gt_semantic_seg'):
        model.train_step(dict(img=torch.zeros(2, 3, 64, 64), img_metas=[{}, {}]), None)
