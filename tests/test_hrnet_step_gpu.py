"""HRNet (presets.baseline_model_cfg('hrnet') narrowed to tests/test_hrnet_cpu.py's NARROW extra and a 90-channel head) through the paths every
model takes, at 2 x 3 x 64 x 64 (branch grids 16 / 8 / 4 / 2): a supervised train_step (finite loss, a non-zero gradient in every parameter, a
bit-identical gradient arena from two deterministic-mode steps), one PFGST step with PFGSTLoss(downscale=None) -- the loss reads the head's
features on the stride-4 grid they share with the logits; downscale=0.5 stays refused --, and a checkpoint that reloads key for key the way
tools/test.py loads it, with inference_segmentor returning a label map of the image size in 'whole' and 'slide' mode; tools/test.py itself
evaluates such a checkpoint; and the step behind the data-parallel reducer in a single-rank RCCL group (PFST_DDP_FORCE=1, read at import: a
spawned process, as tests/test_supervised_gpu.py does): HRNet records no stage markers, so the heads go at their marker and the reducer's final
flush carries the whole backbone -- every bucket holds final values and the arena equals the non-distributed step's bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SGD = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
SIZE = 64


def narrow_cfg():
    from pfst_amd.presets import baseline_model_cfg
    from test_hrnet_cpu import NARROW
    cfg = baseline_model_cfg('hrnet', 6, 3)
    cfg['backbone']['extra'] = NARROW
    cfg['decode_head'].update(in_channels=[6, 12, 24, 48], channels=90)
    return cfg


def build(seed=3):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(narrow_cfg())
    model.cuda()
    return model, build_optimizer(model, dict(SGD))


def sup_batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return {k: v for k, v in synth_batch(2, SIZE, 6, seed=seed).items() if not k.startswith('target_')}


def test_supervised_step_is_deterministic_and_reaches_every_parameter():
    from pfst_amd import hip_ops
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        grads = []
        for _ in range(2):
            model, opt = build()
            out = model.train_step(to_dev(sup_batch(), DEV), opt)
            torch.cuda.synchronize()
            lv = out['log_vars']
            assert list(lv) == ['decode.loss_ce', 'decode.acc_seg', 'loss']
            assert all(np.isfinite(v) for v in lv.values()) and lv['loss'] > 0
            arena = model.param_arena
            grads.append(arena.grad.clone())
        assert bool(torch.isfinite(grads[0]).all())
        parts = dict(backbone=0, decode_head=0)
        for name in arena.names:
            assert float(arena.view(grads[0], name).abs().max()) > 0, f'{name}: zero gradient'
            parts[name.split('.')[0]] += 1
        assert parts['decode_head'] == 2 + 3 and parts['backbone'] == len(list(model.backbone.parameters())), parts
        assert torch.equal(grads[0], grads[1]), 'deterministic mode: two runs differ'
    finally:
        hip_ops.set_deterministic(was)


def test_pfgst_step_reads_the_stride_4_features():
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import UDA
    from pfst_amd.synthetic import synth_batch
    cfg = uda_cfg(threshold=0.2)
    cfg['model'] = narrow_cfg()
    cfg['aux_losses'][0]['downscale'] = None          # logits and decoded features share the stride-4 grid
    torch.manual_seed(5)
    model = UDA.build(cfg)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    handed = []
    h2 = model.aux_losses[0].register_forward_pre_hook(lambda m, a: handed.append(a[0]['x_src'].data))
    try:
        out = model.train_step(to_dev(synth_batch(2, SIZE, 6, seed=1234), DEV), opt)
        torch.cuda.synchronize()
    finally:
        h2.remove()
    assert len(handed) == 1 and tuple(handed[0].shape) == (2, 90, SIZE // 4, SIZE // 4)
    lv = out['log_vars']
    assert all(np.isfinite(v) for v in lv.values()), lv
    assert {'decode.loss_ce', 'mix.decode.loss_ce', 'loss_sim_pos'} <= set(lv) and any(k.startswith('loss_src_pos') for k in lv), list(lv)
    cfg['aux_losses'][0]['downscale'] = 0.5
    model = UDA.build(cfg)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    with pytest.raises(NotImplementedError, match='feature grid'):
        model.train_step(to_dev(synth_batch(2, SIZE, 6, seed=1234), DEV), opt)


@pytest.mark.parametrize('mode', ['whole', 'slide'])
def test_checkpoint_reloads_and_inference_returns_a_label_map(mode, tmp_path):
    from pfst_amd.apis import inference_segmentor, init_segmentor
    from pfst_amd.config import Config
    model, _ = build(seed=11)
    path = str(tmp_path / 'hrnet.pth')
    torch.save(dict(state_dict=model.state_dict(), meta=dict(CLASSES=None)), path)
    sd = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    assert {k.split('.')[0] for k in sd} == {'backbone', 'decode_head'}
    model_cfg = narrow_cfg()
    model_cfg['test_cfg'] = dict(mode='slide', crop_size=(96, 96), stride=(64, 64)) if mode == 'slide' else dict(mode='whole')
    test_pl = [dict(type='LoadImageFromFile'),
               dict(type='MultiScaleFlipAug', img_scale=(200, 160), flip=False,
                    transforms=[dict(type='Resize', keep_ratio=True), dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                                dict(type='Collect', keys=['img'])])]
    torch.manual_seed(12)
    other = init_segmentor(Config(dict(model=model_cfg, data=dict(test=dict(type='ISPRSDataset', pipeline=test_pl)))), path, 'cuda:0')
    assert list(other.state_dict()) == list(sd)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in other.state_dict().items()), 'the checkpoint reloads key for key'
    img = np.random.default_rng(0).integers(0, 256, (160, 200, 3), dtype=np.uint8)          # 160 x 200: grids that are no powers of two apart
    res = inference_segmentor(other, img)
    assert isinstance(res, list) and res[0].shape == (160, 200) and res[0].dtype == np.uint8 and int(res[0].max()) < 6


def _rccl_worker(rank, world, port, outdir):
    """one deterministic supervised step in a single-rank RCCL group with the exchange forced on, overlap on, buckets small enough for the heads"""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      PFST_DDP_FORCE='1', PFST_DDP_OVERLAP='1', PFST_DDP_BUCKET_MB='0.001')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    from pfst_amd import dist as pdist
    from pfst_amd import hip_ops, layers
    assert pdist.is_distributed() and pdist.OVERLAP_ALLREDUCE
    hip_ops.set_deterministic(True)
    snaps, markers = [], []
    launch, ready = pdist.GradReducer._launch, pdist.GradReducer.ready

    def recording_launch(self, lo, hi):
        if hi > lo:
            layers.join_side_stream()
            snaps.append((lo, hi, self.flat[lo:hi].clone()))
        return launch(self, lo, hi)

    def recording_ready(self, offset):
        markers.append(int(offset))
        return ready(self, offset)
    pdist.GradReducer._launch, pdist.GradReducer.ready = recording_launch, recording_ready
    model, opt = build()
    out = model.train_step(to_dev(sup_batch(), DEV), opt)
    torch.cuda.synchronize()
    arena = model.param_arena
    grad = arena.grad.clone().cpu()
    cut = arena.offsets[next(n for n in arena.names if not n.startswith('backbone.'))]
    torch.save(dict(ok=all(bool(torch.equal(s.cpu(), grad[lo:hi])) for lo, hi, s in snaps), ranges=[(lo, hi) for lo, hi, _ in snaps],
                    markers=markers, cut=cut, numel=grad.numel(), grad=grad, log=out['log_vars']), os.path.join(outdir, 'rccl_hrnet.pt'))
    dist.destroy_process_group()


def test_reducer_step_equals_the_non_distributed_one(tmp_path):
    from pfst_amd import hip_ops
    port = 29900 + (os.getpid() % 1000)
    mp.spawn(_rccl_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    res = torch.load(tmp_path / 'rccl_hrnet.pt', weights_only=False)
    # the one marker is 'heads'; its tail goes at once, the final flush carries [0, cut): the whole backbone, nothing twice, nothing left out
    assert res['markers'] == [res['cut']], res['markers']
    assert res['ranges'] == [(res['cut'], res['numel']), (0, res['cut'])], res['ranges']
    assert res['ok'], 'a gradient range was written after the reducer took it'
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        model, opt = build()
        out = model.train_step(to_dev(sup_batch(), DEV), opt)
        torch.cuda.synchronize()
        plain = model.param_arena.grad.clone().cpu()
    finally:
        hip_ops.set_deterministic(was)
    assert float(plain.abs().max()) > 0 and torch.equal(res['grad'], plain), 'the reducer step and the non-distributed step differ'
    assert list(res['log']) == list(out['log_vars'])


def test_the_test_tool_evaluates_a_checkpoint(tmp_path):
    """tools/test.py on a saved HRNet checkpoint and a small tile folder: the keys load (a missing key ends the tool) and the evaluation runs;
    a checkpoint short of a backbone key is refused"""
    import sys
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    import test as test_cli
    from test_data_pipeline_cpu import TEST, _tile
    model, _ = build(seed=11)
    torch.save(dict(state_dict=model.state_dict(), meta=dict(CLASSES=None)), tmp_path / 'hrnet.pth')
    os.makedirs(tmp_path / 'img'), os.makedirs(tmp_path / 'ann')
    for i in range(2):
        img, seg = _tile(40 + i, 96)
        Image.fromarray(img).save(tmp_path / 'img' / f't{i}.png')
        Image.fromarray(seg).save(tmp_path / 'ann' / f't{i}.png')
    ds = dict(type='ISPRSDataset', data_root=str(tmp_path), img_dir='img', ann_dir='ann', gt_seg_map_loader_cfg=dict(reduce_zero_label=True),
              pipeline=[TEST[0], dict(TEST[1], img_scale=(96, 96))])
    (tmp_path / 'cfg.py').write_text('model = %r\ndata = %r\n' % (narrow_cfg(), dict(test=ds, val=ds)))
    res = test_cli.main([str(tmp_path / 'cfg.py'), str(tmp_path / 'hrnet.pth'), '--eval', 'mIoU'])
    assert 0.0 <= res['mIoU'] <= 1.0 or 0.0 <= res['mIoU'] <= 100.0
    short = {k: v for k, v in model.state_dict().items() if k != 'backbone.stage4.1.fuse_layers.0.3.0.weight'}
    torch.save(dict(state_dict=short), tmp_path / 'short.pth')
    with pytest.raises(SystemExit, match='missing'):
        test_cli.main([str(tmp_path / 'cfg.py'), str(tmp_path / 'short.pth'), '--eval', 'mIoU'])
