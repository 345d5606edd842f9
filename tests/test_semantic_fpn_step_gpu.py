"""Semantic FPN (presets.baseline_model_cfg('fpn'): FPN neck + FPNHead on the stride-32 ResNetV1c) through the paths every model takes, on a
narrow backbone (stem 16, base 4; neck 32 channels, head 16) at 2 x 3 x 64 x 64 (level grids 16 / 8 / 4 / 2): a supervised train_step (log
keys, finite non-zero gradients in every parameter of backbone, neck and head, a bit-identical gradient arena under deterministic mode), one
PFGST step with PFGSTLoss(downscale=None) -- the loss reads the head's level sum itself, on the stride-4 grid it shares with the logits --,
inference_segmentor whole and slide, a checkpoint with `neck.*` keys loaded the way tools/test.py loads it, and the order of the
data-parallel marker 'heads': when it fires every gradient of neck and head is final."""
import numpy as np
import pytest
import torch

from helpers import to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SGD = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
SIZE = 64


def narrow_cfg(dropout=0.0):
    from pfst_amd.presets import baseline_model_cfg
    cfg = baseline_model_cfg('fpn', 6, 3, dropout=dropout)
    cfg['backbone'].update(stem_channels=16, base_channels=4)
    cfg['neck'].update(in_channels=[16, 32, 64, 128], out_channels=32)
    cfg['decode_head'].update(in_channels=[32] * 4, channels=16)
    return cfg


def build(seed=3):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(narrow_cfg())
    # (no init_weights(): its zero_init_residual starts every Bottleneck's last norm at 0, which makes the gradient of every other parameter of
    # the residual branches exactly zero at the first step -- the construction's Kaiming convolutions and unit norms leave every gradient live)
    model.cuda()
    return model, build_optimizer(model, dict(SGD))


def sup_batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return {k: v for k, v in synth_batch(2, SIZE, 6, seed=seed).items() if not k.startswith('target_')}


def test_supervised_step():
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
        parts = dict(backbone=0, neck=0, decode_head=0)
        for name in arena.names:
            assert float(arena.view(grads[0], name).abs().max()) > 0, f'{name}: zero gradient'
            parts[name.split('.')[0]] += 1
        assert parts['neck'] == 16 and parts['decode_head'] == 2 + 3 * 7 and parts['backbone'] > 100, parts
        first = next(n for n in arena.names if not n.startswith('backbone.'))
        assert first.startswith('neck.')                      # the 'heads' cut of the arena is the neck's first parameter
        assert torch.equal(grads[0], grads[1]), 'deterministic mode: two runs differ'
    finally:
        hip_ops.set_deterministic(was)


def test_heads_marker_fires_after_every_neck_and_head_gradient():
    from pfst_amd import hip_ops, layers
    from pfst_amd.engine import Tape
    model, _ = build()
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    model.repack_weights(need_dgrad=True)
    batch = to_dev(sup_batch(), DEV)
    mine = {n: p for n, p in model.named_parameters() if n.startswith(('neck.', 'decode_head.'))}
    fired, at_marker = [], {}

    def grad_ready(stage):
        fired.append(stage)
        if stage == 'heads':
            layers.join_side_stream()            # as dist.GradReducer does before it reads the arena: the weight gradients queued so far have landed
            at_marker.update({n: p.grad.clone() for n, p in mine.items()})
    tape = Tape()
    model.forward_train(batch['img'].contiguous(), batch['img_metas'], hip_ops.to_u8(batch['gt_semantic_seg'].contiguous()), tape=tape,
                        grad_ready=grad_ready)
    tape.backward()
    torch.cuda.synchronize()
    assert fired[0] == 'heads' and fired.count('heads') == 1, fired
    assert len(at_marker) == 16 + 2 + 3 * 7
    for n, p in mine.items():
        assert float(p.grad.abs().max()) > 0, n
        assert torch.equal(at_marker[n], p.grad), f'{n}: written after the marker "heads" fired'


def test_pfgst_step_reads_the_level_sum():
    import pfst_amd  # noqa: F401
    from pfst_amd import hip_ops
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
    seen, handed = [], []
    real = hip_ops.fpn_level_sum

    def level_sum(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    hip_ops.fpn_level_sum = level_sum
    h2 = model.aux_losses[0].register_forward_pre_hook(lambda m, a: handed.append(a[0]['x_src'].data))
    try:
        out = model.train_step(to_dev(synth_batch(2, SIZE, 6, seed=1234), DEV), opt)
        torch.cuda.synchronize()
    finally:
        hip_ops.fpn_level_sum = real
        h2.remove()
    assert len(handed) == 1 and len(seen) >= 2                     # the student's source and mixed passes (and the teacher's)
    assert any(handed[0].data_ptr() == s.data_ptr() for s in seen) and tuple(handed[0].shape) == (2, 16, SIZE // 4, SIZE // 4)
    lv = out['log_vars']
    assert all(np.isfinite(v) for v in lv.values()), lv
    assert {'decode.loss_ce', 'mix.decode.loss_ce', 'loss_sim_pos'} <= set(lv) and any(k.startswith('loss_src_pos') for k in lv), list(lv)
    # with the shipped downscale the feature grid would be finer than the loss grid: that stays refused
    cfg['aux_losses'][0]['downscale'] = 0.5
    model = UDA.build(cfg)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    with pytest.raises(NotImplementedError, match='feature grid'):
        model.train_step(to_dev(synth_batch(2, SIZE, 6, seed=1234), DEV), opt)


@pytest.mark.parametrize('mode', ['whole', 'slide'])
def test_inference_segmentor_returns_a_label_map_of_the_image_size(mode):
    from pfst_amd.apis import inference_segmentor, init_segmentor
    from pfst_amd.config import Config
    torch.manual_seed(7)
    model_cfg = narrow_cfg(dropout=0.1)
    model_cfg['test_cfg'] = dict(mode='slide', crop_size=(96, 96), stride=(64, 64)) if mode == 'slide' else dict(mode='whole')
    test_pl = [dict(type='LoadImageFromFile'),
               dict(type='MultiScaleFlipAug', img_scale=(200, 160), flip=False,
                    transforms=[dict(type='Resize', keep_ratio=True), dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                                dict(type='Collect', keys=['img'])])]
    model = init_segmentor(Config(dict(model=model_cfg, data=dict(test=dict(type='ISPRSDataset', pipeline=test_pl)))), None, 'cuda:0')
    img = np.random.default_rng(0).integers(0, 256, (160, 200, 3), dtype=np.uint8)          # level grids 40 x 50 / 20 x 25 / 10 x 13 / 5 x 7
    res = inference_segmentor(model, img)
    assert isinstance(res, list) and res[0].shape == (160, 200) and res[0].dtype == np.uint8 and int(res[0].max()) < 6


def test_checkpoint_with_neck_keys_loads_the_way_the_test_tool_loads_it(tmp_path):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_segmentor
    model, _ = build(seed=11)
    path = tmp_path / 'fpn.pth'
    torch.save(dict(state_dict=model.state_dict(), meta=dict(CLASSES=None)), path)
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    sd = ckpt.get('state_dict', ckpt)
    assert {k.split('.')[0] for k in sd} == {'backbone', 'neck', 'decode_head'}
    torch.manual_seed(12)
    cfg = narrow_cfg()
    cfg['pretrained'], cfg['train_cfg'] = None, None
    other = build_segmentor(cfg)
    res = other.load_state_dict(sd, strict=False)                      # tools/test.py: strict=False, then no key of the segmentor may be missing
    assert not [k for k in res.missing_keys if not k.endswith('num_batches_tracked')] and not res.unexpected_keys
    other.cuda()
    img = torch.randn(1, 3, 96, 80, generator=torch.Generator().manual_seed(1)).to(DEV)
    a, la = model.inference(img)
    b, lb = other.inference(img)
    assert torch.equal(a, b) and torch.equal(la, lb) and tuple(a.shape) == (1, 96, 80)
