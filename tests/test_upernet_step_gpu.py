"""UPerNet (presets.baseline_model_cfg('upernet'): UPerHead on the stride-32 ResNetV1c-50) through the paths every model takes: a supervised
train_step at 2 x 128^2 (log keys, finite non-zero gradients in every decode-head parameter, a bit-identical gradient arena under
deterministic mode), one PFGST step with PFGSTLoss(downscale=None) -- the loss reads the head's fpn_bottleneck output itself, on the
stride-4 grid it shares with the logits --, and inference_segmentor on a 160 x 200 image (level grids 40 x 50 / 20 x 25 / 10 x 13 / 5 x 7),
whole and slide."""
import numpy as np
import pytest
import torch

from helpers import to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SGD = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def build(seed=3):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import build_segmentor
    torch.manual_seed(seed)
    model = build_segmentor(baseline_model_cfg('upernet', 6, 3, dropout=0.0))
    model.init_weights()
    model.cuda()
    return model, build_optimizer(model, dict(SGD))


def sup_batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return {k: v for k, v in synth_batch(2, 128, 6, seed=seed).items() if not k.startswith('target_')}


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
            assert list(lv) == ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss']
            assert all(np.isfinite(v) for v in lv.values()) and lv['loss'] > 0
            arena = model.param_arena
            grads.append(arena.grad.clone())
        assert bool(torch.isfinite(grads[0]).all())
        seen = 0
        for name in arena.names:
            if name.startswith('decode_head.'):
                g = arena.view(grads[0], name)
                assert float(g.abs().max()) > 0, f'{name}: zero gradient'
                seen += 1
        assert seen == 2 + 3 * (4 + 1 + 3 + 3 + 1)          # conv_seg, and (conv weight, BN weight, BN bias) of 12 ConvModules
        assert torch.equal(grads[0], grads[1]), 'deterministic mode: two runs differ'
    finally:
        hip_ops.set_deterministic(was)


def test_pfgst_step_reads_the_fpn_bottleneck_output():
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import baseline_model_cfg
    from pfst_amd.registry import UDA
    from pfst_amd.synthetic import synth_batch
    cfg = uda_cfg(threshold=0.2)
    cfg['model'] = baseline_model_cfg('upernet', 6, 3, dropout=0.0)
    cfg['aux_losses'][0]['downscale'] = None          # logits and decoded features share the stride-4 grid
    torch.manual_seed(5)
    model = UDA.build(cfg)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    student = model.get_model() if hasattr(model, 'get_model') else model.model
    seen, handed = [], []
    h1 = student.decode_head.fpn_bottleneck.register_forward_hook(lambda m, a, out: seen.append(out.data))
    h2 = model.aux_losses[0].register_forward_pre_hook(lambda m, a: handed.append(a[0]['x_src'].data))
    try:
        out = model.train_step(to_dev(synth_batch(2, 128, 6, seed=1234), DEV), opt)
        torch.cuda.synchronize()
    finally:
        h1.remove(), h2.remove()
    assert len(handed) == 1 and len(seen) == 2                     # the source pass and the mixed pass of the student
    assert handed[0].data_ptr() == seen[0].data_ptr() and torch.equal(handed[0], seen[0]) and tuple(handed[0].shape) == (2, 512, 32, 32)
    lv = out['log_vars']
    assert all(np.isfinite(v) for v in lv.values()), lv
    assert {'decode.loss_ce', 'mix.decode.loss_ce', 'loss_sim_pos'} <= set(lv) and any(k.startswith('loss_src_pos') for k in lv), list(lv)
    # with the shipped downscale the feature grid would be finer than the loss grid: that stays refused
    cfg['aux_losses'][0]['downscale'] = 0.5
    model = UDA.build(cfg)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    with pytest.raises(NotImplementedError, match='feature grid'):
        model.train_step(to_dev(synth_batch(2, 128, 6, seed=1234), DEV), opt)


@pytest.mark.parametrize('mode', ['whole', 'slide'])
def test_inference_segmentor_returns_a_label_map_of_the_image_size(mode):
    from pfst_amd.apis import inference_segmentor, init_segmentor
    from pfst_amd.config import Config
    from pfst_amd.presets import baseline_model_cfg
    torch.manual_seed(7)
    model_cfg = baseline_model_cfg('upernet', 6, 3)
    model_cfg['test_cfg'] = dict(mode='slide', crop_size=(96, 96), stride=(64, 64)) if mode == 'slide' else dict(mode='whole')
    test_pl = [dict(type='LoadImageFromFile'),
               dict(type='MultiScaleFlipAug', img_scale=(200, 160), flip=False,
                    transforms=[dict(type='Resize', keep_ratio=True), dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                                dict(type='Collect', keys=['img'])])]
    model = init_segmentor(Config(dict(model=model_cfg, data=dict(test=dict(type='ISPRSDataset', pipeline=test_pl)))), None, 'cuda:0')
    img = np.random.default_rng(0).integers(0, 256, (160, 200, 3), dtype=np.uint8)
    res = inference_segmentor(model, img)
    assert isinstance(res, list) and res[0].shape == (160, 200) and res[0].dtype == np.uint8 and int(res[0].max()) < 6
