"""Whole-scene prediction on the GPU: each of the four scene kernels bit for bit against the chain of existing kernels / the
NumPy expression it replaces, predict_scene against the existing slide path, and tools/predict.py end to end.  The sizes are the smallest
at which each path can go wrong: width 203 (4-pixel tails, rows that start off a 16-byte boundary), windows shifted back to the odd offsets
104 / 107 (unaligned 12-byte reads), batches of 4, 4, 1 (they straddle the rows of the 3 x 3 window grid; a remainder batch), an 80-row
scene under a 96-row window (clipped windows, 20 x 24 logits), 19 and 40 classes (class chunks; the register and the generic finalize)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
CROP, STRIDE = (96, 96), (64, 64)


def _scene(seed, h=200, w=203):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _batches(wins, per):
    return [wins[i:i + per] for i in range(0, len(wins), per)]


# ---------------------------------------------------------------------------------------------------------------- 1. scene_windows
@pytest.mark.parametrize('to_rgb', [True, False])
@pytest.mark.parametrize('hw', [(200, 203), (80, 200), (97, 101)])
def test_scene_windows_equal_pipeline_normalize(hw, to_rgb):
    from pfst_amd import hip_ops as ops
    from pfst_amd import pipeline
    from pfst_amd.scene import window_grid
    scene = _scene(3, *hw)
    crop = (96, 96) if hw != (97, 101) else (95, 94)                 # last case: a window width that is no multiple of 4 (scalar stores)
    wins, size = window_grid(hw[0], hw[1], crop, STRIDE)
    assert len(wins) == {(200, 203): 9, (80, 200): 3, (97, 101): 4}[hw]
    dev = torch.from_numpy(scene).cuda()
    for batch in _batches(wins, 4):
        got = ops.scene_windows(dev, batch, size, NORM['mean'], NORM['std'], to_rgb).cpu()
        assert tuple(got.shape) == (len(batch), 3) + size
        for b, (y1, x1) in enumerate(batch):
            want = pipeline.normalize(np.ascontiguousarray(scene[y1:y1 + size[0], x1:x1 + size[1]]), NORM['mean'], NORM['std'], to_rgb)
            assert torch.equal(got[b], torch.from_numpy(want.transpose(2, 0, 1).copy())), (batch[b], to_rgb)


# ---------------------------------------------------------------------------------------------------------------- 2. scene_accumulate_
_chain_cache = {}


def _chain(hw, C):
    """random low-resolution logits of every window of the scene and what the existing chain makes of them, computed once per case:
    resize_bilinear + window_accumulate_ window by window -> (wins, size, logits, sums, count), then left unchanged"""
    from pfst_amd import hip_ops as ops
    from pfst_amd.scene import window_grid
    key = (hw, C)
    if key not in _chain_cache:
        H, W = hw
        wins, size = window_grid(H, W, CROP, STRIDE)
        logits = (3 * torch.randn(len(wins), C, size[0] // 4, size[1] // 4, generator=torch.Generator().manual_seed(7))).cuda()
        preds, count = torch.zeros(1, C, H, W, device='cuda'), torch.zeros(1, 1, H, W, device='cuda')
        for i, (y1, x1) in enumerate(wins):
            ops.window_accumulate_(preds, count, ops.resize_bilinear(logits[i:i + 1], size), y1, x1)
        _chain_cache[key] = (wins, size, logits, preds, count)
    return _chain_cache[key]


@pytest.mark.parametrize('hw,C,per', [((200, 203), 6, 4), ((200, 203), 6, 1), ((200, 203), 6, 9), ((80, 200), 6, 4), ((200, 203), 19, 4),
                                      ((200, 204), 6, 4)])
def test_scene_accumulate_equals_resize_plus_window_accumulate(hw, C, per):
    """batches of `per` consecutive windows (4: 4 + 4 + 1, straddling the grid's rows); (200, 204): the 16-byte path, W % 4 == 0"""
    from pfst_amd import hip_ops as ops
    wins, size, logits, preds, _ = _chain(hw, C)
    assert tuple(logits.shape[2:]) == {(200, 203): (24, 24), (200, 204): (24, 24), (80, 200): (20, 24)}[hw]
    sums = torch.zeros(C, hw[0], hw[1], device='cuda')
    for i in range(0, len(wins), per):
        ops.scene_accumulate_(sums, logits[i:i + per], wins[i:i + per], size)
    assert torch.equal(sums, preds[0])


def test_scene_accumulate_leaves_uncovered_pixels_alone():
    """one batch of two windows at opposite corners: inside their bounding box only the covered pixels change (NaNs elsewhere survive)"""
    from pfst_amd import hip_ops as ops
    logits = torch.randn(2, 6, 10, 10, generator=torch.Generator().manual_seed(2)).cuda()
    wins, size = [(0, 0), (23, 27)], (40, 40)
    sums = torch.full((6, 63, 67), float('nan'), device='cuda')
    covered = torch.zeros(63, 67, dtype=torch.bool)
    for y1, x1 in wins:
        sums[:, y1:y1 + 40, x1:x1 + 40] = 0
        covered[y1:y1 + 40, x1:x1 + 40] = True
    ops.scene_accumulate_(sums, logits, wins, size)
    out = sums.cpu()
    assert bool(torch.isnan(out[:, ~covered]).all()) and not bool(torch.isnan(out[:, covered]).any())
    want = torch.zeros(1, 6, 63, 67, device='cuda')
    for i, (y1, x1) in enumerate(wins):
        ops.window_accumulate_(want, torch.zeros(1, 1, 63, 67, device='cuda'), ops.resize_bilinear(logits[i:i + 1], size), y1, x1)
    assert torch.equal(out[:, covered], want[0].cpu()[:, covered])


# ---------------------------------------------------------------------------------------------------------------- 3. scene_finalize
@pytest.mark.parametrize('hw,C', [((200, 203), 6), ((200, 204), 6), ((80, 200), 6), ((200, 203), 19)])
def test_scene_finalize_equals_normalize_softmax_argmax(hw, C):
    from pfst_amd import hip_ops as ops
    from pfst_amd.scene import cover_counts
    _, _, _, preds, count = _chain(hw, C)
    rows, cols = cover_counts(hw[0], hw[1], CROP, STRIDE)
    assert torch.equal(torch.from_numpy(np.outer(rows, cols)).float(), count[0, 0].cpu())
    probs_ref = ops.softmax_nchw(ops.window_normalize_(preds.clone(), count))
    lab_ref = ops.argmax_nchw(probs_ref)
    lab, conf, probs = ops.scene_finalize(preds[0], torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda(), confidence=True,
                                          return_probs=True)
    assert torch.equal(probs, probs_ref[0])
    assert torch.equal(lab, lab_ref[0])
    p = probs_ref[0].cpu()
    assert torch.equal(conf.cpu(), (p.max(0).values * 255).round().to(torch.uint8))
    only, none_c, none_p = ops.scene_finalize(preds[0], torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda())
    assert none_c is None and none_p is None and torch.equal(only, lab)


def test_scene_finalize_generic_path_and_ties():
    """40 classes (more than the register kernels hold) against the chain, and constructed ties: equal sums resolve to the first class"""
    from pfst_amd import hip_ops as ops
    H, W, C = 21, 30, 40
    g = torch.Generator().manual_seed(8)
    rows = torch.randint(1, 4, (H,), generator=g, dtype=torch.int32)
    cols = torch.randint(1, 4, (W,), generator=g, dtype=torch.int32)
    sums = (4 * torch.randn(1, C, H, W, generator=g)).cuda()
    count = (rows[:, None] * cols[None, :]).float().reshape(1, 1, H, W).cuda()
    probs_ref = ops.softmax_nchw(ops.window_normalize_(sums.clone(), count))
    lab, conf, probs = ops.scene_finalize(sums[0], rows.cuda(), cols.cuda(), confidence=True, return_probs=True)
    assert torch.equal(probs, probs_ref[0]) and torch.equal(lab, ops.argmax_nchw(probs_ref)[0])
    assert torch.equal(conf.cpu(), (probs_ref[0].cpu().max(0).values * 255).round().to(torch.uint8))
    for C, w in ((6, 8), (6, 7), (19, 7), (40, 7)):
        tie = torch.zeros(C, 4, w)
        tie[2] = 1.5
        tie[4] = 1.5
        ones_r, ones_c = torch.ones(4, dtype=torch.int32).cuda(), torch.full((w,), 2, dtype=torch.int32).cuda()
        lab, _, _ = ops.scene_finalize(tie.cuda(), ones_r, ones_c)
        assert int(lab.min()) == 2 and int(lab.max()) == 2, (C, w)


# ---------------------------------------------------------------------------------------------------------------- 4. paint_labels
@pytest.mark.parametrize('hw', [(37, 53), (40, 44)])
def test_paint_labels_equals_show_result(hw):
    """palette only, then the blend for opacities 0, 0.5, 0.3, 0.77, 1 against show_result's NumPy expression (base.py:278-285) in RGB order"""
    from pfst_amd import hip_ops as ops
    from pfst_amd.data import ISPRS_PALETTE
    rs = np.random.RandomState(5)
    lab = rs.randint(0, 6, hw).astype(np.uint8)
    lab[0, :3] = (6, 200, 255)                                        # beyond the palette: show_result leaves colour 0
    scene = rs.randint(0, 256, hw + (3,)).astype(np.uint8)            # BGR
    palette = np.asarray(ISPRS_PALETTE, np.uint8)
    color_seg = np.zeros(hw + (3,), np.uint8)
    for label, color in enumerate(palette):
        color_seg[lab == label, :] = color
    lab_d, pal_d, scene_d = torch.from_numpy(lab).cuda(), torch.from_numpy(palette).cuda(), torch.from_numpy(scene).cuda()
    assert np.array_equal(ops.paint_labels(lab_d, pal_d).cpu().numpy(), color_seg)
    img = scene[..., ::-1]                                            # RGB
    for opacity in (0, 0.5, 0.3, 0.77, 1):
        want = (img * (1 - opacity) + color_seg * opacity).astype(np.uint8)
        got = ops.paint_labels(lab_d, pal_d, scene_d, opacity).cpu().numpy()
        assert np.array_equal(got, want), opacity
    with pytest.raises(ValueError):
        ops.paint_labels(lab_d, pal_d, scene_d, 1.5)


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
_models = {}


def _model(classifier):
    """the model and state of test_eval_gpu._eval_model_and_state in slide mode.  'fixture': as it is -- on any input its classifier
    answers class 5 with p ~ 1, so the label map is constant; 'zero_mean': the decode head's classifier replaced by seeded zero-mean
    weights without a bias, which gives four classes on the scene below -- the arg-max and the ties are then exercised too"""
    if classifier not in _models:
        from test_eval_gpu import _eval_model_and_state
        model, _, _ = _eval_model_and_state(dict(mode='slide', crop_size=CROP, stride=STRIDE))
        seg = model.get_model()
        if classifier == 'zero_mean':
            w = seg.decode_head.conv_seg.weight
            wr = torch.randn(w.shape, generator=torch.Generator().manual_seed(4))
            with torch.no_grad():
                w.copy_(0.01 * (wr - wr.mean(0, keepdim=True)))
                seg.decode_head.conv_seg.bias.zero_()
        _models[classifier] = (model, seg)
    return _models[classifier]


@pytest.mark.parametrize('classifier', ['fixture', 'zero_mean'])
def test_predict_scene_against_the_existing_slide_path(classifier):
    """Scene: uniform random uint8 200 x 203 x 3, seed 21, the ISPRS normalisation.  Reference: the existing path -- pipeline.normalize on
    the host, then seg.inference_probs / seg.inference in slide mode (window 96, stride 64: 9 windows).

    One window per batch: labels, probabilities and confidence are bit-identical to it, in the default arithmetic (the eval-mode forward
    has no sum between workgroups, so the existing path is bit-reproducible run to run; the deterministic mode is not needed).

    Four windows per batch (4 + 4 + 1): the f16x3 convolutions take their scales over the batch, so the result is not bit-identical; the
    bound is the project's for this situation (test_eval_gpu.py:211,215): probabilities within 1e-3 x max p of the batch-1
    result; every pixel whose label differs has a top-two gap <= 2e-3 there; such pixels are fewer than 2e-3 of the scene.  That cap is a
    condition on the input: with the CPU oracle's inference_probs on the same state and scene, the share of pixels whose top-two
    probability gap is <= 2e-3 is 0.0 for both classifiers (smallest p_max 1.0 / 0.503; label histogram (0, 0, 0, 0, 0, 40600) /
    (0, 32254, 0, 6, 28, 8312))."""
    from pfst_amd import pipeline
    from pfst_amd.scene import predict_scene
    _, seg = _model(classifier)
    scene = _scene(21)
    img = torch.from_numpy(pipeline.normalize(scene, **NORM).transpose(2, 0, 1).copy())[None].cuda()
    with torch.no_grad():
        probs_ref, _ = seg.inference_probs(img, None, False)
        lab_ref, _ = seg.inference(img, None, False)
        scene_d = torch.from_numpy(scene).cuda()
        stats = {}
        lab1, conf1, probs1 = predict_scene(seg, scene_d, NORM, CROP, STRIDE, windows_per_batch=1, confidence=True, return_probs=True,
                                            stats=stats)
        lab4, conf4, probs4 = predict_scene(seg, scene_d, NORM, CROP, STRIDE, windows_per_batch=4, confidence=True, return_probs=True)
    assert stats == dict(windows=9, batches=9, window=[96, 96])
    if classifier == 'zero_mean':
        assert len(torch.unique(lab_ref)) >= 3                        # the label map is not constant
    assert torch.equal(probs1, probs_ref[0])
    assert torch.equal(lab1, lab_ref[0])
    assert torch.equal(conf1.cpu(), (probs_ref[0].cpu().max(0).values * 255).round().to(torch.uint8))
    # batched
    p1, p4 = probs1.cpu(), probs4.cpu()
    err, bound = float((p4 - p1).abs().max()), 1e-3 * float(p1.max())
    differ = (lab4 != lab1).cpu()
    top2 = p1.topk(2, dim=0).values
    gap = top2[0] - top2[1]
    print(f'{classifier}: max |p4 - p1| = {err:.3e} (bound {bound:.1e}); labels differ on {int(differ.sum())} of {differ.numel()} pixels')
    assert err < bound
    assert bool((gap[differ] <= 2e-3).all())
    assert float(differ.float().mean()) < 2e-3
    assert int((conf4.cpu().int() - conf1.cpu().int()).abs().max()) <= 1


def test_predict_scene_refuses_what_it_cannot_do():
    from pfst_amd import scene as S
    _, seg = _model('fixture')
    scene_d = torch.from_numpy(_scene(1, 64, 64)).cuda()
    with pytest.raises(ValueError):
        S.predict_scene(seg, scene_d, NORM, CROP, STRIDE, windows_per_batch=17)
    with pytest.raises(ValueError):
        S.predict_scene(seg, scene_d.float(), NORM, CROP, STRIDE)
    free = torch.cuda.mem_get_info()[0]
    fixed, act = S.memory_needed(6, 200000, 200000, (1024, 1024), 8)
    assert fixed > free                                              # 960 GB of sums: more than any device holds
    big = torch.empty(1, 1, 3, dtype=torch.uint8, device='cuda').expand(200000, 200000, 3)        # a view: nothing that size is allocated
    with pytest.raises(MemoryError, match='MiB'):
        S.predict_scene(seg, big, NORM, (1024, 1024), (512, 512))


# ---------------------------------------------------------------------------------------------------------------- 6. CLI
def test_predict_cli_writes_labels_overlay_and_confidence(tmp_path):
    """tools/predict.py on a folder of two PNGs (130 x 150: four windows, one batch; 96 x 96: one window) with a PFGST checkpoint saved from
    the fixture model: <stem>.png holds inference_segmentor's labels and the palette, the overlay is paint_labels of them, the confidence
    map is predict_image's"""
    import json
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import predict as predict_cli
    from pfst_amd import hip_ops as ops
    from pfst_amd.apis import inference_segmentor, init_segmentor, predict_image
    from pfst_amd.data import ISPRS_CLASSES, ISPRS_PALETTE
    model, seg = _model('zero_mean')
    ckpt = tmp_path / 'pfgst.pth'
    torch.save(dict(state_dict=model.state_dict(), meta=dict(CLASSES=ISPRS_CLASSES, PALETTE=ISPRS_PALETTE)), ckpt)
    from helpers import uda_cfg
    model_cfg = uda_cfg()['model']
    model_cfg['test_cfg'] = dict(mode='slide', crop_size=CROP, stride=STRIDE)
    test_pl = [dict(type='LoadImageFromFile'),
               dict(type='MultiScaleFlipAug', img_scale=(1024, 1024), flip=False,
                    transforms=[dict(type='Resize', keep_ratio=True), dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                                dict(type='Collect', keys=['img'])])]
    cfg_path = tmp_path / 'toy.py'
    cfg_path.write_text('model = %r\ndata = %r\n' % (model_cfg, dict(test=dict(type='ISPRSDataset', pipeline=test_pl))))
    folder = tmp_path / 'scenes'
    folder.mkdir()
    scenes = {'a': _scene(31, 130, 150), 'b': _scene(32, 96, 96)}
    for stem, bgr in scenes.items():
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(folder / f'{stem}.png')
    out = tmp_path / 'out'
    with pytest.raises(SystemExit):
        predict_cli.main([str(cfg_path), str(ckpt), str(folder), '--out-dir', str(out)])     # a PFGST checkpoint needs the key revision
    recs = predict_cli.main([str(cfg_path), str(ckpt), str(folder), '--out-dir', str(out), '--opacity', '0.3', '--confidence',
                             '--revise-checkpoint-key'])
    assert [(r['height'], r['width'], r['windows'], r['batches']) for r in recs] == [(130, 150, 4, 1), (96, 96, 1, 1)]
    listed = json.load(open(out / 'predict.json'))
    assert listed['window'] == [96, 96] and listed['stride'] == [64, 64] and len(listed['images']) == 2
    api_model = init_segmentor(str(cfg_path), str(ckpt), 'cuda:0', revise_checkpoint_key=True)
    assert api_model.CLASSES == tuple(ISPRS_CLASSES) and api_model.PALETTE == [list(c) for c in ISPRS_PALETTE]
    pal_d = torch.from_numpy(np.asarray(ISPRS_PALETTE, np.uint8)).cuda()
    for stem, bgr in scenes.items():
        res = inference_segmentor(api_model, str(folder / f'{stem}.png'))
        assert isinstance(res, list) and len(res) == 1 and res[0].dtype == np.uint8 and res[0].shape == bgr.shape[:2]
        assert np.array_equal(res[0], inference_segmentor(api_model, bgr)[0])                # a path and the array it holds
        im = Image.open(out / f'{stem}.png')
        assert im.mode == 'P' and np.array_equal(np.asarray(im), res[0])
        assert im.getpalette()[:18] == [v for c in ISPRS_PALETTE for v in c]
        over = ops.paint_labels(torch.from_numpy(res[0]).cuda(), pal_d, torch.from_numpy(bgr).cuda(), 0.3).cpu().numpy()
        assert np.array_equal(np.asarray(Image.open(out / f'{stem}_overlay.png')), over)
        conf = predict_image(api_model, bgr, confidence=True)['confidence'].cpu().numpy()
        got = Image.open(out / f'{stem}_conf.png')
        assert got.mode == 'L' and np.array_equal(np.asarray(got), conf)
