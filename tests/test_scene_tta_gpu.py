"""Test-time augmentation on whole scenes on the GPU: each of the three kernels of scene_tta.hip bit for bit against the NumPy
expression / the chain of existing kernels it replaces, predict_scene_tta against the existing per-view tile path (bitwise at one window
per batch), against itself batched and against the oracle's aug_test, its refusals, and tools/predict.py end to end.  Shapes follow
test_scene_gpu.py: crop 96, stride 64, width 203 (4-pixel tails, rows off a 16-byte boundary) and 204 (the 16-byte path), views smaller,
equal and larger than the scene, an 80-row view under a 96-row window (clipped windows), 6 / 19 / 40 classes."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
CROP, STRIDE = (96, 96), (64, 64)
RATIOS = [0.5, 1.0, 1.5]


def _scene(seed, h=200, w=203):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- 1. scene_resize_u8
@pytest.mark.parametrize('ratio', [0.5, 0.75, 1.0, 1.25, 1.75])
@pytest.mark.parametrize('hw', [(37, 53), (200, 203)])
def test_scene_resize_equals_the_pipelines_resize(hw, ratio):
    """against pipeline.resize_bilinear_u8 at the view size of the ratio (1.0: the equal-size copy), plain and mirrored: bitwise"""
    from pfst_amd import hip_ops as ops
    from pfst_amd import pipeline
    from pfst_amd.scene import tta_views
    scene = _scene(5, *hw)
    size = tta_views(hw[0], hw[1], [ratio], False)[0]['size']
    assert (size == hw) == (ratio == 1.0)
    want = pipeline.resize_bilinear_u8(scene, size)
    assert want.shape == size + (3,)
    dev = torch.from_numpy(scene).cuda()
    plain = ops.scene_resize_u8(dev, size).cpu().numpy()
    assert np.array_equal(plain, want)
    assert np.array_equal(ops.scene_resize_u8(dev, size, hflip=True).cpu().numpy(), np.flip(want, axis=1))
    assert np.array_equal(ops.scene_resize_u8(dev, size, vflip=True).cpu().numpy(), np.flip(want, axis=0))
    assert np.array_equal(ops.scene_resize_u8(dev, size, hflip=True, vflip=True).cpu().numpy(), np.flip(want, axis=(0, 1)))
    assert np.array_equal(dev.cpu().numpy(), scene)                  # the source is left alone


# ---------------------------------------------------------------------------------------------------------------- 2. scene_tta_accumulate_
_chain_cache = {}


def _chain(hw, C):
    """window sums of a view of size hw as the existing slide path forms them from random low-resolution logits (resize_bilinear +
    window_accumulate_ per window), with the count plane: computed once per case -> (sums [1, C, h, w], count [1, 1, h, w]), left unchanged"""
    from pfst_amd import hip_ops as ops
    from pfst_amd.scene import window_grid
    key = (hw, C)
    if key not in _chain_cache:
        wins, size = window_grid(hw[0], hw[1], CROP, STRIDE)
        logits = (3 * torch.randn(len(wins), C, size[0] // 4, size[1] // 4, generator=torch.Generator().manual_seed(7))).cuda()
        preds, count = torch.zeros(1, C, *hw, device='cuda'), torch.zeros(1, 1, *hw, device='cuda')
        for i, (y1, x1) in enumerate(wins):
            ops.window_accumulate_(preds, count, ops.resize_bilinear(logits[i:i + 1], size), y1, x1)
        _chain_cache[key] = (preds, count)
    return _chain_cache[key]


VIEW_CASES = [((100, 101), (200, 203)), ((300, 304), (200, 203)), ((200, 203), (200, 203)), ((200, 204), (200, 204)), ((80, 101), (160, 203))]


@pytest.mark.parametrize('flips', [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize('C', [6, 19])
@pytest.mark.parametrize('view_hw,out_hw', VIEW_CASES)
def test_view_accumulate_is_bitwise_the_chain(view_hw, out_hw, C, flips):
    """window_normalize_ -> resize_bilinear (skipped when equal) -> softmax_nchw -> flip_planes -> axpy_ / store, against the one pass.
    (200, 204): the 16-byte path; (80, 101): sums of clipped 80 x 96 windows; C = 19: one pixel per thread"""
    from pfst_amd import hip_ops as ops
    from pfst_amd.scene import _view_add_chain, cover_counts
    hflip, vflip = flips
    preds, count = _chain(view_hw, C)
    rows, cols = cover_counts(view_hw[0], view_hw[1], CROP, STRIDE)
    assert torch.equal(torch.from_numpy(np.outer(rows, cols)).float(), count[0, 0].cpu())
    rows_d, cols_d = torch.from_numpy(rows).cuda(), torch.from_numpy(cols).cuda()
    p = ops.window_normalize_(preds.clone(), count)
    if view_hw != out_hw:
        p = ops.resize_bilinear(p, out_hw)
    p = ops.softmax_nchw(p)
    if hflip or vflip:
        p = ops.flip_planes(p, horizontal=hflip, vertical=vflip)
    sums = preds[0].clone()
    # the first view: a store -- whatever acc held (NaNs) is gone
    acc = torch.full((C,) + out_hw, float('nan'), device='cuda')
    ops.scene_tta_accumulate_(acc, sums, rows_d, cols_d, hflip, vflip, accumulate=False)
    assert torch.equal(acc, p[0])
    # a later view: an add
    start = torch.rand((C,) + out_hw, generator=torch.Generator().manual_seed(11)).cuda()
    want = ops.axpy_(start.clone(), p[0].contiguous())
    got = ops.scene_tta_accumulate_(start.clone(), sums, rows_d, cols_d, hflip, vflip, accumulate=True)
    assert torch.equal(got, want)
    assert torch.equal(sums, preds[0])                               # the view sums are read only: no normalised copy is written into them
    # the host's chain for more classes than the kernel holds gives the same values
    assert torch.equal(_view_add_chain(None, sums.clone(), rows_d, cols_d, out_hw, hflip, vflip), p[0])
    assert torch.equal(_view_add_chain(start.clone(), sums.clone(), rows_d, cols_d, out_hw, hflip, vflip), want)


def test_view_accumulate_refuses_too_many_classes():
    from pfst_amd import hip_ops as ops
    from pfst_amd._lib import PfstHipError
    ones_r, ones_c = torch.ones(4, dtype=torch.int32).cuda(), torch.ones(5, dtype=torch.int32).cuda()
    with pytest.raises(PfstHipError):
        ops.scene_tta_accumulate_(torch.zeros(40, 8, 10).cuda(), torch.zeros(40, 4, 5).cuda(), ones_r, ones_c)
    with pytest.raises(ValueError):
        ops.scene_tta_accumulate_(torch.zeros(6, 8, 10).cuda(), torch.zeros(6, 4, 5).cuda(), ones_c, ones_r)


# ---------------------------------------------------------------------------------------------------------------- 3. scene_tta_finalize
@pytest.mark.parametrize('W', [203, 204])
@pytest.mark.parametrize('C', [6, 19, 40])
def test_finalize_equals_div_argmax_and_confidence(C, W):
    """H = 21: 21 x 203 pixels are no multiple of 4 (scalar accesses, a tail group), 21 x 204 are (16-byte accesses)"""
    from pfst_amd import hip_ops as ops
    H, views = 21, 6
    g = torch.Generator().manual_seed(8)
    acc = (views * torch.softmax(2 * torch.randn(C, H, W, generator=g), 0)).cuda()
    before = acc.clone()
    p = ops.div_scalar_(acc.clone()[None], views)
    lab_ref = ops.argmax_nchw(p)[0]
    lab, conf, probs = ops.scene_tta_finalize(acc, views, confidence=True, return_probs=True)
    assert torch.equal(probs, p[0]) and torch.equal(lab, lab_ref) and torch.equal(acc, before)
    assert torch.equal(conf.cpu(), (p[0].cpu().max(0).values * 255).round().to(torch.uint8))
    only, none_c, none_p = ops.scene_tta_finalize(acc, views)
    assert none_c is None and none_p is None and torch.equal(only, lab)
    assert len(torch.unique(lab)) > 1


def test_finalize_ties_go_to_the_first_class():
    from pfst_amd import hip_ops as ops
    for C, w in ((6, 8), (6, 7), (19, 7), (40, 7)):
        tie = torch.zeros(C, 4, w)
        tie[2] = 1.5
        tie[4] = 1.5
        lab, conf, _ = ops.scene_tta_finalize(tie.cuda(), 3, confidence=True)
        assert int(lab.min()) == 2 and int(lab.max()) == 2, (C, w)
        assert int(conf.min()) == 128 and int(conf.max()) == 128     # rint(0.5 * 255) = rint(127.5): half to even


# ---------------------------------------------------------------------------------------------------------------- 4-6. end to end
_state = {}


def _model(classifier):
    """the model and state of test_eval_gpu._eval_model_and_state in slide mode, built once.  'fixture': its classifier as it is -- class 5
    with p ~ 1 on any input, a constant label map; 'small': the decode head's classifier replaced by seeded zero-mean weights of scale 3e-4
    without a bias -- per-view probabilities far from saturation, so that the average over six views has few near-ties (the docstring of the
    batched test).  -> (model, seg, student state for the oracle, oracle module)"""
    if 'model' not in _state:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        from test_eval_gpu import _eval_model_and_state
        model, student, O = _eval_model_and_state(dict(mode='slide', crop_size=CROP, stride=STRIDE))
        seg = model.get_model()
        head = seg.decode_head.conv_seg
        assert 'decode_head.conv_seg.weight' in student and 'decode_head.conv_seg.bias' in student
        wr = torch.randn(head.weight.shape, generator=torch.Generator().manual_seed(4))
        small = (3e-4 * (wr - wr.mean(0, keepdim=True)), torch.zeros(head.bias.shape))
        fixture = (head.weight.detach().cpu().clone(), head.bias.detach().cpu().clone())
        _state.update(model=(model, seg, student, O), weights=dict(fixture=fixture, small=small))
    model, seg, student, O = _state['model']
    w, b = _state['weights'][classifier]
    with torch.no_grad():
        seg.decode_head.conv_seg.weight.copy_(w)
        seg.decode_head.conv_seg.bias.copy_(b)
    sd = dict(student)
    sd['decode_head.conv_seg.weight'], sd['decode_head.conv_seg.bias'] = w.clone(), b.clone()
    return model, seg, sd, O


def _host_views(scene):
    """the six views as the data pipeline makes them on the host: resize_bilinear_u8, np.flip after it, normalize -> [(img [1, 3, h, w]
    float32, flipped)]"""
    from pfst_amd import pipeline
    from pfst_amd.scene import tta_views
    out = []
    for v in tta_views(scene.shape[0], scene.shape[1], RATIOS, True):
        a = pipeline.resize_bilinear_u8(scene, v['size'])
        if v['flip']:
            a = np.flip(a, axis=1)
        img = pipeline.normalize(np.ascontiguousarray(a), **NORM)
        out.append((torch.from_numpy(img.transpose(2, 0, 1).copy())[None], v['flip']))
    return out


def _e2e(classifier):
    """scene seed 21 (200 x 203), ratios 0.5 / 1.0 / 1.5 + flip: the per-view tile path (the reference), predict_scene_tta at one and at
    four windows per batch; computed once per classifier and left unchanged"""
    key = ('e2e', classifier)
    if key not in _state:
        from pfst_amd import hip_ops as ops
        from pfst_amd.scene import predict_scene_tta
        _, seg, _, _ = _model(classifier)
        scene = _scene(21)
        views = _host_views(scene)
        with torch.no_grad():
            seg.repack_weights(need_dgrad=False)
            acc = None
            for img, flipped in views:
                src, mid = seg._tta_forward(img.cuda())
                acc = seg._tta_add(acc, src, mid, scene.shape[:2], 'horizontal' if flipped else None)
            lab_ref = ops.tta_finalize(acc, len(views))[0]
            probs_ref = ops.div_scalar_(acc.clone(), len(views))[0]
            scene_d = torch.from_numpy(scene).cuda()
            stats1, stats4 = {}, {}
            one = predict_scene_tta(seg, scene_d, NORM, CROP, STRIDE, RATIOS, True, windows_per_batch=1, confidence=True, return_probs=True,
                                    stats=stats1)
            four = predict_scene_tta(seg, scene_d, NORM, CROP, STRIDE, RATIOS, True, windows_per_batch=4, confidence=True, return_probs=True,
                                     stats=stats4)
        _state[key] = dict(views=views, lab_ref=lab_ref, probs_ref=probs_ref, one=one, four=four, stats1=stats1, stats4=stats4)
    return _state[key]


@pytest.mark.parametrize('classifier', ['fixture', 'small'])
def test_predict_scene_tta_is_bitwise_the_per_view_tile_path(classifier):
    """One window per batch against the existing tile path, view by view: resize_bilinear_u8 / np.flip / pipeline.normalize on the host,
    seg._tta_forward in slide mode (the metas carry no flip_permutes: every view has its own forward) and seg._tta_add, then tta_finalize.
    Labels and probabilities are bit-identical in the default arithmetic (the eval-mode forward has no sum between workgroups, so the tile
    path is bit-reproducible run to run), the confidence is round(255 p_max)."""
    r = _e2e(classifier)
    lab1, conf1, probs1 = r['one']
    assert r['stats1'] == dict(views=6, view_windows=[4, 4, 9, 9, 25, 25], windows=76, batches=76, window=[96, 96])
    assert r['stats4'] == dict(views=6, view_windows=[4, 4, 9, 9, 25, 25], windows=76, batches=2 * (1 + 3 + 7), window=[96, 96])
    assert torch.equal(probs1, r['probs_ref'])
    assert torch.equal(lab1, r['lab_ref'])
    assert torch.equal(conf1.cpu(), (r['probs_ref'].cpu().max(0).values * 255).round().to(torch.uint8))
    if classifier == 'small':
        assert len(torch.unique(lab1)) >= 2                           # the label map is not constant


@pytest.mark.parametrize('classifier', ['fixture', 'small'])
def test_predict_scene_tta_batched_against_one_window_per_batch(classifier):
    """Four windows per batch: the f16x3 convolutions take their scales over the batch, so the result is not bit-identical; the bound is the
    project's for this situation (test_scene_gpu.py): probabilities within 1e-3 x max p of the batch-1 result, every pixel
    whose label differs has a top-two gap <= 2e-3 there, confidence within 1.  What the gap rule may excuse is capped at 1e-2 of the pixels,
    a condition on the input: the zero-mean classifier of scale 0.01 of test_scene_gpu.py does not meet it under augmentation (the CPU
    oracle puts 11 % of this scene's pixels within 2e-3: saturated per-view probabilities voting 3 : 3), the one of scale 3e-4 used here
    does -- oracle.aug_test on this scene and these six views gives a near-tie share of 0.0019 (76 of 40 600 pixels), smallest p_max 0.484,
    label histogram (0, 37557, 0, 0, 0, 3043); the fixture classifier answers class 5 everywhere (share 0.0)."""
    r = _e2e(classifier)
    (lab1, conf1, probs1), (lab4, conf4, probs4) = r['one'], r['four']
    p1, p4 = probs1.cpu(), probs4.cpu()
    err, bound = float((p4 - p1).abs().max()), 1e-3 * float(p1.max())
    differ = (lab4 != lab1).cpu()
    top2 = p1.topk(2, dim=0).values
    gap = top2[0] - top2[1]
    share = float((gap <= 2e-3).float().mean())
    print(f'{classifier}: max |p4 - p1| = {err:.3e} (bound {bound:.1e}); labels differ on {int(differ.sum())} of {differ.numel()} pixels; '
          f'near-tie share of the batch-1 result {share:.4f}; smallest p_max {float(top2[0].min()):.3f}; '
          f'labels {torch.bincount(lab1.cpu().flatten().long(), minlength=6).tolist()}')
    assert share < 1e-2                                               # the condition on the input
    if classifier == 'small':
        assert len(torch.unique(lab1)) >= 2
    assert err < bound
    assert bool((gap[differ] <= 2e-3).all())
    assert float(differ.float().mean()) < 1e-2
    assert int((conf4.cpu().int() - conf1.cpu().int()).abs().max()) <= 1


def test_predict_scene_tta_against_the_oracle():
    """oracle.aug_test (the reference's aug_test over slide_inference, restated in PyTorch on the CPU) on the same six host-made views, the
    'small' classifier: probabilities within 1e-3 x max, labels differ only where the oracle's top-two gap is <= 2e-3"""
    _, _, sd, O = _model('small')
    r = _e2e('small')
    metas = [[dict(ori_shape=(200, 203, 3), flip=flipped, flip_direction='horizontal')] for _, flipped in r['views']]
    with torch.no_grad():
        ref_pred, ref_prob = O.aug_test(sd, [img.clone() for img, _ in r['views']], metas, dict(mode='slide', crop_size=CROP, stride=STRIDE))
    lab1, _, probs1 = r['one']
    err, bound = float((probs1.cpu() - ref_prob[0]).abs().max()), 1e-3 * float(ref_prob.max())
    differ = lab1.cpu().long() != ref_pred[0]
    top2 = ref_prob[0].topk(2, dim=0).values
    gap = top2[0] - top2[1]
    print(f'max |p - oracle| = {err:.3e} (bound {bound:.1e}); labels differ on {int(differ.sum())} of {differ.numel()} pixels; oracle near-tie '
          f'share {float((gap <= 2e-3).float().mean()):.4f}, smallest p_max {float(top2[0].min()):.3f}, labels '
          f'{torch.bincount(ref_pred.flatten(), minlength=6).tolist()}')
    assert err < bound
    assert bool((gap[differ] <= 2e-3).all())


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_predict_scene_tta_refuses_what_it_cannot_do():
    from pfst_amd import scene as S
    _, seg, _, _ = _model('fixture')
    scene_d = torch.from_numpy(_scene(1, 64, 64)).cuda()
    for bad in ([0.0], [-0.5], [1], [1.0, '2'], []):
        with pytest.raises(ValueError):
            S.predict_scene_tta(seg, scene_d, NORM, CROP, STRIDE, bad)
    for per in (0, 17):
        with pytest.raises(ValueError):
            S.predict_scene_tta(seg, scene_d, NORM, CROP, STRIDE, [1.0], windows_per_batch=per)
    with pytest.raises(ValueError):
        S.predict_scene_tta(seg, scene_d.float(), NORM, CROP, STRIDE, [1.0])
    free = torch.cuda.mem_get_info()[0]
    views = S.tta_views(200000, 200000, [1.0], True)
    fixed, view, act = S.tta_memory_needed(6, 200000, 200000, views, (1024, 1024), (512, 512), 8)
    assert fixed > free                                              # 960 GB for the sum over views: more than any device holds
    big = torch.empty(1, 1, 3, dtype=torch.uint8, device='cuda').expand(200000, 200000, 3)        # a view: nothing that size is allocated
    with pytest.raises(MemoryError, match='MiB'):
        S.predict_scene_tta(seg, big, NORM, (1024, 1024), (512, 512), [1.0], True)


# ---------------------------------------------------------------------------------------------------------------- 8. CLI
def test_predict_cli_with_ratios_and_annotations(tmp_path):
    """tools/predict.py --ratios 0.5 1.0 1.5 on a 200 x 203 PNG with a PFGST checkpoint saved from the model: <stem>.png holds
    inference_segmentor(model, path, ratios=..., flip=True)'s labels, predict.json the ratios and six views; scored with --ann-dir against
    a label map made from that prediction the mIoU over the classes present is 100; without --aug-test / --ratios the outputs are
    today's (inference_segmentor without options)"""
    import json
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import predict as predict_cli
    from helpers import uda_cfg
    from pfst_amd.apis import inference_segmentor, init_segmentor
    from pfst_amd.data import ISPRS_CLASSES, ISPRS_PALETTE
    model, _, _, _ = _model('small')
    ckpt = tmp_path / 'pfgst.pth'
    torch.save(dict(state_dict=model.state_dict(), meta=dict(CLASSES=ISPRS_CLASSES, PALETTE=ISPRS_PALETTE)), ckpt)
    model_cfg = uda_cfg()['model']
    model_cfg['test_cfg'] = dict(mode='slide', crop_size=CROP, stride=STRIDE)
    test_pl = [dict(type='LoadImageFromFile'),
               dict(type='MultiScaleFlipAug', img_scale=(1024, 1024), flip=False,
                    transforms=[dict(type='Resize', keep_ratio=True), dict(type='Normalize', **NORM), dict(type='ImageToTensor', keys=['img']),
                                dict(type='Collect', keys=['img'])])]
    cfg_path = tmp_path / 'toy.py'
    cfg_path.write_text('model = %r\ndata = %r\n' % (model_cfg, dict(test=dict(type='ISPRSDataset', pipeline=test_pl))))
    bgr = _scene(21)
    path = tmp_path / 's.png'
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)
    api_model = init_segmentor(str(cfg_path), str(ckpt), 'cuda:0', revise_checkpoint_key=True)
    want = inference_segmentor(api_model, str(path), ratios=[0.5, 1.0, 1.5], flip=True)[0]
    assert want.shape == (200, 203) and want.dtype == np.uint8 and len(np.unique(want)) >= 2
    assert np.array_equal(want, inference_segmentor(api_model, bgr, ratios=[0.5, 1.0, 1.5], flip=True)[0])
    plain = inference_segmentor(api_model, str(path))[0]
    ann = tmp_path / 'ann'
    ann.mkdir()
    Image.fromarray(want).save(ann / 's.png')
    out = tmp_path / 'out'
    recs = predict_cli.main([str(cfg_path), str(ckpt), str(path), '--out-dir', str(out), '--ratios', '0.5', '1.0', '1.5', '--ann-dir', str(ann),
                             '--revise-checkpoint-key'])
    assert np.array_equal(np.asarray(Image.open(out / 's.png')), want)
    listed = json.load(open(out / 'predict.json'))
    assert listed['ratios'] == [0.5, 1.0, 1.5] and listed['flip'] is True and listed['window'] == [96, 96] and listed['stride'] == [64, 64]
    (rec,) = listed['images']
    assert rec['views'] == 6 and rec['windows'] == 76 and (rec['height'], rec['width']) == (200, 203) and recs[0]['views'] == 6
    present = [c for c in range(6) if (want == c).any()]
    for m in (rec['metric'], listed['metric']):
        assert m['mIoU'] == 100.0 and m['aAcc'] == 100.0 and m['mAcc'] == 100.0
        assert [c for c in range(6) if m['IoU'][c] is not None] == present and all(m['IoU'][c] == 100.0 for c in present)
    assert listed['scored'] == 1
    # without the new options: today's outputs and keys, plus ratios None / flip False / views 1
    out0 = tmp_path / 'out0'
    predict_cli.main([str(cfg_path), str(ckpt), str(path), '--out-dir', str(out0), '--revise-checkpoint-key'])
    assert np.array_equal(np.asarray(Image.open(out0 / 's.png')), plain)
    listed0 = json.load(open(out0 / 'predict.json'))
    assert listed0['ratios'] is None and listed0['flip'] is False and 'metric' not in listed0
    (rec0,) = listed0['images']
    assert rec0['views'] == 1 and rec0['windows'] == 9 and rec0['batches'] == 2 and 'metric' not in rec0
