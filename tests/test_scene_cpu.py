"""Whole-scene prediction, the host side without a GPU: the window enumeration and cover counts of pfst_amd/scene.py against a literal
restatement of slide_inference's loop, tools/predict.py's arguments and window defaults, its palette PNG, and the Normalize lookup."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

GRIDS = [(200, 203, 96, 64), (80, 200, 96, 64), (96, 96, 96, 64), (300, 97, 96, 85)]


def _slide_loop(h_img, w_img, h_crop, w_crop, h_stride, w_stride):
    """the window loop of EncoderDecoder.slide_inference (encoder_decoder.py:231-243), restated: -> [(y1, x1, y2, x2)] in its order"""
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    out = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1 = h_idx * h_stride
            x1 = w_idx * w_stride
            y2 = min(y1 + h_crop, h_img)
            x2 = min(x1 + w_crop, w_img)
            y1 = max(y2 - h_crop, 0)
            x1 = max(x2 - w_crop, 0)
            out.append((y1, x1, y2, x2))
    return out


@pytest.mark.parametrize('H,W,crop,stride', GRIDS)
def test_window_grid_is_the_loop_of_slide_inference(H, W, crop, stride):
    from pfst_amd.scene import window_grid
    wins, (h, w) = window_grid(H, W, (crop, crop), (stride, stride))
    ref = _slide_loop(H, W, crop, crop, stride, stride)
    assert wins == [(y1, x1) for y1, x1, _, _ in ref]
    assert all((y2 - y1, x2 - x1) == (h, w) for y1, x1, y2, x2 in ref)          # one window size per scene
    assert (h, w) == (min(crop, H), min(crop, W))
    assert all(0 <= y and y + h <= H and 0 <= x and x + w <= W for y, x in wins)


@pytest.mark.parametrize('H,W,crop,stride', GRIDS + [(130, 150, 96, 64)])
def test_cover_counts_factorise_the_count_plane(H, W, crop, stride):
    from pfst_amd.scene import cover_counts
    rows, cols = cover_counts(H, W, (crop, crop), (stride, stride))
    assert rows.dtype == np.int32 and cols.dtype == np.int32 and rows.shape == (H,) and cols.shape == (W,)
    count = np.zeros((H, W), np.int64)
    for y1, x1, y2, x2 in _slide_loop(H, W, crop, crop, stride, stride):
        count[y1:y2, x1:x2] += 1
    assert np.array_equal(rows[:, None].astype(np.int64) * cols[None, :], count)
    assert count.min() >= 1


def test_window_grid_with_a_rectangular_window():
    from pfst_amd.scene import cover_counts, window_grid
    wins, size = window_grid(150, 260, (64, 96), (48, 80))
    ref = _slide_loop(150, 260, 64, 96, 48, 80)
    assert wins == [(a, b) for a, b, _, _ in ref] and size == (64, 96)
    rows, cols = cover_counts(150, 260, (64, 96), (48, 80))
    count = np.zeros((150, 260), np.int64)
    for y1, x1, y2, x2 in ref:
        count[y1:y2, x1:x2] += 1
    assert np.array_equal(np.outer(rows, cols), count)


def _write_cfg(tmp_path, test_cfg):
    from pfst_amd.presets import model_cfg
    m = model_cfg()
    m['test_cfg'] = test_cfg
    path = tmp_path / f"cfg_{test_cfg['mode']}.py"
    path.write_text('model = %r\n' % (m,))
    return str(path)


def test_predict_cli_arguments_and_window_defaults(tmp_path):
    import predict
    args = predict.parse_args(['c.py', 'w.pth', 'a.png', 'dir', '--out-dir', 'o'])
    assert (args.config, args.checkpoint, args.inputs, args.out_dir) == ('c.py', 'w.pth', ['a.png', 'dir'], 'o')
    assert args.opacity is None and args.confidence is False and args.window is None and args.stride is None
    assert args.windows_per_batch == 8 and args.revise_checkpoint_key is False and args.gpu_id == 0 and args.cfg_options is None
    args = predict.parse_args(['c.py', 'w.pth', 'a.png', '--out-dir', 'o', '--opacity', '0.3', '--confidence', '--window', '512', '--stride',
                               '256', '--windows-per-batch', '4', '--revise-checkpoint-key', '--gpu-id', '1', '--cfg-options', 'a.b=1'])
    assert (args.opacity, args.confidence, args.window, args.stride, args.windows_per_batch) == (0.3, True, 512, 256, 4)
    assert args.revise_checkpoint_key and args.gpu_id == 1 and args.cfg_options == ['a.b=1']
    for bad in (['--opacity', '1.5'], ['--windows-per-batch', '17'], ['--windows-per-batch', '0']):
        with pytest.raises(SystemExit):
            predict.parse_args(['c.py', 'w.pth', 'a.png', '--out-dir', 'o'] + bad)
    with pytest.raises(SystemExit):
        predict.parse_args(['c.py', 'w.pth', 'a.png'])                          # --out-dir is required
    # window / stride: a slide config's own, 1024 / 512 for a whole-image config, the flags over both
    slide = _write_cfg(tmp_path, dict(mode='slide', crop_size=(96, 128), stride=(64, 85)))
    whole = _write_cfg(tmp_path, dict(mode='whole'))
    base = lambda cfg, *more: predict.parse_args([cfg, 'w.pth', 'a.png', '--out-dir', 'o', *more])
    a = base(slide)
    assert predict.window_and_stride(a, predict.load_config(a)) == ((96, 128), (64, 85))
    a = base(whole)
    assert predict.window_and_stride(a, predict.load_config(a)) == ((1024, 1024), (512, 512))
    a = base(slide, '--window', '256')
    assert predict.window_and_stride(a, predict.load_config(a)) == ((256, 256), (64, 85))
    a = base(whole, '--window', '768', '--stride', '384')
    assert predict.window_and_stride(a, predict.load_config(a)) == ((768, 768), (384, 384))
    a = base(whole, '--cfg-options', 'model.test_cfg.mode=slide', 'model.test_cfg.crop_size=(640,640)', 'model.test_cfg.stride=(320,320)')
    assert predict.window_and_stride(a, predict.load_config(a)) == ((640, 640), (320, 320))


def test_list_images_expands_folders_and_refuses_equal_stems(tmp_path):
    import predict
    (tmp_path / 'd').mkdir()
    for name in ('d/b.png', 'd/a.tif', 'd/notes.txt', 'c.png'):
        (tmp_path / name).write_bytes(b'')
    got = predict.list_images([str(tmp_path / 'd'), str(tmp_path / 'c.png')])
    assert [s for _, s in got] == ['a', 'b', 'c']
    (tmp_path / 'd' / 'c.tif').write_bytes(b'')
    with pytest.raises(SystemExit):
        predict.list_images([str(tmp_path / 'd'), str(tmp_path / 'c.png')])


def test_label_png_reads_back_to_the_indices_and_the_palette(tmp_path):
    import predict
    from PIL import Image
    from pfst_amd.data import ISPRS_PALETTE
    lab = np.random.RandomState(0).randint(0, 6, (37, 53)).astype(np.uint8)
    path = str(tmp_path / 'lab.png')
    predict.write_label_png(path, lab, ISPRS_PALETTE)
    im = Image.open(path)
    assert im.mode == 'P'
    assert np.array_equal(np.asarray(im), lab)
    assert im.getpalette()[:18] == [v for c in ISPRS_PALETTE for v in c]
    assert np.array_equal(np.asarray(im.convert('RGB')), np.asarray(ISPRS_PALETTE, np.uint8)[lab])       # the same file is the colour picture


def _dec(v):
    if isinstance(v, dict):
        return tuple(_dec(x) for x in v['__tuple__']) if set(v) == {'__tuple__'} else {k: _dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_dec(x) for x in v]
    return v


@pytest.mark.parametrize('name', ['pfst_inria_da', 'pfst_pots_irrg2vaih_irrg', 'pfst_vaih_irrg2pots_irrg', 'pfst_season_net_sp2fa'])
def test_normalize_lookup_in_the_shipped_presets(name):
    """the four shipped test pipelines: three carry Normalize inside their MultiScaleFlipAug; season_net has none anywhere (it clips and
    scales 16-bit bands with ClipNormalize), so the lookup finds nothing there and scene prediction, which reads 8-bit images, refuses it"""
    from pfst_amd.apis import find_normalize, scene_norm_cfg
    with open(os.path.join(ROOT, 'tests', 'golden', 'reference_configs.json')) as f:
        pipeline = _dec(json.load(f)[name])['data']['test']['pipeline']
    assert not any(s['type'] == 'Normalize' for s in pipeline)                  # never at the top level: the lookup has to descend
    if name == 'pfst_season_net_sp2fa':
        assert find_normalize(pipeline) is None
        with pytest.raises(NotImplementedError):
            scene_norm_cfg(pipeline)
        return
    want = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    assert find_normalize(pipeline) == want and scene_norm_cfg(pipeline) == want


def test_normalize_lookup_defaults_to_the_loader_metas():
    from pfst_amd.apis import find_normalize, scene_norm_cfg
    flat = [dict(type='LoadImageFromFile'), dict(type='Normalize', mean=[1.0, 2.0, 3.0], std=[4.0, 5.0, 6.0], to_rgb=False)]
    assert find_normalize(flat) == dict(mean=[1.0, 2.0, 3.0], std=[4.0, 5.0, 6.0], to_rgb=False)
    for none in ([dict(type='LoadImageFromFile')], [], None):
        assert scene_norm_cfg(none) == dict(mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], to_rgb=False)


def test_scene_entry_points_check_their_arguments():
    """bad arguments are refused on the host before any launch: more than 16 windows, a window outside the scene, null pointers, C < 1"""
    import ctypes
    from pfst_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)                                   # a non-null pointer; no call below gets as far as a launch
    yx = lambda *v: (ctypes.c_int * len(v))(*v)
    assert L.pfst_scene_windows(one, 100, 100, yx(*([0, 0] * 17)), 17, 10, 10, 0, 0, 0, 1, 1, 1, 0, one, None) == -1
    assert L.pfst_scene_windows(one, 100, 100, yx(0, 0, 91, 0), 2, 10, 10, 0, 0, 0, 1, 1, 1, 0, one, None) == -1
    assert L.pfst_scene_windows(one, 100, 100, yx(0, -1), 1, 10, 10, 0, 0, 0, 1, 1, 1, 0, one, None) == -1
    assert L.pfst_scene_windows(None, 100, 100, yx(0, 0), 1, 10, 10, 0, 0, 0, 1, 1, 1, 0, one, None) == -1
    assert b'scene.hip' in L.pfst_last_error()
    assert L.pfst_scene_accumulate(one, 600, 1, 0, 10, 10, yx(0, 0), 40, 40, one, 100, 100, None) == -1
    assert L.pfst_scene_accumulate(one, 600, 1, 6, 10, 10, yx(0, 61), 40, 40, one, 100, 100, None) == -1
    assert L.pfst_scene_accumulate(one, 600, 1, 6, 10, 10, yx(0, 0), 40, 40, None, 100, 100, None) == -1
    assert L.pfst_scene_finalize(one, 0, 10, 10, one, one, one, None, None, None) == -1
    assert L.pfst_scene_finalize(one, 6, 10, 10, None, one, one, None, None, None) == -1
    assert L.pfst_paint_labels(one, 10, 10, one, 257, None, 0.0, 0.0, one, None) == -1
    assert L.pfst_paint_labels(one, 10, 10, one, 6, one, 0.5, 1.5, one, None) == -1
    from pfst_amd import hip_ops as ops
    assert ops.SCENE_MAX_WINDOWS == 16
    with pytest.raises(ValueError):
        ops._win_yx([(0, 0)] * 17)
