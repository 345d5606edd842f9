"""Test-time augmentation on whole scenes, the host side without a GPU: the view list of pfst_amd/scene.py against the data
pipeline's MultiScaleFlipAug, the memory estimate, tools/predict.py's new arguments, and the argument plumbing of predict_image."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def test_tta_views_order_and_sizes():
    from pfst_amd.scene import tta_views
    views = tta_views(200, 203, [0.5, 1.0, 1.5], True)
    assert [(v['ratio'], v['size'], v['flip']) for v in views] == [(0.5, (100, 101), False), (0.5, (100, 101), True),
                                                                    (1.0, (200, 203), False), (1.0, (200, 203), True),
                                                                    (1.5, (300, 304), False), (1.5, (300, 304), True)]
    assert [v['scale_index'] for v in views] == [0, 0, 1, 1, 2, 2] and all(v['flip_direction'] == 'horizontal' for v in views)
    plain = tta_views(200, 203, [0.75], False)
    assert len(plain) == 1 and plain[0]['size'] == (150, 152) and plain[0]['flip'] is False
    vert = tta_views(200, 203, [1.0], True, 'vertical')
    assert [(v['flip'], v['flip_direction']) for v in vert] == [(False, 'vertical'), (True, 'vertical')]
    for bad in ([], [0.0], [-1.0], [1], ['1.0'], [1.0, 0]):
        with pytest.raises(ValueError):
            tta_views(200, 203, bad, True)
    with pytest.raises(ValueError):
        tta_views(200, 203, [1e-3], False)                          # nothing left of the scene
    with pytest.raises(ValueError):
        tta_views(200, 203, [1.0], True, 'diagonal')
    with pytest.raises(ValueError):
        tta_views(200, 203, [1.0], True, ['horizontal', 'vertical'])


@pytest.mark.parametrize('hw', [(200, 203), (160, 203), (97, 331)])
def test_tta_views_are_the_pipelines(hw):
    """the sizes (and the order, the flips) are those of the images a Pipeline with MultiScaleFlipAug(img_scale=None) makes of the array"""
    from pfst_amd.evaluation import AUG_TEST_RATIOS
    from pfst_amd.pipeline import Pipeline
    from pfst_amd.scene import tta_views
    ratios = list(AUG_TEST_RATIOS)
    steps = [dict(type='LoadImageFromFile'),
             dict(type='MultiScaleFlipAug', img_scale=None, img_ratios=ratios, flip=True,
                  transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **NORM),
                              dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    img = np.random.RandomState(3).randint(0, 256, hw + (3,)).astype(np.uint8)
    res = Pipeline(steps)(img)
    views = tta_views(hw[0], hw[1], ratios, True)
    assert len(views) == len(res['img']) == 12
    assert [v['size'] for v in views] == [tuple(a.shape[1:]) for a in res['img']]
    assert [v['flip'] for v in views] == list(res['flip']) and [v['scale_index'] for v in views] == list(res['scale_index'])


def test_a_small_view_gives_clipped_windows():
    from pfst_amd.scene import tta_views, window_grid
    (v,) = tta_views(160, 203, [0.5], False)
    assert v['size'] == (80, 101)
    wins, size = window_grid(80, 101, (96, 96), (64, 64))
    assert size == (80, 96) and wins == [(0, 0), (0, 5)]


def test_tta_memory_estimate():
    from pfst_amd import scene as S
    views = S.tta_views(200, 203, [0.5, 1.0, 1.5], True)
    crop, stride = (96, 96), (64, 64)
    fixed, view, act = S.tta_memory_needed(6, 200, 203, views, crop, stride, 4)
    assert fixed == 4 * 6 * 200 * 203 + 200 * 203                    # the sum over views + the labels
    assert view == 4 * 6 * 300 * 304 + 3 * 300 * 304                  # the largest view: its window sums and its resized scene
    assert act == S.ACTIVATION_BYTES_PER_PIXEL * 4 * 96 * 96
    fixed2, _, _ = S.tta_memory_needed(6, 200, 203, views, crop, stride, 4, confidence=True, return_probs=True)
    assert fixed2 == 2 * 4 * 6 * 200 * 203 + 2 * 200 * 203
    # ratio 1 without a flip resizes nothing: the view is the scene itself
    _, view1, act1 = S.tta_memory_needed(6, 200, 203, S.tta_views(200, 203, [1.0], False), crop, stride, 16)
    assert view1 == 4 * 6 * 200 * 203 and act1 == S.ACTIVATION_BYTES_PER_PIXEL * 9 * 96 * 96            # nine windows: one batch of nine
    _, view2, _ = S.tta_memory_needed(6, 200, 203, S.tta_views(200, 203, [1.0], True), crop, stride, 16)
    assert view2 == 4 * 6 * 200 * 203 + 3 * 200 * 203                # the mirrored copy
    # a clipped window: 80 x 96
    _, _, act3 = S.tta_memory_needed(6, 160, 203, S.tta_views(160, 203, [0.5], False), crop, stride, 8)
    assert act3 == S.ACTIVATION_BYTES_PER_PIXEL * 2 * 80 * 96


def test_predict_cli_tta_arguments():
    import predict
    base = lambda *more: predict.parse_args(['c.py', 'w.pth', 'a.png', '--out-dir', 'o', *more])
    a = base()
    assert a.aug_test is False and a.ratios is None and a.no_flip is False and a.ann_dir is None and a.reduce_zero_label is False
    assert predict.tta_options(a) == (None, False)
    assert predict.tta_options(base('--aug-test')) == ([0.5, 0.75, 1.0, 1.25, 1.5, 1.75], True)
    assert predict.tta_options(base('--aug-test', '--no-flip')) == ([0.5, 0.75, 1.0, 1.25, 1.5, 1.75], False)
    assert predict.tta_options(base('--ratios', '0.5', '1', '1.5')) == ([0.5, 1.0, 1.5], True)
    assert predict.tta_options(base('--aug-test', '--ratios', '2')) == ([2.0], True)
    assert predict.tta_options(base('--ratios', '0.75', '--no-flip')) == ([0.75], False)
    assert predict.tta_options(base('--no-flip')) == (None, False)
    assert all(isinstance(r, float) for r in predict.tta_options(base('--ratios', '1', '2'))[0])
    a = base('--ann-dir', 'labels', '--reduce-zero-label')
    assert a.ann_dir == 'labels' and a.reduce_zero_label is True
    for bad in (['--ratios', '0'], ['--ratios', '-1.5'], ['--ratios'], ['--reduce-zero-label']):
        with pytest.raises(SystemExit):
            base(*bad)


def test_metrics_record_and_annotation_lookup(tmp_path):
    import predict
    from PIL import Image
    inter, pred, lab = np.array([30.0, 0.0, 10.0]), np.array([40.0, 0.0, 20.0]), np.array([30.0, 0.0, 30.0])
    rec = predict.metrics_record((inter, pred + lab - inter, pred, lab))
    assert rec == dict(aAcc=round(100 * 40 / 60, 4), mIoU=50.0, mAcc=round(100 * (1 + 1 / 3) / 2, 4), IoU=[75.0, None, 25.0])
    seg = np.random.RandomState(1).randint(0, 7, (13, 17)).astype(np.uint8)
    Image.fromarray(seg).save(tmp_path / 'a.png')
    assert predict.read_annotation(str(tmp_path), 'missing') is None
    assert np.array_equal(predict.read_annotation(str(tmp_path), 'a'), seg)
    reduced = predict.read_annotation(str(tmp_path), 'a', reduce_zero_label=True)
    assert np.array_equal(reduced[seg > 0], seg[seg > 0] - 1) and bool((reduced[seg == 0] == 255).all())


def test_predict_image_selects_the_path_by_its_arguments(monkeypatch):
    """defaults run predict_scene with today's arguments; ratios and / or flip run predict_scene_tta.  The two are replaced by recorders, the
    model by a stand-in whose parameter lives on the host: no GPU work"""
    import torch
    from pfst_amd import apis
    calls = []

    def plain(*a):
        calls.append(('plain', a))
        a[-1].update(windows=1, batches=1, window=[4, 4])
        return torch.zeros(8, 9, dtype=torch.uint8), None, None

    def tta(*a):
        calls.append(('tta', a))
        a[-1].update(windows=2, batches=2, window=[4, 4], views=2, view_windows=[1, 1])
        return torch.zeros(8, 9, dtype=torch.uint8), None, None

    class Model:
        cfg = dict(data=dict(test=dict(pipeline=[dict(type='Normalize', **NORM)])))
        test_cfg = dict(mode='slide', crop_size=(96, 96), stride=(64, 64))

        def parameters(self):
            return iter([torch.zeros(1)])

    monkeypatch.setattr(apis, 'predict_scene', plain)
    monkeypatch.setattr(apis, 'predict_scene_tta', tta)
    img = np.zeros((8, 9, 3), np.uint8)
    out = apis.predict_image(Model(), img)
    kind, a = calls.pop()
    assert kind == 'plain' and len(a) == 9 and a[2:8] == (NORM, (96, 96), (64, 64), 8, False, False) and 'views' not in out
    out = apis.predict_image(Model(), img, ratios=[0.5, 1.0], flip=True, windows_per_batch=4, confidence=True)
    kind, a = calls.pop()
    assert kind == 'tta' and a[2:11] == (NORM, (96, 96), (64, 64), [0.5, 1.0], True, 'horizontal', 4, True, False) and out['views'] == 2
    apis.predict_image(Model(), img, flip=True, flip_direction='vertical')
    kind, a = calls.pop()
    assert kind == 'tta' and a[5:8] == ([1.0], True, 'vertical')               # flip alone: the scene and its mirror image
    apis.predict_image(Model(), img, ratios=[0.75])
    kind, a = calls.pop()
    assert kind == 'tta' and a[5:7] == ([0.75], False)                          # one ratio: the scene at another resolution
    res = apis.inference_segmentor(Model(), img, ratios=None, flip=False, window=None)
    assert calls.pop()[0] == 'plain' and len(res) == 1 and res[0].shape == (8, 9)


def test_scene_tta_entry_points_check_their_arguments():
    """bad arguments are refused on the host before any launch"""
    import ctypes
    from pfst_amd import _lib
    L = _lib.lib()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)            # non-null pointers; no call below gets as far as a launch
    assert L.pfst_scene_resize_u8(None, 10, 10, one, one, one, one, 5, 5, 0, 0, two, None) == -1
    assert L.pfst_scene_resize_u8(one, 10, 10, one, one, one, None, 5, 5, 0, 0, two, None) == -1
    assert L.pfst_scene_resize_u8(one, 10, 10, one, one, one, one, 0, 5, 0, 0, two, None) == -1
    assert L.pfst_scene_resize_u8(one, 10, 10, one, one, one, one, 5, 5, 0, 0, one, None) == -1          # in place
    assert b'scene_tta.hip' in L.pfst_last_error()
    assert L.pfst_scene_tta_accumulate(one, 33, 10, 10, one, one, 0, 0, two, 20, 20, 1, None) == -1       # more classes than registers
    assert L.pfst_scene_tta_accumulate(one, 6, 10, 10, None, one, 0, 0, two, 20, 20, 1, None) == -1
    assert L.pfst_scene_tta_accumulate(one, 6, 10, 10, one, one, 0, 0, one, 20, 20, 1, None) == -1        # in place
    assert L.pfst_scene_tta_accumulate(one, 6, 10, 0, one, one, 0, 0, two, 20, 20, 1, None) == -1
    assert L.pfst_scene_tta_finalize(one, 6, 10, 10, 0, two, None, None, None) == -1                      # no views
    assert L.pfst_scene_tta_finalize(one, 256, 10, 10, 2, two, None, None, None) == -1
    assert L.pfst_scene_tta_finalize(one, 6, 10, 10, 2, None, None, None, None) == -1
