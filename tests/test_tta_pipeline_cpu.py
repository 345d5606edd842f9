"""MultiScaleFlipAug with ratios, scales and flips (rsiseg/datasets/pipelines/test_time_aug.py) on the CPU: the views' order, multiplicity
and metas, the single-view path unchanged, flipped views as exact flips of their plain view (the premise of the paired-flip forward), and
tools/test.py --aug-test rewriting the right pipeline step."""
import copy
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]


def _dec(v):
    if isinstance(v, dict):
        return tuple(_dec(x) for x in v['__tuple__']) if set(v) == {'__tuple__'} else {k: _dec(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_dec(x) for x in v]
    return v


def _shipped_test_pipeline(name):
    with open(os.path.join(ROOT, 'tests', 'golden', 'reference_configs.json')) as f:
        return _dec(json.load(f)[name])['data']['test']['pipeline']


def _tile(seed, h, w):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def _expected_views(scales, flip, directions):
    """test_time_aug.py:108-117: scale-major, then flip, then each direction"""
    return [(s, f, d) for s in scales for f in ([False, True] if flip else [False]) for d in directions]


@pytest.mark.parametrize('name', ['pfst_pots_irrg2vaih_irrg', 'pfst_vaih_irrg2pots_irrg'])
def test_shipped_test_pipelines_with_six_ratios_and_flip(name):
    from pfst_amd.evaluation import enable_aug_test
    from pfst_amd.pipeline import Pipeline
    single = _shipped_test_pipeline(name)
    pl = copy.deepcopy(single)
    step = enable_aug_test(pl)
    msfa = [s for s in pl if s['type'] == 'MultiScaleFlipAug'][0]
    assert step is msfa and msfa['img_ratios'] == RATIOS and msfa['flip'] is True
    assert [t['type'] for t in msfa['transforms']][:2] == ['Resize', 'RandomFlip']       # the commented-out RandomFlip, after the Resize
    base = single[1]['img_scale']
    scales = [(int(base[0] * r), int(base[1] * r)) for r in RATIOS]
    img = _tile(1, 300, 200)
    P = Pipeline(pl)
    out = P(img)
    views = _expected_views(scales, True, ['horizontal'])
    assert list(zip(out['scale'], out['flip'], out['flip_direction'])) == views
    assert out['scale_index'] == [i // 2 for i in range(len(views))] and all(out['flip_permutes'])
    from pfst_amd.pipeline import rescale_size
    for v, (s, f, d) in enumerate(views):
        hw = rescale_size((300, 200), s)
        assert out['img'][v].shape == (3,) + hw and out['img'][v].dtype == np.float32
    # the r = 1.0, unflipped view is byte for byte the single-view pipeline's output
    ref = Pipeline(single)(img)
    assert Pipeline(single).tta is None
    v1 = views.index((tuple(base), False, 'horizontal'))
    assert out['img'][v1].tobytes() == ref['img'].tobytes() and out['img_norm_cfg'][v1] == ref['img_norm_cfg']
    # every flipped view is its plain view mirrored, exactly
    for v in range(0, len(views), 2):
        assert np.array_equal(out['img'][v + 1], np.ascontiguousarray(out['img'][v][:, :, ::-1]))


def test_flip_false_with_two_directions_keeps_the_duplicated_plain_view():
    from pfst_amd.pipeline import Pipeline
    pl = copy.deepcopy(_shipped_test_pipeline('pfst_pots_irrg2vaih_irrg'))
    pl[1].update(img_ratios=[0.5, 1.0], flip=False, flip_direction=['horizontal', 'vertical'])
    pl[1]['transforms'].insert(1, dict(type='RandomFlip'))
    img = _tile(2, 64, 96)
    with pytest.warns(UserWarning, match='flip_direction has no effect'):
        P = Pipeline(pl)
    out = P(img)
    assert list(zip(out['scale'], out['flip'], out['flip_direction'])) == _expected_views([(512, 512), (1024, 1024)], False,
                                                                                          ['horizontal', 'vertical'])
    assert np.array_equal(out['img'][0], out['img'][1]) and np.array_equal(out['img'][2], out['img'][3])
    # flip=True with both directions: plain, plain, h-flip, v-flip per scale
    pl[1]['flip'] = True
    out = Pipeline(pl)(img)
    assert list(zip(out['flip'], out['flip_direction']))[:4] == [(False, 'horizontal'), (False, 'vertical'), (True, 'horizontal'),
                                                                  (True, 'vertical')]
    assert np.array_equal(out['img'][2], out['img'][0][:, :, ::-1]) and np.array_equal(out['img'][3], out['img'][0][:, ::-1, :])


def test_img_scale_none_takes_the_image_size_times_each_ratio():
    from pfst_amd.pipeline import Pipeline
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    pl = [dict(type='LoadImageFromFile'),
          dict(type='MultiScaleFlipAug', img_scale=None, img_ratios=[0.5, 1.5], flip=True,
               transforms=[dict(type='Resize', keep_ratio=False), dict(type='RandomFlip'), dict(type='Normalize', **norm),
                           dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])])]
    out = Pipeline(pl)(_tile(3, 40, 60))
    # (int(w * r), int(h * r)) -- Resize(keep_ratio=False) reads it as (w, h)
    assert out['scale'] == [(30, 20), (30, 20), (90, 60), (90, 60)]
    assert [a.shape for a in out['img']] == [(3, 20, 30)] * 2 + [(3, 60, 90)] * 2
    with pytest.raises(ValueError):
        Pipeline([dict(type='MultiScaleFlipAug', img_scale=(64, 64), img_ratios=[1, 2], transforms=[dict(type='Resize')])])


def test_flips_that_are_not_permutations_are_recorded():
    """RandomFlip in front of the Resize: a flipped view is not the plain view mirrored, the item says so (the model then runs each view)"""
    from pfst_amd.pipeline import Pipeline
    pl = [dict(type='MultiScaleFlipAug', img_scale=(48, 48), img_ratios=[1.0], flip=True,
               transforms=[dict(type='RandomFlip'), dict(type='Resize', keep_ratio=True), dict(type='ImageToTensor', keys=['img'])])]
    out = Pipeline(pl)(_tile(4, 30, 30))
    assert out['flip'] == [False, True] and out['flip_permutes'] == [False, False]


def test_tile_folder_items_of_a_multi_view_pipeline(tmp_path):
    from PIL import Image
    from pfst_amd.data import TileFolder
    from pfst_amd.evaluation import enable_aug_test
    os.makedirs(tmp_path / 'img'), os.makedirs(tmp_path / 'ann')
    Image.fromarray(_tile(5, 50, 70)).save(tmp_path / 'img' / 'a.png')
    Image.fromarray(np.zeros((50, 70), np.uint8)).save(tmp_path / 'ann' / 'a.png')
    pl = copy.deepcopy(_shipped_test_pipeline('pfst_vaih_irrg2pots_irrg'))
    pl[1]['img_scale'] = (64, 64)
    single = copy.deepcopy(pl)
    enable_aug_test(pl)
    cfg = dict(type='ISPRSDataset', data_root=str(tmp_path), img_dir='img', ann_dir='ann', pipeline=pl)
    item = TileFolder(cfg, test_mode=True)[0]
    assert isinstance(item['img'], list) and len(item['img']) == len(item['img_metas']) == 12
    m = item['img_metas'][1]
    assert m['ori_shape'] == (50, 70, 3) and m['flip'] is True and m['flip_direction'] == 'horizontal' and m['scale'] == (32, 32)
    assert m['img_shape'] == tuple(item['img'][1].shape[1:]) + (3,) and m['scale_index'] == 0 and m['flip_permutes'] is True
    one = TileFolder(dict(cfg, pipeline=single), test_mode=True)[0]          # single-view items keep their layout
    assert not isinstance(one['img'], list) and one['img_metas']['ori_shape'] == (50, 70, 3)
    assert one['img'].numpy().tobytes() == item['img'][4].numpy().tobytes()


def test_test_cli_aug_test_flag_rewrites_the_multi_scale_step(tmp_path):
    """--aug-test finds MultiScaleFlipAug by type (season_net's test pipeline has it at index 3, not 1) and sets the six ratios + flip"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import test as test_cli
    with open(os.path.join(ROOT, 'tests', 'golden', 'reference_configs.json')) as f:
        cfg = _dec(json.load(f)['pfst_season_net_sp2fa'])
    path = tmp_path / 'c.py'
    path.write_text('data = %r\n' % (cfg['data'],))
    args = test_cli.parse_args([str(path), 'ck.pth', '--aug-test', '--work-dir', str(tmp_path)])
    assert args.aug_test
    pl = test_cli.load_config(args).data['test']['pipeline']
    idx = [i for i, s in enumerate(pl) if s['type'] == 'MultiScaleFlipAug']
    assert idx == [3]
    assert pl[3]['img_ratios'] == RATIOS and pl[3]['flip'] is True
    assert not test_cli.parse_args([str(path), 'ck.pth']).aug_test
    plain = test_cli.load_config(test_cli.parse_args([str(path), 'ck.pth'])).data['test']['pipeline']
    assert plain[3].get('img_ratios') is None and plain[3]['flip'] is False
