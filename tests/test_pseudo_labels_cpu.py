"""Offline pseudo-labels, the parts that need no GPU: the float64 restatement of the reference's two formulas against numbers
the reference's own files returned (tests/golden/pseudo_labels.npz), the radix select's digit walk against np.sort over a NumPy emulation of
the histogram kernel, the rank arithmetic, the refusals, the C ABI of the three entry points, the command line and the teacher's keys."""
import ctypes
import os
import sys

import numpy as np
import pytest

import pseudo_label_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import pseudo_label
    return pseudo_label


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'pseudo_labels.npz')))


# ------------------------------------------------------------------------------------------------ the restatement against the reference
def test_fp64_restatement_agrees_with_the_reference(golden):
    logits, ratios, table, labels = golden['logits'], [float(r) for r in golden['ratios']], golden['thresholds'], golden['labels']
    N, C, H, W = logits.shape
    z = oracle.upsample64(logits, (H, W))
    p = oracle.softmax64(z)
    e0, q0 = oracle.hook_entropy(p)
    # thresholds: the same order statistic of the same class sets once the pixel the reference's permutation dropped is removed.  The
    # reference's numbers are float32 entropies: six terms |p log p| <= 0.37, each a few float32 roundings (6e-8) off -> within 1e-6 of the
    # float64 value
    t64, n_c = oracle.thresholds(e0, q0, ratios, C, drop=golden['dropped'])
    assert n_c.sum() == N * H * W - 1 and (n_c > 0).all()
    assert table.dtype == np.float32 and table.shape == t64.shape
    print('thresholds: max |reference - float64|', np.abs(table - t64).max())
    assert np.abs(table - t64).max() <= 1e-6
    # ... and that bound IS the rank identity: of the class's float64 order statistics the one nearest to the reference's number has index
    # int(n_c r), and its neighbours lie more than twice the bound away
    flat_e, flat_q = np.delete(e0.reshape(-1), golden['dropped']), np.delete(q0.reshape(-1), golden['dropped'])
    for c in range(C):
        s = np.sort(flat_e[flat_q == c])
        for i, r in enumerate(ratios):
            k = int(s.size * r)
            assert int(np.argmin(np.abs(s - float(table[i, c])))) == k, (r, c)
            near = min(s[k] - s[k - 1] if k > 0 else np.inf, s[k + 1] - s[k] if k + 1 < s.size else np.inf)
            assert near > 2e-6, (r, c, near)
    # ... and not otherwise: the dropped pixel moves the ranks of its class
    t_all, n_all = oracle.thresholds(e0, q0, ratios, C)
    assert n_all.sum() == N * H * W and np.abs(table - t_all).max() > 1e-4
    # labels: everywhere but at each class's threshold pixel itself.  thre@r IS the hook's entropy of one pixel of the class, and the loader's
    # entropy of that pixel differs from it by the 1e-8 inside the logarithm and float32 rounding only: which side of `<` it falls on is the
    # reference's rounding, not the formula.  Those are the pixels within the 1e-6 of above of their threshold -- at most one per class.
    e1, q1 = oracle.loader_entropy(z, p)
    thr = table[ratios.index(float(golden['label_ratio']))].astype(np.float64)
    lab, counts = oracle.labels(e1, q1, thr)
    own = np.abs(e1 - thr[q1]) <= 1e-6
    print('labels:', int((lab != labels).sum()), 'differ, all among the', int(own.sum()), 'threshold pixels')
    assert own.sum() <= C and np.array_equal(lab[~own], labels[~own])
    assert counts[:, 0].sum() == N * H * W and abs(int(counts[:, 1].sum()) - int((labels != 255).sum())) <= C
    ann, _ = oracle.labels(e1, q1, thr, annotation_space=True)
    assert np.array_equal(np.where(ann == 0, 255, ann.astype(np.int64) - 1), lab)


# ------------------------------------------------------------------------------------------------ the digit walk
def emulated_hist(keys, pred, C):
    """the histogram kernel on NumPy arrays: keys uint32, pred per key -> hist_fn(shift, bits, prefix)"""
    calls = []

    def hist_fn(shift, bits, prefix):
        calls.append((shift, bits))
        h = np.zeros((C, 1 << bits), np.int64)
        k64 = keys.astype(np.uint64)
        live = np.ones(keys.size, bool) if prefix is None else (k64 >> np.uint64(shift + bits)) == prefix.astype(np.uint64)[pred]
        np.add.at(h, (pred[live], ((k64[live] >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)), 1)
        return h
    return hist_fn, calls


@pytest.mark.parametrize('levels', [[(21, 11), (10, 11), (0, 10)], [(24, 8), (16, 8), (8, 8), (0, 8)], [(16, 16), (0, 16)]])
def test_digit_walk_equals_sort(levels):
    from pfst_amd.pseudo_labels import digit_walk, rank_of
    rng = np.random.RandomState(3)
    C = 5
    ent = np.abs(rng.randn(4000).astype(np.float32)) * np.float32(0.7)
    ent[:600] = np.float32(0.25)                   # a long tie run
    ent[600:640] = 0.0                             # +0 keys
    pred = rng.randint(0, 3, size=ent.size)        # classes 0..2 populated
    pred[-1] = 3                                   # class 3: exactly one key; class 4: empty
    pred[:600] = 1
    pred[600:640] = 0
    keys = ent.view(np.uint32)
    hist_fn, calls = emulated_hist(keys, pred, C)
    n_c = np.bincount(pred, minlength=C)
    assert n_c[3] == 1 and n_c[4] == 0
    for name, ranks in (('k = 0', [0, 0, 0, 0, None]), ('k = n - 1', [n_c[0] - 1, n_c[1] - 1, n_c[2] - 1, 0, None]),
                        ('inside the tie run', [rank_of(n_c[0], 0.5), 300, rank_of(n_c[2], 0.99), 0, None])):
        got = digit_walk(hist_fn, ranks, levels)
        for c in range(C):
            if ranks[c] is None:
                assert got[c] == 0, name                                                   # an empty class gives 0
            else:
                want = np.sort(ent[pred == c])[ranks[c]]
                assert got[c:c + 1].view(np.float32)[0].tobytes() == want.tobytes(), (name, c)
    tie = digit_walk(hist_fn, [None, 300, None, None, None], levels)
    assert tie[1:2].view(np.float32)[0] == np.float32(0.25) and (np.sort(ent[pred == 1]) == np.float32(0.25)).sum() >= 600
    # one histogram per level, the first without a prefix; a rank outside the class is refused
    assert calls[:len(levels)] == list(levels)
    with pytest.raises(ValueError, match='outside'):
        digit_walk(hist_fn, [int(n_c[0]), 0, 0, 0, None], levels)
    # a precomputed first level is used instead of a call
    n0 = len(calls)
    digit_walk(hist_fn, [0, 0, 0, 0, None], levels, top=hist_fn(*levels[0], None))
    assert len(calls) - n0 == len(levels)


def test_radix_levels_cover_the_key():
    from pfst_amd.pseudo_labels import LDS_ENTRIES, radix_levels
    for C in (1, 2, 6, 7, 12, 13, 24, 33, 48, 49, 255):
        lv = radix_levels(C)
        assert sum(b for _, b in lv) == 32 and lv[-1][0] == 0 and lv[0][0] + lv[0][1] == 32
        assert all(a[0] == b[0] + b[1] for a, b in zip(lv, lv[1:]))
        assert (C << lv[0][1]) <= LDS_ENTRIES or lv[0][1] == 8
    assert radix_levels(6) == [(21, 11), (10, 11), (0, 10)] and radix_levels(33)[0] == (24, 8)


def test_rank_is_the_python_float_product():
    from pfst_amd.pseudo_labels import rank_of
    for n in (1, 2, 3, 10, 477, 12800, 398 * 1024 * 1024, 2 ** 40 + 1):
        for r in (0.0, 0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.99):
            assert rank_of(n, r) == int(n * r) and 0 <= rank_of(n, r) < n
    # the float product, not exact rational arithmetic: 0.3 is below 3/10 as a double, 0.1 + 0.2 above it
    assert rank_of(10, 0.3) == 3 and rank_of(10, 0.1 + 0.2) == 3 and rank_of(100, 0.29) == int(100 * 0.29) == 28
    assert rank_of(np.int64(7), np.float64(0.5)) == 3


def test_ratios_outside_the_range_are_refused():
    from pfst_amd.pseudo_labels import DEFAULT_RATIOS, check_ratios
    assert check_ratios(DEFAULT_RATIOS, 0.5) == [0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5]
    assert check_ratios([0, 0.99]) == [0.0, 0.99]
    for bad in ([-0.1], [1.0], [0.5, 1.5], [float('nan')], []):
        with pytest.raises(ValueError):
            check_ratios(bad)
    with pytest.raises(ValueError, match='not one of'):
        check_ratios([0.2, 0.4], 0.5)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points():
    from pfst_amd import _lib
    decls = _lib.parse_header()
    names = lambda f: [a[1] for a in decls[f][1]]
    shape = ['logits', 'N', 'C', 'h', 'w', 'H', 'W']
    assert names('pfst_entropy_upsample') == shape + ['mode', 'ent', 'pred', 'stream']
    assert names('pfst_entropy_class_hist') == shape + ['shift', 'bits', 'prefix', 'hist', 'stream']
    assert names('pfst_entropy_pseudo_label') == shape + ['thr', 'annotation_space', 'label', 'counts', 'stream']
    assert [a[0] for a in decls['pfst_entropy_class_hist'][1]] == [ctypes.c_void_p] + [ctypes.c_int] * 8 + [ctypes.c_void_p] * 3
    # the definitions' parameter lists are the declarations', token for token; the file is built without the SLP vectoriser and reads no
    # environment
    import re
    text = open(_lib.HEADER).read()
    src = open(os.path.join(ROOT, 'pfst_amd', 'csrc', 'entropy_labels.hip')).read()
    for name in ('pfst_entropy_upsample', 'pfst_entropy_class_hist', 'pfst_entropy_pseudo_label'):
        norm = lambda s: ' '.join(re.search(name + r'\s*\(([^)]*)\)', s).group(1).split())
        assert norm(text) == norm(src[src.index('extern "C" int ' + name):]), name
    from pfst_amd.build import NO_SLP, SOURCES
    assert 'entropy_labels.hip' in SOURCES and 'entropy_labels.hip' in NO_SLP and 'getenv' not in src
    assert os.path.exists(_lib.LIB_PATH), 'run python -m pfst_amd.build'
    L = _lib.lib()
    assert L.pfst_abi_version() == 1
    # arguments are checked on the host before any launch
    assert L.pfst_entropy_upsample(None, 1, 6, 8, 8, 32, 32, 0, None, None, None) == -1
    assert b'entropy_labels.hip' in L.pfst_last_error()
    assert L.pfst_entropy_class_hist(None, 1, 6, 8, 8, 32, 32, 21, 11, None, None, None) == -1
    assert L.pfst_entropy_pseudo_label(None, 1, 6, 8, 8, 32, 32, None, 0, None, None, None) == -1
    for f in ('pfst_entropy_upsample', 'pfst_entropy_class_hist', 'pfst_entropy_pseudo_label'):
        n = len(decls[f][1])
        with pytest.raises(TypeError, match='takes'):
            _lib.call(f, *([0] * (n + 1)))
        with pytest.raises(TypeError, match='takes'):
            _lib.call(f, *([0] * (n - 1)))


def test_front_end_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from pfst_amd import hip_ops as ops
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.entropy_upsample(torch.zeros(1, 6, 4, 4), (16, 16))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.entropy_class_hist(torch.zeros(1, 6, 4, 4), (16, 16), 21, 11, torch.zeros(6, 2048, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.entropy_pseudo_label(torch.zeros(1, 6, 4, 4), (16, 16), torch.zeros(6))


# ------------------------------------------------------------------------------------------------ the command line, the teacher's keys
def test_cli_parsing():
    tool = _tool()
    a = tool.parse_args(['--synthetic', '3', '--out-dir', 'o'])
    assert a.ratio == [0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5] and a.label_ratio == 0.5 and a.split == 'test'
    assert not (a.teacher or a.reduce_zero_label or a.entropy or a.revise_checkpoint_key) and a.max_images is None
    a = tool.parse_args(['cfg.py', 'ck.pth', '--out-dir', 'o', '--split', 'val', '--ratio', '0.2', '0.5', '--label-ratio', '0.2', '--teacher',
                         '--reduce-zero-label', '--entropy', '--max-images', '7', '--gpu-id', '1', '--cfg-options', 'a=1'])
    assert (a.config, a.checkpoint, a.split, a.ratio, a.label_ratio, a.max_images, a.gpu_id) == ('cfg.py', 'ck.pth', 'val', [0.2, 0.5], 0.2, 7, 1)
    assert a.teacher and a.reduce_zero_label and a.entropy
    for bad in (['--out-dir', 'o'], ['cfg.py', '--out-dir', 'o'], ['--synthetic', '2'], ['--synthetic', '0', '--out-dir', 'o'],
                ['--synthetic', '2', '--out-dir', 'o', '--ratio', '1.0', '--label-ratio', '1.0'],
                ['--synthetic', '2', '--out-dir', 'o', '--ratio', '-0.1', '0.5'],
                ['--synthetic', '2', '--out-dir', 'o', '--ratio', '0.2', '0.4'],                       # the default label ratio 0.5 is not among them
                ['--synthetic', '2', '--out-dir', 'o', '--label-ratio', '0.25'],
                ['--synthetic', '2', '--out-dir', 'o', '--max-images', '0']):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_teacher_key_revision():
    from pfst_amd.evaluation import revise_checkpoint_keys, teacher_checkpoint_keys
    sd = {'module.model.backbone.conv1.weight': 1, 'module.ema_model.backbone.conv1.weight': 2, 'ema_model.decode_head.bn.running_mean': 3,
          'model.decode_head.bn.running_mean': 4, 'model.decode_head.ema_model.x': 5, 'optimizer_step': 6}
    assert dict(teacher_checkpoint_keys(sd)) == {'backbone.conv1.weight': 2, 'decode_head.bn.running_mean': 3}
    student = revise_checkpoint_keys(sd)                                 # unchanged behaviour of the student's revision
    assert student['backbone.conv1.weight'] == 1 and student['decode_head.bn.running_mean'] == 4
    with pytest.raises(ValueError, match='ema_model'):
        teacher_checkpoint_keys({'backbone.conv1.weight': 1})


def test_second_stage_command_trains_on_the_written_label_maps(tmp_path):
    """the README's second-stage command: `tools/train.py CONFIG --supervised` reads the config's data.train.source entry, so that entry is
    pointed at the target tiles and at the written PNGs.  What the supervised run's dataset then yields is the pseudo-label map: class /
    255 from files written in annotation space (--reduce-zero-label) and read with reduce_zero_label=True."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from predict import write_label_png
    from pfst_amd.data import ISPRS_PALETTE, TileFolder, build_dataset
    rng = np.random.RandomState(0)
    for d in ('src/img', 'src/ann', 'trg/img', 'pseudo/ann'):
        os.makedirs(tmp_path / d)
    pred = rng.randint(0, 6, size=(16, 20)).astype(np.uint8)
    keep = rng.rand(16, 20) < 0.5
    Image.fromarray(rng.randint(0, 255, size=(16, 20, 3)).astype(np.uint8)).save(tmp_path / 'trg/img/tile_a.png')
    Image.fromarray(rng.randint(0, 255, size=(16, 20, 3)).astype(np.uint8)).save(tmp_path / 'src/img/other.png')
    write_label_png(str(tmp_path / 'src/ann/other.png'), np.zeros((16, 20), np.uint8), ISPRS_PALETTE)
    # the tool's annotation-space file of the tile: pred + 1 where kept, 0 where ignored
    write_label_png(str(tmp_path / 'pseudo/ann/tile_a.png'), np.where(keep, pred + 1, 0).astype(np.uint8), [[0, 0, 0]] + ISPRS_PALETTE)
    pipe = ("[dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', reduce_zero_label=True), "
            "dict(type='Normalize', mean=[0, 0, 0], std=[1, 1, 1], to_rgb=True), dict(type='DefaultFormatBundle'), "
            "dict(type='Collect', keys=['img', 'gt_semantic_seg'])]")
    cfg_file = tmp_path / 'uda_cfg.py'
    cfg_file.write_text(f"pipe = {pipe}\n"
                        f"data = dict(samples_per_gpu=1, train=dict(type='UDADataset', "
                        f"source=dict(type='ISPRSDataset', data_root={str(tmp_path / 'src')!r}, img_dir='img', ann_dir='ann', pipeline=pipe), "
                        f"target=dict(type='ISPRSDataset', data_root={str(tmp_path / 'trg')!r}, img_dir='img', ann_dir=None, pipeline=pipe)))\n"
                        "uda = dict(type='PFGST')\n")
    args = train_cli.parse_args([str(cfg_file), '--supervised', '--cfg-options', f"data.train.source.data_root={tmp_path / 'trg'}",
                                 'data.train.source.img_dir=img', f"data.train.source.ann_dir={tmp_path / 'pseudo/ann'}"])
    cfg = train_cli.load_cfg(args)
    assert 'uda' not in cfg and cfg.data.train['img_dir'] == 'img' and cfg.data.train['ann_dir'] == str(tmp_path / 'pseudo/ann')
    ds = build_dataset(cfg.data.train)
    assert type(ds) is TileFolder and len(ds) == 1 and ds.img_infos[0]['filename'] == 'tile_a.png'
    got = ds[0]['gt_semantic_seg'].numpy().reshape(16, 20)
    assert np.array_equal(got, np.where(keep, pred, 255))
    # an override of data.train.target.* does NOT reach a supervised run: it still reads the source entry
    args = train_cli.parse_args([str(cfg_file), '--supervised', '--cfg-options', f"data.train.target.ann_dir={tmp_path / 'pseudo/ann'}"])
    assert train_cli.load_cfg(args).data.train['data_root'] == str(tmp_path / 'src')
