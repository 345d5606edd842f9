"""Offline pseudo-labels on the GPU: the three kernels of csrc/entropy_labels.hip against the float64 restatement that
tests/test_pseudo_labels_cpu.py pins to the reference, the radix select against np.sort of the device's own entropies (bit for bit), the
identity-size golden case, and tools/pseudo_label.py end to end.

Every case asserts, in float64 on the CPU, the conditions under which its comparison is exact:
  (a) the two largest probabilities of every pixel lie >= 1e-5 apart: the device's arg-max (of the rounded probabilities in mode 0, of the
      logits in mode 1) and the float64 arg-max coincide, so the per-class pixel sets are equal;
  (b) for the label test every threshold is the midpoint of a gap >= 1e-4 between consecutive float64 order statistics of the loader's
      entropy: with entropies within 1e-5 of float64 no pixel can fall on the other side -- no exclusions."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pseudo_label_oracle as oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENT_TOL = 1e-5          # 5 x the worst float32-vs-float64 error of the reference's own torch computation on these shapes (1.9e-6 at C = 33)
RATIOS = [0.0, 0.2, 0.5, 0.99]

# name: (C, (h, w), (H, W), seed) -- logits N(0, 3^2), N = 2; the seeds are ones for which conditions (a) and (b) hold (each test asserts them)
CASES = {
    'x4': (6, (19, 17), (76, 68), 2),          # the head's ratio, ragged against the 256-thread blocks
    'x8': (6, (17, 18), (136, 144), 1),        # the auxiliary head's ratio, several workgroups per image
    'g33': (33, (7, 9), (30, 37), 4),          # non-integer ratio, C > 8: the generic form
    'g2': (2, (7, 9), (30, 37), 4),            # non-integer ratio, two classes
    'id': (6, (40, 36), (40, 36), 0),          # H == h: identity
}


def make_logits(name):
    C, lo, _, seed = CASES[name]
    return (torch.randn(2, C, *lo, generator=torch.Generator().manual_seed(seed)) * 3).contiguous()


def reference(logits, size):
    """the float64 side of a case, computed once: both entropies and arg-maxima, the top-2 gap"""
    z = oracle.upsample64(logits.numpy(), size)
    p = oracle.softmax64(z)
    e0, q0 = oracle.hook_entropy(p)
    e1, q1 = oracle.loader_entropy(z, p)
    return dict(z=z, p=p, e0=e0, q0=q0, e1=e1, q1=q1, gap=oracle.top2_gap(p))


_REF = {}


def case(name):
    if name not in _REF:
        logits = make_logits(name)
        _REF[name] = (logits, CASES[name][2], reference(logits, CASES[name][2]))
    return _REF[name]


def device_sort_thresholds(ent, pred, ratios, C):
    """np.sort of the DEVICE's entropies per class -> float32 table, n_c (the select must reproduce it bit for bit)"""
    return oracle.thresholds(np.asarray(ent, np.float32), np.asarray(pred), ratios, C)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1. entropy and arg-max
@pytest.mark.parametrize('name', list(CASES))
def test_entropy_and_prediction_against_float64(name):
    from pfst_amd import hip_ops as ops
    logits, size, ref = case(name)
    assert ref['gap'].min() >= 1e-5, f'condition (a) fails for this seed: {ref["gap"].min()}'
    # the reference's own float32 error on this shape, for the record: torch's resize, softmax and entropy in float32 on the CPU
    up = F.interpolate(logits, size=size, mode='bilinear', align_corners=False) if tuple(logits.shape[2:]) != tuple(size) else logits
    pr = F.softmax(up, dim=1)
    ref32 = (-pr * torch.log(pr)).sum(dim=1).numpy()
    print(f'{name}: float32 reference |H - H64| max {np.abs(ref32 - ref["e0"]).max():.3g}')
    for mode, ek, qk in ((0, 'e0', 'q0'), (1, 'e1', 'q1')):
        ent, pred = ops.entropy_upsample(logits.cuda(), size, mode)
        ent, pred = ent.cpu().numpy(), pred.cpu().numpy()
        err = np.abs(ent - ref[ek]).max()
        print(f'{name} mode {mode}: device |H - H64| max {err:.3g}')
        assert ent.dtype == np.float32 and not np.signbit(ent).any() and not np.isnan(ent).any()
        assert err <= ENT_TOL
        assert np.array_equal(pred, ref[qk])
        only_e, none = ops.entropy_upsample(logits.cuda(), size, mode, want_pred=False)
        none2, only_p = ops.entropy_upsample(logits.cuda(), size, mode, want_entropy=False)
        assert none is None and none2 is None and same_bits(only_e.cpu().numpy(), ent) and np.array_equal(only_p.cpu().numpy(), pred)


def test_saturated_pixels_give_plus_zero():
    """one class 200 above the rest: p = (1, 0, ...), every term 0 -> +0 (never -0 or NaN), key 0 in the histogram"""
    from pfst_amd import hip_ops as ops
    for C in (6, 11):
        z = torch.zeros(1, C, 5, 7)
        z[:, 2] = 200.0
        for mode in (0, 1):
            ent, pred = ops.entropy_upsample(z.cuda(), (20, 28), mode)
            assert (ent.cpu().numpy().view(np.uint32) == 0).all() and (pred == 2).all()
        hist = torch.zeros(C, 256, dtype=torch.int64, device='cuda')
        ops.entropy_class_hist(z.cuda(), (20, 28), 24, 8, hist)
        want = np.zeros((C, 256), np.int64)
        want[2, 0] = 20 * 28
        assert np.array_equal(hist.cpu().numpy(), want)


def test_register_and_generic_form_give_the_same_bits():
    """the x4 logits with three more classes at -1e30 (probability exactly 0: they add 0 to the sum and nothing to either entropy) go through
    the generic form (C = 9); entropy and arg-max must be those of the register form (C = 6), bit for bit, in both modes -- and so must the
    histogram and the labels"""
    from pfst_amd import hip_ops as ops
    logits, size, _ = case('x4')
    d6 = logits.cuda()
    d9 = torch.cat([d6, torch.full((2, 3, 19, 17), -1e30, device='cuda')], 1).contiguous()
    for mode in (0, 1):
        e6, q6 = ops.entropy_upsample(d6, size, mode)
        e9, q9 = ops.entropy_upsample(d9, size, mode)
        assert torch.equal(e6.view(torch.int32), e9.view(torch.int32)) and torch.equal(q6, q9)
    h6 = ops.entropy_class_hist(d6, size, 24, 8, torch.zeros(6, 256, dtype=torch.int64, device='cuda'))
    h9 = ops.entropy_class_hist(d9, size, 24, 8, torch.zeros(9, 256, dtype=torch.int64, device='cuda'))
    assert torch.equal(h6, h9[:6]) and int(h9[6:].sum()) == 0
    thr = torch.full((9,), 0.7, device='cuda')
    l6, c6 = ops.entropy_pseudo_label(d6, size, thr[:6].contiguous())
    l9, c9 = ops.entropy_pseudo_label(d9, size, thr)
    assert torch.equal(l6, l9) and torch.equal(c6, c9[:6]) and 0 < int(c6[:, 1].sum()) < int(c6[:, 0].sum())


# ------------------------------------------------------------------------------------------------ 2. the select is exact
def select_case(tiles, C, ratios=RATIOS):
    """tiles: [(logits, size)] -> (table, n_c) of ClassEntropyThresholds and of np.sort over the device's own mode-0 entropies"""
    from pfst_amd import hip_ops as ops
    from pfst_amd.pseudo_labels import ClassEntropyThresholds
    acc = ClassEntropyThresholds(C)
    ents, preds = [], []
    for logits, size in tiles:
        acc.add(logits.cuda(), size)
        e, q = ops.entropy_upsample(logits.cuda(), size, 0)
        ents.append(e.cpu().numpy().reshape(-1))
        preds.append(q.cpu().numpy().reshape(-1))
    table, n_c = acc.thresholds(ratios)
    want, n_want = device_sort_thresholds(np.concatenate(ents), np.concatenate(preds), ratios, C)
    return table, n_c, want, n_want, np.concatenate(ents), np.concatenate(preds)


@pytest.mark.parametrize('name', ['x8', 'x4', 'g33', 'g2'])
def test_thresholds_equal_sort_of_the_device_entropies(name):
    logits, size, _ = case(name)
    table, n_c, want, n_want, _, _ = select_case([(logits, size)], CASES[name][0])
    assert table.dtype == np.float32 and table.shape == (len(RATIOS), CASES[name][0])
    assert np.array_equal(n_c, n_want) and n_c.sum() == 2 * size[0] * size[1]
    assert same_bits(table, want)


def test_rank_inside_a_tie_run():
    """logits constant over 5 x 5 low-resolution blocks, x4: most pixels interpolate between equal cells, few distinct entropies"""
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(2, 6, 4, 4, generator=g) * 3).repeat_interleave(5, 2).repeat_interleave(5, 3).contiguous()
    table, n_c, want, n_want, ent, pred = select_case([(logits, (80, 80))], 6)
    distinct = np.unique(ent.view(np.uint32)).size
    print('distinct entropies', distinct, 'of', ent.size)
    assert ent.size == 12800 and distinct < ent.size // 2
    # rank k of some (ratio, class) lies strictly inside a run of equal keys
    inside = 0
    for c in range(6):
        s = np.sort(ent[pred == c])
        for r in RATIOS:
            k = int(s.size * r)
            inside += int(s.size > 2 and 0 < k < s.size - 1 and s[k - 1] == s[k] == s[k + 1])
    assert inside > 0
    assert np.array_equal(n_c, n_want) and same_bits(table, want)


def test_empty_class_and_single_pixel_class():
    g = torch.Generator().manual_seed(6)
    logits = (torch.randn(2, 6, 12, 10, generator=g) * 3).contiguous()
    logits[:, 5] = -60.0                        # class 5 is never predicted
    logits[:, 4] = -60.0
    logits[1, 4, 7, 3] = 60.0                   # class 4 at exactly one pixel (identity size: one cell is one pixel)
    table, n_c, want, n_want, ent, pred = select_case([(logits, (12, 10))], 6)
    assert n_c[5] == 0 and n_c[4] == 1 and np.array_equal(n_c, n_want)
    assert (table[:, 5] == 0).all() and same_bits(table, want)
    assert same_bits(table[:, 4], np.repeat(ent[pred == 4], len(RATIOS)))


def test_two_adds_of_different_tile_shapes():
    a, size_a, _ = case('x4')
    g = torch.Generator().manual_seed(8)
    b = (torch.randn(3, 6, 7, 9, generator=g) * 3).contiguous()
    table, n_c, want, n_want, _, _ = select_case([(a, size_a), (b, (30, 37))], 6)
    assert n_c.sum() == 2 * 76 * 68 + 3 * 30 * 37 and np.array_equal(n_c, n_want)
    assert same_bits(table, want)


def test_histogram_paths_agree_with_numpy():
    """every form of the histogram kernel -- registers / generic classes, LDS / global counters -- with and without a prefix"""
    from pfst_amd import hip_ops as ops
    for name, settings in (('x4', [(21, 11), (10, 11), (0, 10), (19, 13)]), ('g33', [(24, 8), (16, 8), (21, 11), (10, 11)])):
        logits, size, _ = case(name)
        C = CASES[name][0]
        d = logits.cuda()
        e, q = ops.entropy_upsample(d, size, 0)
        keys, pred = e.cpu().numpy().reshape(-1).view(np.uint32).astype(np.uint64), q.cpu().numpy().reshape(-1).astype(np.int64)
        for shift, bits in settings:
            prefix = None
            if shift + bits < 32:                 # the most frequent higher bits of each class as its prefix
                hi = keys >> np.uint64(shift + bits)
                prefix = np.array([np.bincount(hi[pred == c].astype(np.int64)).argmax() if (pred == c).any() else 0 for c in range(C)], np.uint32)
            live = np.ones(keys.size, bool) if prefix is None else (keys >> np.uint64(shift + bits)) == prefix.astype(np.uint64)[pred]
            want = np.zeros((C, 1 << bits), np.int64)
            np.add.at(want, (pred[live], ((keys[live] >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)), 1)
            hist = torch.zeros(C, 1 << bits, dtype=torch.int64, device='cuda')
            pre = None if prefix is None else torch.from_numpy(prefix.view(np.int32).copy()).cuda()
            ops.entropy_class_hist(d, size, shift, bits, hist, pre)
            ops.entropy_class_hist(d, size, shift, bits, hist, pre)                       # ADDS: twice the counts
            assert np.array_equal(hist.cpu().numpy(), 2 * want), (name, shift, bits)
            assert want.sum() > 0
    with pytest.raises(ValueError):
        ops.entropy_class_hist(d, size, 24, 8, torch.zeros(C, 256, dtype=torch.int64, device='cuda'), torch.zeros(C, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        ops.entropy_class_hist(d, size, 24, 8, torch.zeros(C, 128, dtype=torch.int64, device='cuda'))


# ------------------------------------------------------------------------------------------------ 3. thresholds against float64
@pytest.mark.parametrize('name', ['x8', 'x4', 'g33', 'g2'])
def test_thresholds_against_float64(name):
    from pfst_amd.pseudo_labels import ClassEntropyThresholds
    logits, size, ref = case(name)
    C = CASES[name][0]
    assert ref['gap'].min() >= 1e-5
    table, n_c = ClassEntropyThresholds(C).add(logits.cuda(), size).thresholds(RATIOS)
    t64, n64 = oracle.thresholds(ref['e0'], ref['q0'], RATIOS, C)
    # equal class sets (a): an order statistic moves at most as far as the largest perturbation of the values
    print(f'{name}: |thr - thr64| max {np.abs(table - t64).max():.3g}')
    assert np.array_equal(n_c, n64) and np.abs(table - t64).max() <= ENT_TOL


# ------------------------------------------------------------------------------------------------ 4. labels
@pytest.mark.parametrize('name', ['x8', 'x4', 'g33', 'g2', 'id'])
def test_labels_exact_against_float64(name):
    from pfst_amd.pseudo_labels import label_maps
    logits, size, ref = case(name)
    C = CASES[name][0]
    assert ref['gap'].min() >= 1e-5
    thr, ok = oracle.midpoint_thresholds(ref['e1'], ref['q1'], 0.5, C, 1e-4)
    assert ok, 'condition (b) fails for this seed'
    d = logits.cuda()
    for ann in (False, True):
        want, cnt = oracle.labels(ref['e1'], ref['q1'], thr.astype(np.float64), annotation_space=ann)
        lab, counts = label_maps(d, size, thr, annotation_space=ann)
        assert lab.dtype == torch.uint8 and np.array_equal(lab.cpu().numpy(), want)
        assert np.array_equal(counts.cpu().numpy(), cnt) and 0 < cnt[:, 1].sum() < cnt[:, 0].sum()
        label_maps(d, size, thr, annotation_space=ann, counts=counts)                         # counts are ADDED to
        assert np.array_equal(counts.cpu().numpy(), 2 * cnt)
    # a threshold of 0 keeps nothing of that class, one above ln C everything
    mixed = np.where(np.arange(C) % 2 == 0, 0.0, math.log(C) + 0.1).astype(np.float32)
    lab, counts = label_maps(d, size, mixed)
    lab, counts = lab.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(lab, np.where(ref['q1'] % 2 == 0, 255, ref['q1']).astype(np.uint8))
    assert (counts[::2, 1] == 0).all() and np.array_equal(counts[1::2, 1], counts[1::2, 0])
    assert np.array_equal(counts[:, 0], np.bincount(ref['q1'].reshape(-1), minlength=C))


# ------------------------------------------------------------------------------------------------ 5. run to run, launch by launch
def test_runs_are_bit_identical_and_batching_does_not_matter():
    from pfst_amd import hip_ops as ops
    from pfst_amd.pseudo_labels import ClassEntropyThresholds, label_maps
    assert not ops.is_deterministic()
    logits, size, _ = case('x8')
    d = logits.cuda()
    runs = []
    for _ in range(2):
        acc = ClassEntropyThresholds(6).add(d, size)
        table, n_c = acc.thresholds(RATIOS)
        lab, counts = label_maps(d, size, table[2])
        runs.append((table.copy(), n_c.copy(), lab.cpu().numpy(), counts.cpu().numpy(), acc.class_hist(10, 11, np.full(6, 0x1FC, np.uint32))))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    one = ClassEntropyThresholds(6)
    for i in range(2):
        one.add(d[i:i + 1], size)
    together = ClassEntropyThresholds(6).add(d, size)
    launches = torch.zeros(6, 2048, dtype=torch.int64, device='cuda')
    for i in range(2):
        ops.entropy_class_hist(d[i:i + 1].contiguous(), size, 21, 11, launches)
    h = together.class_hist(21, 11)
    assert np.array_equal(h, one.class_hist(21, 11)) and np.array_equal(h, launches.cpu().numpy()) and h.sum() == 2 * size[0] * size[1]
    assert same_bits(one.thresholds(RATIOS)[0], runs[0][0])
    assert [t for _, _, t in one.blocks()] == [[0, 1]] and one.tile(1)[0].shape == (1, 6, 17, 18)
    assert torch.equal(one.tile(1)[0], d[1:2])


def test_refusals():
    from pfst_amd.pseudo_labels import ClassEntropyThresholds
    logits, size, _ = case('x4')
    acc = ClassEntropyThresholds(6, max_bytes=1 << 20)
    with pytest.raises(ValueError, match='classes'):
        acc.add(torch.zeros(1, 5, 4, 4, device='cuda'), (16, 16))
    with pytest.raises(ValueError, match='no tiles'):
        acc.thresholds([0.5])
    with pytest.raises(MemoryError, match='--max-images'):
        acc.add(torch.zeros(1, 6, 256, 256, device='cuda'), (1024, 1024))
    acc.add(logits.cuda(), size)
    # one add() that brings more than a block is gathered by a concatenation of its own size: 100 tiles of 6 x 8 x 8 are 150 KB, twice over
    # they do not fit in 250 KB although the copy and one 64-tile block would
    small = ClassEntropyThresholds(6, max_bytes=250 * 1024)
    with pytest.raises(MemoryError, match='--max-images'):
        small.add(torch.zeros(100, 6, 8, 8, device='cuda'), (32, 32))
    small.add(torch.zeros(60, 6, 8, 8, device='cuda'), (32, 32))
    for bad in ([1.0], [-0.01], [0.5, 2]):
        with pytest.raises(ValueError, match=r'outside \[0, 1\)'):
            acc.thresholds(bad)


# ------------------------------------------------------------------------------------------------ 6. the reference's own numbers
def test_identity_size_golden_case(golden_dir):
    from pfst_amd import hip_ops as ops
    from pfst_amd.pseudo_labels import ClassEntropyThresholds, label_maps
    g = np.load(os.path.join(golden_dir, 'pseudo_labels.npz'))
    logits, ratios, table_ref, labels_ref = torch.from_numpy(g['logits']), [float(r) for r in g['ratios']], g['thresholds'], g['labels']
    N, C, H, W = logits.shape
    ref = reference(logits, (H, W))
    d = logits.cuda()
    # thresholds: the order statistics of the device's entropies once the pixel the reference dropped is removed ...
    e, q = ops.entropy_upsample(d, (H, W), 0)
    dropped, n_ref = oracle.thresholds(e.cpu().numpy(), q.cpu().numpy(), ratios, C, drop=g['dropped'])
    print('golden thresholds: |device order statistic - reference| max', np.abs(dropped - table_ref).max())
    assert n_ref.sum() == N * H * W - 1 and np.abs(dropped - table_ref).max() <= ENT_TOL
    # ... and the select over every pixel: one more value in one class moves a rank by at most one place
    table, n_c = ClassEntropyThresholds(C).add(d, (H, W)).thresholds(ratios)
    assert n_c.sum() == N * H * W
    ent, pred = e.cpu().numpy().reshape(-1), q.cpu().numpy().reshape(-1)
    for c in range(C):
        s = np.sort(ent[pred == c])
        for i, r in enumerate(ratios):
            k = int(s.size * r)
            assert s[max(k - 1, 0)] - ENT_TOL <= table_ref[i, c] <= s[min(k + 1, s.size - 1)] + ENT_TOL
            assert table[i, c] == s[k]
    # labels with the reference's thresholds; pixels that break (a) or lie within 1e-5 of their threshold are left out: at most 1 %
    thr = table_ref[ratios.index(float(g['label_ratio']))]
    lab, counts = label_maps(d, (H, W), thr)
    lab = lab.cpu().numpy()
    out = (ref['gap'] < 1e-5) | (np.abs(ref['e1'] - thr.astype(np.float64)[ref['q1']]) <= 1e-5)
    print('golden labels: excluded', int(out.sum()), 'of', out.size, '; differing among them', int((lab != labels_ref)[out].sum()))
    assert out.mean() <= 0.01 and np.array_equal(lab[~out], labels_ref[~out])
    assert int(counts[:, 0].sum()) == N * H * W and abs(int(counts[:, 1].sum()) - int((labels_ref != 255).sum())) <= int(out.sum())


# ------------------------------------------------------------------------------------------------ 7. the tool, end to end
def test_cli_synthetic_end_to_end(tmp_path):
    from pfst_amd.data import _read_label
    from pfst_amd.pipeline import reduce_zero_label
    from pfst_amd.pseudo_labels import ClassEntropyThresholds, collect, label_maps
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import pseudo_label as tool
    argv = ['--synthetic', '3', '--ratio', '0.2', '0.5', '--label-ratio', '0.5', '--entropy', '--reduce-zero-label', '--out-dir', str(tmp_path)]
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'tools', 'pseudo_label.py')] + argv
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    out = json.load(open(tmp_path / 'pseudo_labels.json'))
    assert out['images'] == 3 and out['stems'] == ['synthetic0', 'synthetic1', 'synthetic2'] and out['ratios'] == [0.2, 0.5]
    assert sorted(out['seconds']) == ['forward', 'labels', 'thresholds'] and out['reduce_zero_label'] is True
    # the same logits in process
    args = tool.parse_args(argv)
    cfg = tool.load_config(args)
    model, data = tool.build_model_and_data(args, cfg, torch.device('cuda'))
    C = cfg.model.decode_head.num_classes
    acc = ClassEntropyThresholds(C)
    assert collect(model, data, acc) == out['stems']
    table, n_c = acc.thresholds([0.2, 0.5])
    assert [out['thresholds']['thre@0.2'], out['thresholds']['thre@0.5']] == [[float(v) for v in row] for row in table]
    assert out['n_c'] == n_c.tolist() and sum(out['n_c']) == 3 * 128 * 128
    kept = 0
    for stem in out['stems']:
        logits, size = acc.tile(stem)
        want, _ = label_maps(logits, size, table[1])                                   # prediction space: class / 255
        got = reduce_zero_label(_read_label(os.path.join(tmp_path, stem + '.png')))     # LoadAnnotations(reduce_zero_label=True)
        assert got.shape == (128, 128) and np.array_equal(got, want[0].cpu().numpy())
        kept += int((got != 255).sum())
        ent = _read_label(os.path.join(tmp_path, stem + '_entropy.png'))
        assert ent.shape == (128, 128) and ent.dtype == np.uint8
    assert sum(out['kept']) == kept and sum(out['predicted']) == 3 * 128 * 128 and 0 < kept < 3 * 128 * 128
    assert all(k <= p for k, p in zip(out['kept'], out['predicted']))
    # the refusals of collect: several views, a resized tile
    item = data[0]
    with pytest.raises(ValueError, match='single-view'):
        collect(model, [dict(img=[item['img']], img_metas=[item['img_metas']])], ClassEntropyThresholds(C))
    with pytest.raises(ValueError, match='image grid'):
        collect(model, [dict(img=item['img'], img_metas=dict(filename='a.png', ori_shape=(64, 64, 3)))], ClassEntropyThresholds(C))
    with pytest.raises(ValueError, match='flipped'):
        collect(model, [dict(img=item['img'], img_metas=dict(filename='a.png', ori_shape=(128, 128, 3), flip=True))], ClassEntropyThresholds(C))
    whole, model.test_cfg = model.test_cfg, dict(mode='slide', crop_size=(64, 64), stride=(32, 32))
    try:
        with pytest.raises(NotImplementedError, match='slide'):
            collect(model, data, ClassEntropyThresholds(C))
    finally:
        model.test_cfg = whole
