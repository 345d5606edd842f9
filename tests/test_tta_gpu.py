"""Multi-scale + flip test-time augmentation on the GPU: pfst_tta_accumulate / pfst_tta_finalize bit for bit against the chain they fuse,
aug_test (per-view and paired-flip forwards) against the oracle, and tools/test.py --aug-test end to end."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain(src, mid_hw, ori_hw, hflip, vflip, acc, slide):
    """what aug_test ran per view before the fused kernel: resize -> resize -> softmax -> flip -> axpy"""
    from pfst_amd import hip_ops as ops
    p = src if slide else ops.resize_bilinear(src, mid_hw)
    if tuple(mid_hw) != tuple(ori_hw):
        p = ops.resize_bilinear(p, ori_hw)
    p = ops.softmax_nchw(p)
    if hflip or vflip:
        p = ops.flip_planes(p, horizontal=hflip, vertical=vflip)
    if acc is None:
        return p
    ops.axpy_(acc, p)
    return acc


CASES = [  # (C, src hw, mid hw, ori hw, slide)
    (6, (32, 32), (128, 128), (256, 256), False),       # input != ori: two resizes, the second the x2 kernel
    (6, (25, 38), (100, 150), (100, 150), False),       # ori equal to the input: one resize
    (6, (26, 19), (101, 75), (100, 150), False),        # ori 100 x 150 (not a multiple of 8) from an odd input grid
    (2, (16, 24), (64, 96), (50, 75), False),
    (19, (12, 20), (48, 80), (100, 150), False),
    (6, (96, 80), (96, 80), (128, 112), True),           # slide mode: the window average at input size, one resize
    (19, (40, 40), (40, 40), (40, 40), True),            # nothing to resize
]


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('flips', [(False, False), (True, False), (False, True), (True, True)])
def test_tta_accumulate_is_bitwise_the_chain(case, flips):
    from pfst_amd import hip_ops as ops
    C, shw, mhw, ohw, slide = case
    g = torch.Generator().manual_seed(C * 131 + shw[0] + 7 * flips[0] + 11 * flips[1])
    srcs = [(torch.randn(2, C, *shw, generator=g) * 4).cuda() for _ in range(3)]
    srcs[1] = torch.randn(2, C + 1, *shw, generator=g).cuda()[:, :C]          # a channel slice: batch stride != C * H * W
    ref = None
    got = torch.full((2, C, *ohw), float('nan'), device='cuda')
    for i, s in enumerate(srcs):
        hf, vf = flips if i != 1 else (not flips[0], flips[1])
        ref = _chain(s, mhw, ohw, hf, vf, ref, slide)
        ops.tta_accumulate_(got, s, mhw, hf, vf, accumulate=i > 0)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_tta_accumulate_refuses_too_many_classes():
    from pfst_amd import hip_ops as ops
    from pfst_amd._lib import PfstHipError
    src = torch.zeros(1, ops.TTA_MAX_C + 1, 4, 4, device='cuda')
    with pytest.raises(PfstHipError):
        ops.tta_accumulate_(torch.zeros(1, ops.TTA_MAX_C + 1, 8, 8, device='cuda'), src, (8, 8))


@pytest.mark.parametrize('shape', [(2, 6, 64, 96), (1, 19, 37, 41), (1, 2, 1, 3)])
def test_tta_finalize_labels_are_div_then_argmax(shape):
    from pfst_amd import hip_ops as ops
    g = torch.Generator().manual_seed(shape[2])
    acc = torch.rand(*shape, generator=g).cuda() * 12
    for views in (1, 3, 12):
        ref = ops.argmax_nchw(ops.div_scalar_(acc.clone(), views))
        assert torch.equal(ops.tta_finalize(acc, views), ref)
    # a tie made by the rounding of the division: a < b but a / 3 == b / 3 -- the first class wins, as with div_scalar_ + argmax_nchw
    a, two = torch.tensor(1.75), torch.tensor(2.0)
    while float(a / 3) != float(torch.nextafter(a, two) / 3):             # in [1.5, 2) the quotients are closer than their ulp
        a = torch.nextafter(a, two)
    b = torch.nextafter(a, two)
    assert float(a) < float(b) and float(a / 3) == float(b / 3)
    tie = torch.zeros(1, 4, 2, 4)
    tie[:, 1], tie[:, 3] = a, b
    tie = tie.cuda()
    assert int(ops.argmax_nchw(tie).max()) == 3                                # undivided, class 3 is larger
    lab = ops.tta_finalize(tie, 3)
    assert torch.equal(lab, ops.argmax_nchw(ops.div_scalar_(tie.clone(), 3))) and int(lab.max()) == 1


def _model(test_cfg):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_eval_gpu import _eval_model_and_state
    return _eval_model_and_state(test_cfg)


def _views(base, scales, flips_per_scale):
    """plain views resized to each scale, then flipped: images + metas as the pipeline makes them"""
    imgs, metas = [], []
    H, W = base.shape[2:]
    for si, s in enumerate(scales):
        plain = base if s == (H, W) else F.interpolate(base, size=s, mode='bilinear', align_corners=False)
        for d in flips_per_scale:
            img = plain if d is None else plain.flip(3 if d == 'horizontal' else 2)
            imgs.append(img.contiguous())
            metas.append([dict(ori_shape=(H, W, 3), flip=d is not None, flip_direction=d or 'horizontal', scale_index=si,
                               flip_permutes=True)] * base.shape[0])
    return imgs, metas


@pytest.mark.parametrize('mode', ['whole', 'slide'])
def test_aug_test_paired_flips_against_the_oracle(mode):
    """aug_test in both modes against oracle.aug_test (tolerances of test_eval_gpu's aug test); the paired-flip forward of pipeline items
    (batch 1 + D) within the same bound of the per-view forwards; a duplicated direction adds its view twice, in order"""
    test_cfg = dict(mode='whole') if mode == 'whole' else dict(mode='slide', crop_size=(96, 96), stride=(64, 64))
    model, student, O = _model(test_cfg)
    seg = model.get_model()
    g = torch.Generator().manual_seed(21)
    base = torch.randn(1, 3, 112, 128, generator=g)
    dirs = [None, None, 'horizontal', 'vertical']                 # flip=True, directions [h, v]: plain, plain, h-flip, v-flip
    imgs, metas = _views(base, [(112, 128), (144, 160)], dirs)
    with torch.no_grad():
        ref_pred, ref_prob = O.aug_test(student, [i.clone() for i in imgs], metas, test_cfg)
    paired = seg.aug_test_labels([i.cuda() for i in imgs], metas)
    per_view_metas = [[dict(m[0], flip_permutes=False)] for m in metas]
    per_view = seg.aug_test_labels([i.cuda() for i in imgs], per_view_metas)
    out, st = model([i.cuda() for i in imgs], metas, return_loss=False)
    assert st == {} and len(out) == 1 and out[0].shape == (112, 128)
    assert torch.equal(torch.from_numpy(out[0]), paired[0].cpu())
    for pred in (paired, per_view):
        assert (pred.cpu().long() != ref_pred).float().mean() < 2e-3
    # the sums themselves: per-view vs the oracle, paired vs per-view
    acc_pv = None
    acc_pr = None
    for s in range(2):
        acc_pr = seg.aug_test_scale_(imgs[4 * s].cuda(), metas[4 * s], dirs, acc_pr)
        for v in range(4 * s, 4 * s + 4):
            src, mid = seg._tta_forward(imgs[v].cuda())
            acc_pv = seg._tta_add(acc_pv, src, mid, (112, 128), dirs[v % 4])
    tol = 1e-3 * float(ref_prob.max()) * 8
    assert float((acc_pv.cpu() / 8 - ref_prob).abs().max()) < tol
    assert float((acc_pr.cpu() - acc_pv.cpu()).abs().max()) < tol
    # order and multiplicity: the duplicated plain view counts twice -- the same as the plain view weighted 2 in the oracle's sum
    with torch.no_grad():
        p_plain = O.inference_probs(student, imgs[0].clone(), metas[0], test_cfg)
        p_h = O.inference_probs(student, imgs[2].clone(), metas[2], test_cfg)
    single = seg.aug_test_scale_(imgs[0].cuda(), metas[0], [None, None, 'horizontal'])
    assert float((single.cpu() - (2 * p_plain + p_h)).abs().max()) < 3 * 1e-3 * float(p_plain.max())
    one = seg.aug_test_scale_(imgs[0].cuda(), metas[0], [None, 'horizontal'])
    assert not torch.equal(one, single)


def test_test_cli_aug_test_end_to_end(tmp_path):
    """tools/test.py --aug-test on a small tile folder: eval_multi_scale.json with the ratios and the view count, and the mIoU of the
    oracle's aug_test over the same views"""
    import json
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test as test_cli
    from helpers import uda_cfg
    from test_data_pipeline_cpu import TEST, _tile
    from pfst_amd.data import TileFolder
    from pfst_amd.evaluation import total_area_to_metrics
    model, student, O = _model(None)
    os.makedirs(tmp_path / 'img'), os.makedirs(tmp_path / 'ann')
    for i in range(2):
        img, seg = _tile(40 + i, 96)
        Image.fromarray(img).save(tmp_path / 'img' / f't{i}.png')
        Image.fromarray(seg).save(tmp_path / 'ann' / f't{i}.png')
    test_pl = [TEST[0], dict(TEST[1], img_scale=(96, 96))]
    ds = dict(type='ISPRSDataset', data_root=str(tmp_path), img_dir='img', ann_dir='ann', gt_seg_map_loader_cfg=dict(reduce_zero_label=True),
              pipeline=test_pl)
    model_cfg = uda_cfg()['model']
    (tmp_path / 'cfg.py').write_text('model = %r\ndata = %r\n' % (model_cfg, dict(test=ds, val=ds)))
    torch.save({'state_dict': {'model.' + k: v.clone() for k, v in student.items()}}, tmp_path / 'ck.pth')      # a PFGST checkpoint's layout
    work = tmp_path / 'work'
    res = test_cli.main([str(tmp_path / 'cfg.py'), str(tmp_path / 'ck.pth'), '--aug-test', '--revise-checkpoint-key', '--work-dir', str(work)])
    out = json.load(open(work / 'eval_multi_scale.json'))
    assert out['img_ratios'] == [0.5, 0.75, 1.0, 1.25, 1.5, 1.75] and out['views'] == 12 and out['flip'] is True
    assert out['metric']['mIoU'] == res['mIoU'] and not (work / 'eval.json').exists()
    # the oracle over the same views
    pl = copy.deepcopy(test_pl)
    from pfst_amd.evaluation import enable_aug_test
    enable_aug_test(pl)
    folder = TileFolder(dict(ds, pipeline=pl), test_mode=True)
    hist = np.zeros((3, 6))
    for i in range(len(folder)):
        item = folder[i]
        with torch.no_grad():
            pred, _ = O.aug_test(student, [v[None] for v in item['img']], [[m] for m in item['img_metas']], dict(mode='whole'))
        gt = folder.gt_seg_map(i)
        p, lab = pred[0].numpy(), gt
        keep = lab != 255
        p, lab = p[keep], lab[keep]
        hist[0] += np.bincount(lab[p == lab], minlength=6)
        hist[1] += np.bincount(p, minlength=6)
        hist[2] += np.bincount(lab, minlength=6)
    inter, pred_a, lab_a = hist
    m = total_area_to_metrics(inter, pred_a + lab_a - inter, pred_a, lab_a)
    assert abs(100 * float(np.nanmean(m['IoU'])) - res['mIoU']) < 0.5
