#!/usr/bin/env python3
"""Golden vectors for OHEMPixelSampler behind the decode head's bilinear resize, produced by EXECUTING the reference's
core/seg/sampler/ohem_pixel_sampler.py and BaseDecodeHead.losses on CPU in fp32 through make_golden.py's loader (same rules: only seeded
inputs and the numbers the reference returns are stored; weight maps are bit-packed).

Cases (N = 2; every label map has a 255 region):
  x4r_thresh   19 x 17 -> 76 x 68, C =  6   thresh = 0.7, min_kept = 100: thresh wins
  x4r_sk       the same logits, labels mostly the arg-max, thresh = 0.3, min_kept = 1500: s[k] wins
  x8_topk       8 x  8 -> 64 x 64, C =  6   thresh = None, min_kept = 750, one CE term
  g19_sk       13 x  9 -> 50 x 37, C = 19   non-integer ratio; labels mostly the arg-max, thresh = 0.3, min_kept = 1500
  head_thresh  the x4r_thresh inputs through DepthwiseSeparableASPPHead.losses with a sampler and a seg_weight (which the sampler replaces)
  head_topk    the x8_topk inputs through FCNHead.losses, [CE(0.4, class weights), CE(0.2, loss_ce2)], thresh = None, min_kept = 800
The generator asserts what the tests rely on: no tie at the cut of a top-k case (the band holds the pixel at the cut alone), and at most 0.25 % of the valid
pixels inside the fp64 oracle's band around the cut (tests/ohem_oracle.py), none of which the fp32 path decides differently.

Usage:  python tests/golden/make_golden_ohem.py        (writes tests/golden/ohem_sampler.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, _load, load_reference  # noqa: E402
import ohem_oracle as O  # noqa: E402

N = 2
CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
CASES = {
    # name: (C, (h, w), (H, W), logits of, labels mostly the arg-max, thresh, min_kept)
    'x4r_thresh': (6, (19, 17), (76, 68), None, False, 0.7, 100),
    'x4r_sk': (6, (19, 17), (76, 68), 'x4r_thresh', True, 0.3, 1500),
    'x8_topk': (6, (8, 8), (64, 64), None, False, None, 750),
    'g19_sk': (19, (13, 9), (50, 37), None, True, 0.3, 1500),
}
HEADS = {
    'head_thresh': ('DepthwiseSeparableASPPHead', 'x4r_thresh', dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                    dict(thresh=0.7, min_kept=100)),
    'head_topk': ('FCNHead', 'x8_topk', [dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.4, class_weight=CW6),
                                         dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.2, loss_name='loss_ce2')],
                  dict(thresh=None, min_kept=800)),
}


def seeded_inputs():
    g = torch.Generator().manual_seed(4242)
    out = {}
    for name, (C, lo, hi, src, argmax, _, _) in CASES.items():
        logits = out[src][0] if src else torch.randn(N, C, *lo, generator=g) * 2
        label = torch.randint(0, C, (N, *hi), generator=g)
        if argmax:
            arg = O.upsample(logits, hi, torch.float64).argmax(1)
            label = torch.where(torch.rand(N, *hi, generator=g) < 0.9, arg, label)
        label[:, 5:14, 9:23] = 255
        out[name] = (logits, label.to(torch.uint8))
    return out


def check_case(name, logits, label, thresh, batch_kept, weight, coef=None):
    """what the tests rely on: the fp64 oracle's band is thin and the fp32 map agrees with it everywhere"""
    k64, valid = O.keys(logits, label, 255, thresh is not None, coef, dtype=torch.float64)
    if thresh is not None:
        w64, cut, _ = O.select_thresh(k64, valid, thresh, batch_kept)
        band = O.band_thresh(k64, valid, cut)
    else:
        w64, cut, m = O.select_topk(k64, valid, batch_kept)
        band = O.band_topk(k64, valid, cut, 1.0 if coef is None else max(coef))
        assert int(band.sum()) == 1, f'{name}: a tie (or nearly one) at the cut: {int(band.sum())} pixels within the band of the cut value'
    assert int(band.sum()) <= O.BAND_SHARE * int(valid.sum()), f'{name}: {int(band.sum())} pixels in the band'
    assert torch.equal(w64, weight), f'{name}: the fp32 reference and the fp64 oracle disagree on {int((w64 != weight).sum())} pixels'
    print(f'{name}: valid {int(valid.sum())} kept {int(weight.sum())} cut {cut!r} band {int(band.sum())}')
    return cut


def build_ref_head(ref, kind, loss_decode):
    common = dict(dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True), align_corners=False, loss_decode=loss_decode)
    if kind == 'FCNHead':
        return ref.builder.build_head(dict(type='FCNHead', in_channels=32, in_index=2, channels=16, num_convs=1, concat_input=False, **common))
    return ref.builder.build_head(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                                       c1_in_channels=8, c1_channels=4, **common))


def gen_ohem(ref):
    import types
    for pkg in ('rsiseg.core.seg', 'rsiseg.core.seg.sampler'):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    _load('rsiseg.core.seg.builder', 'rsiseg/core/seg/builder.py')
    _load('rsiseg.core.seg.sampler.base_pixel_sampler', 'rsiseg/core/seg/sampler/base_pixel_sampler.py')
    Sampler = _load('rsiseg.core.seg.sampler.ohem_pixel_sampler', 'rsiseg/core/seg/sampler/ohem_pixel_sampler.py').OHEMPixelSampler
    inputs = seeded_inputs()
    out = dict(cases=np.array(list(CASES)), heads=np.array(list(HEADS)))
    plain = build_ref_head(ref, 'FCNHead', dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))       # the samplers' context
    for name, (C, lo, hi, src, _, thresh, min_kept) in CASES.items():
        logits, label = inputs[name]
        up = ref.resize(input=logits, size=hi, mode='bilinear', align_corners=False)
        w = Sampler(plain, thresh=thresh, min_kept=min_kept).sample(up, label.long().unsqueeze(1))
        assert w.dtype == torch.float32 and bool(((w == 0) | (w == 1)).all())
        cut = check_case(name, logits, label, thresh, min_kept * N, w)
        if not src:
            out[name + '|logits'] = logits.numpy()
        out[name + '|label'] = label.numpy()
        out[name + '|weight_bits'] = np.packbits(w.numpy().astype(bool).reshape(-1))
        out[name + '|cut'] = np.array(cut, dtype=np.float64)                                        # the fp64 oracle's threshold / cut value
        out[name + '|kept'] = np.array(int(w.sum()), dtype=np.int64)
    g = torch.Generator().manual_seed(99)
    for name, (kind, src, loss_decode, opts) in HEADS.items():
        logits, label = inputs[src]
        head = build_ref_head(ref, kind, loss_decode)
        head.sampler = Sampler(head, **opts)
        z = logits.clone().requires_grad_()
        passed = torch.rand(N, *label.shape[-2:], generator=g)                                     # replaced by the sampler's map
        res = head.losses(z, label.long().unsqueeze(1), passed)
        sum(v for k, v in res.items() if k.startswith('loss')).backward()
        terms = loss_decode if isinstance(loss_decode, list) else [loss_decode]
        coef = [sum(t['loss_weight'] * (t.get('class_weight') or [1.0] * 6)[c] for t in terms) for c in range(6)]
        up = ref.resize(input=logits, size=tuple(label.shape[-2:]), mode='bilinear', align_corners=False)
        w = head.sampler.sample(up, label.long().unsqueeze(1))
        check_case(name, logits, label, opts['thresh'], opts['min_kept'] * N, w, coef)
        out[name + '|names'] = np.array(list(res))
        out[name + '|values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
        out[name + '|grad'] = z.grad.numpy().copy()
        out[name + '|weight_bits'] = np.packbits(w.numpy().astype(bool).reshape(-1))
        print(name, dict(zip(res, out[name + '|values'])))
    path = os.path.join(OUT, 'ohem_sampler.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= 170 * 1024


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_ohem(load_reference())
