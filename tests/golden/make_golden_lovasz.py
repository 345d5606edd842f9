#!/usr/bin/env python3
"""Golden vectors for LovaszLoss behind the decode head's bilinear resize, produced by EXECUTING the reference's losses/lovasz_loss.py and
BaseDecodeHead.losses on CPU in fp32 through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference
returns are stored).  lovasz_loss.py calls mmcv.is_list_of, which the loader's mmcv stand-in lacks: a two-line equivalent is installed here.

Cases (N = 2; labels constant on 4 x 4 blocks, a 255 region, one class absent from image 0; N(0, 1) logits -- wider logits push most
probabilities to 0 / 1, where the errors of foreground and background pixels meet within fp32 rounding and their order, hence the gradient,
is not determined: tests/lovasz_oracle.py):
  x4          19 x 17 -> 76 x 68, C =  6   reduction='none' (what the constructor requires with per_image=False), otherwise defaults
  x4_all      the same inputs              classes='all', class weights
  x4_img      the same inputs              per_image=True, reduction='mean'
  x4_img_sum  the same inputs              per_image=True, reduction='sum'
  x8           9 x 10 -> 72 x 80, C =  6   classes=[1, 4]; a 4 x 4 block of label 7: a valid pixel that is foreground for no class
  g11          7 x  9 -> 30 x 37, C = 11   the generic route
  head        the x4 inputs through DepthwiseSeparableASPPHead.losses with [CrossEntropyLoss(1.0), LovaszLoss(2.0, reduction='none')] and
              pixel weights handed in; head_half: the same with the weights halved -- loss_lovasz does not move
The seeds are chosen so that the share of low-resolution cells whose gradient fp32 cannot determine (lovasz_oracle's mask) stays below 5 %.

Usage:  python tests/golden/make_golden_lovasz.py        (writes tests/golden/lovasz_loss.npz)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402
from make_golden_focal import expand_weight, make_labels, make_weight_blocks  # noqa: E402

CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
# name: (C, low-resolution size, full size, seed)
SHAPES = {'x4': (6, (19, 17), (76, 68), 0), 'x8': (6, (9, 10), (72, 80), 2), 'g11': (11, (7, 9), (30, 37), 0)}
CASES = {
    'x4': ('x4', dict(reduction='none')),
    'x4_all': ('x4', dict(reduction='none', classes='all', class_weight=CW6)),
    'x4_img': ('x4', dict(per_image=True, reduction='mean')),
    'x4_img_sum': ('x4', dict(per_image=True, reduction='sum')),
    'x8': ('x8', dict(reduction='none', classes=[1, 4])),
    'g11': ('g11', dict(reduction='none')),
}
HEAD_LOSSES = [dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
               dict(type='LovaszLoss', loss_weight=2.0, reduction='none')]


def seeded_inputs():
    out = {}
    for name, (C, lo, hi, seed) in SHAPES.items():
        g = torch.Generator().manual_seed(9100 + seed)
        logits = torch.randn(2, C, *lo, generator=g)
        lab = make_labels(g, C, hi, absent=min(3, C - 1))
        if name == 'x8':
            lab[1, 40:44, 40:44] = 7
        out[name] = (logits, lab, make_weight_blocks(g, hi))
    return out


def run_term(ref, cfg, logits, lab, size):
    """the reference module on the reference's resize; the head hands every loss weight= and ignore_index= (decode_head.py:269-273)"""
    L = ref.builder.build_loss(dict(type='LovaszLoss', **cfg))
    z = logits.clone().requires_grad_()
    up = ref.resize(input=z, size=size, mode='bilinear', align_corners=False)
    loss = L(up, lab.long(), weight=None, ignore_index=255)
    return z, loss


def gen_lovasz(ref):
    def is_list_of(seq, expected_type):
        return isinstance(seq, list) and all(isinstance(v, expected_type) for v in seq)
    sys.modules['mmcv'].is_list_of = is_list_of
    _load('rsiseg.models.losses.lovasz_loss', 'rsiseg/models/losses/lovasz_loss.py')
    inputs = seeded_inputs()
    out = dict(cases=np.array(list(CASES)))
    for name, (logits, lab, wb) in inputs.items():
        out[name + '|logits'] = logits.numpy()
        out[name + '|label'] = lab.numpy()
        out[name + '|weight_blocks'] = wb.numpy()
    for name, (src, cfg) in CASES.items():
        logits, lab, _ = inputs[src]
        z, loss = run_term(ref, cfg, logits, lab, SHAPES[src][2])
        assert loss.dim() == 0, (name, loss.shape)
        loss.backward()
        out[name + '|loss'] = np.array(float(loss.detach()), dtype=np.float64)
        out[name + '|grad'] = z.grad.numpy().copy()
        print(name, float(loss.detach()), 'max |grad|', float(z.grad.abs().max()))
    head_cfg = dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36), c1_in_channels=8,
                    c1_channels=4, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True), align_corners=False,
                    loss_decode=HEAD_LOSSES)
    logits, lab, wb = inputs['x4']
    weight = expand_weight(wb, SHAPES['x4'][2])
    for tag, wgt in (('head', weight), ('head_half', weight * 0.5)):
        head = ref.builder.build_head(dict(head_cfg))
        z = logits.clone().requires_grad_()
        res = head.losses(z, lab.long().unsqueeze(1), wgt)
        assert list(res) == ['loss_ce', 'loss_lovasz', 'acc_seg'], list(res)
        (res['loss_ce'] + res['loss_lovasz']).backward()
        out[tag + '|names'] = np.array(list(res))
        out[tag + '|values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
        out[tag + '|grad'] = z.grad.numpy().copy()
        print(tag, dict(zip(res, out[tag + '|values'])))
    assert out['head|values'][1] == out['head_half|values'][1] and out['head|values'][0] != out['head_half|values'][0]
    path = os.path.join(OUT, 'lovasz_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_lovasz(load_reference())
