#!/usr/bin/env python3
"""Golden vectors for the sigmoid decode-head losses -- FocalLoss and CrossEntropyLoss(use_sigmoid=True) -- behind the decode head's bilinear
resize, produced by EXECUTING the reference's losses/focal_loss.py, losses/cross_entropy_loss.py and BaseDecodeHead.losses on CPU in fp32
through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns are stored).

focal_loss.py imports `mmcv.ops.sigmoid_focal_loss` for its CUDA branch; on the CPU the module runs its own py_sigmoid_focal_loss.  This
script installs an `mmcv.ops` stand-in whose function raises if it is ever called, so the executed arithmetic is the reference's alone.

Cases (N = 2; labels and pixel weights are constant on 4 x 4 blocks, the weights hold exact zeros), at make_golden_dice.py's shapes:
  x4_focal   19 x 17 ->  76 x  68, C =  6   FocalLoss defaults (gamma 2, alpha 0.5), pixel weights
  x4_bce     the same inputs                CrossEntropyLoss(use_sigmoid=True), pixel weights
  x8_focal   17 x 18 -> 136 x 144, C =  6   gamma 3, alpha a list, class weights, pixel weights
  g11_focal   7 x  9 ->  30 x  37, C = 11   gamma 0.5, alpha 0.25, reduction='none' (the mean of the returned map); image 1 is entirely 255
  g2_focal    7 x  9 ->  30 x  37, C =  2   gamma 0, alpha a list, reduction='sum', no pixel weights
  g2_bce     the same inputs                CrossEntropyLoss(use_sigmoid=True), no pixel weights
  head       the x4 inputs through DepthwiseSeparableASPPHead.losses with [CrossEntropyLoss(1.0), FocalLoss(2.0, alpha 0.25, class_weight)]
  head_w     the same two reference modules on the reference's resize WITH the pixel weights, added as the head adds them
Every case has a 255 region and a class that is absent from image 0.

Two things the reference cannot execute, so they are not here (tests compare them with the fp64 closed form only):
  * FocalLoss takes pixel weights as a FLAT [N H W] tensor only (focal_loss.py:56-61 asserts on [N, H, W]), softmax CE as [N, H, W] only,
    so BaseDecodeHead.losses cannot run a [CE, Focal] list with seg_weight: `head` runs without weights, `head_w` hands each module the
    layout it accepts.
  * CrossEntropyLoss(use_sigmoid=True, class_weight=...) hands a [C] pos_weight to binary_cross_entropy_with_logits on [N, C, H, W], which
    broadcasts against W and raises unless W == C.

Usage:  python tests/golden/make_golden_focal.py        (writes tests/golden/sigmoid_losses.npz)
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402

CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
ALPHA6 = [0.25, 0.5, 0.75, 0.1, 0.9, 0.4]
SHAPES = {'x4': (6, (19, 17), (76, 68)), 'x8': (6, (17, 18), (136, 144)), 'g11': (11, (7, 9), (30, 37)), 'g2': (2, (7, 9), (30, 37))}
CASES = {
    # name: (inputs, loss config, pixel weights?)
    'x4_focal': ('x4', dict(type='FocalLoss'), True),
    'x4_bce': ('x4', dict(type='CrossEntropyLoss', use_sigmoid=True), True),
    'x8_focal': ('x8', dict(type='FocalLoss', gamma=3.0, alpha=ALPHA6, class_weight=CW6), True),
    'g11_focal': ('g11', dict(type='FocalLoss', gamma=0.5, alpha=0.25, reduction='none'), True),
    'g2_focal': ('g2', dict(type='FocalLoss', gamma=0.0, alpha=[0.3, 0.6], reduction='sum'), False),
    'g2_bce': ('g2', dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=0.5), False),
}
HEAD_LOSSES = [dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
               dict(type='FocalLoss', loss_weight=2.0, gamma=2.0, alpha=0.25, class_weight=CW6)]


def make_labels(g, C, size, absent, all_ignored_image1=False):
    H, W = size
    blocks = torch.randint(0, C, (2, (H + 3) // 4, (W + 3) // 4), generator=g)
    lab = blocks.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    img0 = lab[0]
    img0[img0 == absent] = (absent + 1) % C              # one class absent from image 0
    lab[:, 4:12, 8:20] = 255
    if all_ignored_image1:
        lab[1] = 255
    return lab.to(torch.uint8)


def make_weight_blocks(g, size):
    """[2, ceil(H / 4), ceil(W / 4)] in [0, 1) with a quarter of the blocks exactly 0"""
    H, W = size
    blocks = torch.rand(2, (H + 3) // 4, (W + 3) // 4, generator=g)
    blocks[torch.rand(blocks.shape, generator=g) < 0.25] = 0.0
    return blocks


def expand_weight(blocks, size):
    H, W = size
    return blocks.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()


def seeded_inputs():
    g = torch.Generator().manual_seed(4177)
    out = {}
    for name, (C, lo, hi) in SHAPES.items():
        logits = torch.randn(2, C, *lo, generator=g) * 2
        lab = make_labels(g, C, hi, absent=min(3, C - 1), all_ignored_image1=name == 'g11')
        out[name] = (logits, lab, make_weight_blocks(g, hi))
    return out


def install_mmcv_ops():
    def refuse(*a, **k):
        raise RuntimeError('mmcv.ops.sigmoid_focal_loss is the CUDA branch; the CPU run must not reach it')
    m = types.ModuleType('mmcv.ops')
    m.sigmoid_focal_loss = refuse
    sys.modules['mmcv.ops'] = m
    sys.modules['mmcv'].ops = m


def run_term(ref, cfg, logits, lab, weight, size):
    """the reference module on the reference's resize; the head hands every loss weight= and ignore_index= (decode_head.py:269-273)"""
    L = ref.builder.build_loss(dict(cfg))
    z = logits.clone().requires_grad_()
    up = ref.resize(input=z, size=size, mode='bilinear', align_corners=False)
    if weight is not None and cfg['type'] == 'FocalLoss':
        weight = weight.reshape(-1)                      # the only layout focal_loss.py:56-61 accepts
    loss = L(up, lab.long(), weight=weight, ignore_index=255)
    loss = loss.mean() if loss.dim() else loss           # reduction='none': _parse_losses takes the mean of the map
    return z, loss


def gen_focal(ref):
    install_mmcv_ops()
    _load('rsiseg.models.losses.focal_loss', 'rsiseg/models/losses/focal_loss.py')
    inputs = seeded_inputs()
    out = dict(cases=np.array(list(CASES)))
    for name, (logits, lab, wb) in inputs.items():
        out[name + '|logits'] = logits.numpy()
        out[name + '|label'] = lab.numpy()
        out[name + '|weight_blocks'] = wb.numpy()
    for name, (src, cfg, weighted) in CASES.items():
        logits, lab, wb = inputs[src]
        size = SHAPES[src][2]
        z, loss = run_term(ref, cfg, logits, lab, expand_weight(wb, size) if weighted else None, size)
        loss.backward()
        out[name + '|loss'] = np.array(float(loss.detach()), dtype=np.float64)
        out[name + '|grad'] = z.grad.numpy().copy()
        print(name, float(loss.detach()), 'max |grad|', float(z.grad.abs().max()))
    # the head case, without weights (see the module docstring)
    head = ref.builder.build_head(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                                       c1_in_channels=8, c1_channels=4, dropout_ratio=0.0, num_classes=6,
                                       norm_cfg=dict(type='BN', requires_grad=True), align_corners=False, loss_decode=HEAD_LOSSES))
    logits, lab, wb = inputs['x4']
    z = logits.clone().requires_grad_()
    res = head.losses(z, lab.long().unsqueeze(1), None)
    assert list(res) == ['loss_ce', 'loss_focal', 'acc_seg'], list(res)
    (res['loss_ce'] + res['loss_focal']).backward()
    out['head|names'] = np.array(list(res))
    out['head|values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
    out['head|grad'] = z.grad.numpy().copy()
    print('head', dict(zip(res, out['head|values'])))
    # the same two modules with the pixel weights, each in the layout it accepts, added as the head adds them
    size = SHAPES['x4'][2]
    w = expand_weight(wb, size)
    z1, l1 = run_term(ref, HEAD_LOSSES[0], logits, lab, w, size)
    z2, l2 = run_term(ref, HEAD_LOSSES[1], logits, lab, w, size)
    l1.backward()
    l2.backward()
    out['head_w|values'] = np.array([float(l1.detach()), float(l2.detach())], dtype=np.float64)
    out['head_w|grad'] = (z1.grad + z2.grad).numpy().copy()
    print('head_w', out['head_w|values'])
    path = os.path.join(OUT, 'sigmoid_losses.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_focal(load_reference())
