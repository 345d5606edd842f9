#!/usr/bin/env python3
"""Golden vectors for DiceLoss behind the decode head's bilinear resize, produced by EXECUTING the reference's losses/dice_loss.py and
BaseDecodeHead.losses on CPU in fp32 through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns
are stored).

Cases (N = 2; labels are constant on 4 x 4 blocks): the smallest shapes that reach every kernel form of csrc/dice_loss.hip --
  x4      19 x 17 ->  76 x  68, C =  6   inter-cell blocks, crosses a 16-block tile edge in both axes and ends ragged
  x8      17 x 18 -> 136 x 144, C =  6   the same for the auxiliary head's ratio; holds labels of 7 (the reference clamps them)
  x8c33   17 x 18 -> 136 x 144, C = 33   generic kernels, C > 8; ignore_index = 2 (a class index)
  g11      7 x  9 ->  30 x  37, C = 11   non-integer ratio, C > 8; image 1 is entirely 255
  g2       7 x  9 ->  30 x  37, C =  2   non-integer ratio, C <= 8
  head    the x4 inputs through DepthwiseSeparableASPPHead.losses with [CrossEntropyLoss(1.0), DiceLoss(3.0, class_weight)] and pixel weights
Every case has a 255 region and a class that is absent from image 0.  The x8c33 logits are formed from the x8 ones by exact fp32 operations
(make_c33) instead of being stored.

Usage:  python tests/golden/make_golden_dice.py        (writes tests/golden/dice_loss.npz)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402

CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
CASES = {
    # name: (C, (h, w), (H, W), DiceLoss options)
    'x4': (6, (19, 17), (76, 68), dict()),
    'x8': (6, (17, 18), (136, 144), dict(exponent=3, smooth=0.5, class_weight=CW6)),
    'x8c33': (33, (17, 18), (136, 144), dict(ignore_index=2, class_weight=[0.5 + 0.05 * i for i in range(33)])),
    'g11': (11, (7, 9), (30, 37), dict(exponent=3)),
    'g2': (2, (7, 9), (30, 37), dict(smooth=0.5, class_weight=[0.6, 1.4])),
}
HEAD_LOSSES = [dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), dict(type='DiceLoss', loss_weight=3.0, class_weight=CW6)]


def make_c33(base):
    """[2, 6, h, w] -> [2, 33, h, w]: class c is class c % 6 of the base scaled by 1 + (c // 6) / 8 and shifted by (c // 6) / 4 -- one fp32
    multiply and one fp32 add per element, the same bits on every machine"""
    return torch.stack([base[:, c % 6] * (1.0 + (c // 6) / 8.0) + (c // 6) / 4.0 for c in range(33)], 1).contiguous()


def make_labels(g, C, size, absent, all_ignored_image1=False, bad=False):
    H, W = size
    blocks = torch.randint(0, C, (2, (H + 3) // 4, (W + 3) // 4), generator=g)
    lab = blocks.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    img0 = lab[0]
    img0[img0 == absent] = (absent + 1) % C              # one class absent from image 0: T = I = 0 there
    lab[:, 4:12, 8:20] = 255
    if bad:
        lab[1, 16:20, 4:8] = 7                            # outside [0, 6), not an ignore index: the reference clamps it to class 5
    if all_ignored_image1:
        lab[1] = 255
    return lab.to(torch.uint8)


def expand_weight(blocks):
    return blocks.repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()


def seeded_inputs():
    g = torch.Generator().manual_seed(77)
    out = {}
    for name, (C, lo, hi, _) in CASES.items():
        if name == 'x8c33':
            logits = make_c33(out['x8'][0])
        else:
            logits = torch.randn(2, C, *lo, generator=g) * 2
        lab = make_labels(g, C, hi, absent=min(3, C - 1), all_ignored_image1=name == 'g11', bad=name == 'x8')
        out[name] = (logits, lab)
    out['head_weight'] = expand_weight(torch.rand(2, 19, 17, generator=g))       # stored at 19 x 17: constant on 4 x 4 blocks
    return out


def gen_dice(ref):
    _load('rsiseg.models.losses.dice_loss', 'rsiseg/models/losses/dice_loss.py')
    inputs = seeded_inputs()
    out = dict(cases=np.array(list(CASES)), head_weight_blocks=inputs['head_weight'][:, ::4, ::4].numpy().copy())
    for name, (C, lo, hi, opts) in CASES.items():
        logits, lab = inputs[name]
        L = ref.builder.build_loss(dict(type='DiceLoss', loss_weight=1.0, **opts))
        z = logits.clone().requires_grad_()
        up = ref.resize(input=z, size=hi, mode='bilinear', align_corners=False)
        # the head hands every loss weight= and ignore_index= (decode_head.py:269-273); DiceLoss.forward swallows both
        loss = L(up, lab.long(), weight=torch.rand(2, *hi, generator=torch.Generator().manual_seed(1)), ignore_index=255)
        loss.backward()
        if name != 'x8c33':
            out[name + '|logits'] = logits.numpy()
        out[name + '|label'] = lab.numpy()
        out[name + '|loss'] = np.array(float(loss.detach()), dtype=np.float64)
        out[name + '|grad'] = z.grad.numpy().copy()
        print(name, float(loss.detach()), 'max |grad|', float(z.grad.abs().max()))
    # the head case
    head = ref.builder.build_head(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                                       c1_in_channels=8, c1_channels=4, dropout_ratio=0.0, num_classes=6,
                                       norm_cfg=dict(type='BN', requires_grad=True), align_corners=False, loss_decode=HEAD_LOSSES))
    logits, lab = inputs['x4']
    z = logits.clone().requires_grad_()
    res = head.losses(z, lab.long().unsqueeze(1), inputs['head_weight'])
    assert list(res) == ['loss_ce', 'loss_dice', 'acc_seg'], list(res)
    (res['loss_ce'] + res['loss_dice']).backward()
    out['head|names'] = np.array(list(res))
    out['head|values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
    out['head|grad'] = z.grad.numpy().copy()
    print('head', dict(zip(res, out['head|values'])))
    path = os.path.join(OUT, 'dice_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_dice(load_reference())
