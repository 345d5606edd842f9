#!/usr/bin/env python3
"""Golden vectors for the HRNet backbone under a multi-level FCNHead, produced by EXECUTING the reference's backbones/hrnet.py and
decode_heads/fcn_head.py on the CPU in fp32 through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns
are stored).  What hrnet.py imports beyond that loader is added here: `rsiseg.ops.Upsample` from rsiseg/ops/wrappers.py and a stand-in for
`mmcv.runner.ModuleList` (nn.ModuleList under the loader's BaseModule).

Model: HRNet(extra: stage1 BOTTLENECK (1,) (8,); stage2 BASIC 1 module (1, 1) (6, 12); stage3 1 module (1, 1, 1) (6, 12, 24); stage4 2 modules
(1, 1, 1, 1) (6, 12, 24, 48)) -- widths that are no multiples of 4 or 16, and a four-output exchange that feeds another module -- under
FCNHead([6, 12, 24, 48], input_transform='resize_concat', channels=90, kernel_size=1, num_convs=1, concat_input=False, dropout_ratio=-1), six
classes, N = 2, BatchNorm in training mode, labels with a 255 region.  Two geometries:
  A  3 x 64 x 64   grids 16 x 16 / 8 x 8 / 4 x 4 / 2 x 2: every exchange is an exact power of two;
  B  3 x 72 x 56   grids 18 x 14 / 9 x 7 / 5 x 4 / 3 x 2: the reference interpolates twice.
Stored per geometry: the image (fp16: its values are fp16 numbers), the labels, the four backbone outputs, the logits, the head's features, the
loss, the input gradient and every parameter gradient; once: the key lists and shapes of the reference's state_dicts (backbone, head).

A tensor with many elements is stored as an evenly strided sample of its flat view (tests/hrnet_oracle.py `sample`: parameter gradients beyond
448 elements, the features and the input gradient beyond 4096: as much as the size limit leaves room for).  Stored whole, the parameter gradients alone (about 240 k floats per geometry,
the 64-channel stem's 3x3 and the 48-channel branch's eight 3x3 kernels most of it) are three times the size this file may have (that of
upernet.npz); every tensor is still represented, and the per-element bound is the same.

The PARAMETERS are not stored: they are pfst_amd.synthetic.fill_state_dict(state_dict, SEED) over the stored key order, backbone and head each.

The coarsest branch's BatchNorms see 8 (A) or 12 (B) values per channel, so how much of a value the reference's own fp32 arithmetic gets
right depends on the draw: as in make_golden_semantic_fpn.py every stored tensor is compared with the same modules run in fp64 and the file is
refused if that error exceeds OWN_ERROR_MAX of the per-link bound the GPU test holds the project to.  A draw is also refused when a ReLU
of the network sits on its kink: with 2 x 10^5 gated values per pass, a pre-activation within a few 10^-6 of zero (relative) is common, any
fp32-faithful arithmetic may flip it, and one flipped gate moves a whole channel's BatchNorm-backward sums -- and every gradient behind
them -- by tens of bounds (seen with draw 2031 on B: channel 63 of the head under the split arithmetics).  The rule: the image moved by
KINK_EPS = 2^-19 relative (one fp32 rounding per conv -> BN link over the about 32 links of the longest path), either way, must leave every
stored tensor inside the bound.  The generator searches the draw seed upwards from DRAW = 2031 until both geometries pass; the draw that
passes is 2036 (N(0, 1) images, drawn in the order A, B), parameter seed 97.

Usage:  python tests/golden/make_golden_hrnet.py        (writes tests/golden/hrnet.npz)
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import OUT, _load, load_reference  # noqa: E402
from hrnet_oracle import KEEP_GRAD, KEEP_MAP, sample  # noqa: E402
from pfst_amd.synthetic import fill_state_dict  # noqa: E402

SEED, DRAW = 97, int(os.environ.get('HRNET_GOLDEN_DRAW', 2031))
N, NC = 2, 6
WIDTHS = (6, 12, 24, 48)
GEOMETRIES = dict(A=(64, 64), B=(72, 56))
GRIDS = dict(A=[(16, 16), (8, 8), (4, 4), (2, 2)], B=[(18, 14), (9, 7), (5, 4), (3, 2)])
NORM = dict(type='BN', requires_grad=True)
EXTRA = dict(stage1=dict(num_modules=1, num_branches=1, block='BOTTLENECK', num_blocks=(1,), num_channels=(8,)),
             stage2=dict(num_modules=1, num_branches=2, block='BASIC', num_blocks=(1, 1), num_channels=WIDTHS[:2]),
             stage3=dict(num_modules=1, num_branches=3, block='BASIC', num_blocks=(1, 1, 1), num_channels=WIDTHS[:3]),
             stage4=dict(num_modules=2, num_branches=4, block='BASIC', num_blocks=(1, 1, 1, 1), num_channels=WIDTHS))
BACKBONE = dict(type='HRNet', extra=EXTRA, norm_cfg=NORM)
HEAD = dict(type='FCNHead', in_channels=list(WIDTHS), in_index=[0, 1, 2, 3], input_transform='resize_concat', channels=sum(WIDTHS), kernel_size=1,
            num_convs=1, concat_input=False, dropout_ratio=-1, num_classes=NC, norm_cfg=NORM, align_corners=False,
            loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
OWN_ERROR_MAX = 0.1          # the reference's fp32 error may use up to this share of the per-link bound the GPU test holds the project to
MAX_BYTES = 593947           # the size of upernet.npz
MAX_DRAWS = 400
# one fp32 rounding (2^-24) per conv -> BN link over the about 32 links of the network's longest path: the deviation any fp32-faithful
# arithmetic (the bf16x6 / f16x3 splits included) may have built up in front of a ReLU
KINK_EPS = 2.0 ** -19


def seeded_inputs(draw):
    """-> {geometry: (img, label)}; one generator, geometries in the order A, B"""
    g = torch.Generator().manual_seed(draw)
    out = {}
    for name in ('A', 'B'):
        h, w = GEOMETRIES[name]
        img = torch.randn(N, 3, h, w, generator=g).half().float()
        label = torch.randint(0, NC, (N, 1, h, w), generator=g)
        label[:, :, 7:19, w // 2 - 10:w // 2 + 8] = 255
        out[name] = (img, label)
    return out


def shapes_of(sd):
    return np.array([','.join(str(d) for d in v.shape) for v in sd.values()])


def run(net, head, img0, label, dtype):
    """backbone -> head -> loss -> backward; -> dict of every tensor the golden stores (in `dtype`, sampled as stored)"""
    net.zero_grad(), head.zero_grad()
    img = img0.to(dtype).clone().requires_grad_()
    outs = net(img)
    seen = {}
    hook = head.conv_seg.register_forward_pre_hook(lambda m, a: seen.__setitem__('feats', a[0]))
    logits = head(list(outs))
    hook.remove()
    res = head.losses(logits, label)
    sum(v for k, v in res.items() if k.startswith('loss')).backward()
    t = dict(logits=logits, feats=sample(seen['feats'], KEEP_MAP), dimg=sample(img.grad, KEEP_MAP))
    t.update({f'out{i}': o for i, o in enumerate(outs)})
    t.update({'grad|backbone.' + k: sample(p.grad, KEEP_GRAD) for k, p in net.named_parameters()})
    t.update({'grad|head.' + k: sample(p.grad, KEEP_GRAD) for k, p in head.named_parameters()})
    return {k: v.detach().clone() for k, v in t.items()}, res


def own_error(name, got32, ref64):
    """-> the worst share of the bound |a - b| <= 1e-4 max|b| + 1e-3 |b| that the reference's own fp32 rounding uses up, over every stored tensor"""
    worst = {}
    for k, b in ref64.items():
        a = got32[k].double()
        worst[k] = float(((a - b).abs() / (1e-4 * b.abs().max() + 1e-3 * b.abs())).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f'geometry {name}: reference fp32 against fp64, share of the per-link bound:', [(k, round(v, 4)) for k, v in top])
    return top[0][1]


def gen_hrnet(ref):
    R = sys.modules
    R['rsiseg.ops'].Upsample = R['rsiseg.ops.wrappers'].Upsample
    base_module = R['mmcv.runner'].BaseModule

    class ModuleList(base_module, torch.nn.ModuleList):          # mmcv.runner.ModuleList, the one name the loader's shim lacks
        def __init__(self, modules=None, init_cfg=None):
            base_module.__init__(self, init_cfg)
            torch.nn.ModuleList.__init__(self, modules)
    R['mmcv.runner'].ModuleList = ModuleList
    _load('rsiseg.models.backbones.hrnet', 'rsiseg/models/backbones/hrnet.py')
    net = ref.builder.BACKBONES.build(copy.deepcopy(BACKBONE))
    head = ref.builder.build_head(copy.deepcopy(HEAD))
    net.train(), head.train()
    base = dict(seed=np.array(SEED))
    for tag, m in (('backbone', net), ('head', head)):
        sd = m.state_dict()
        fill_state_dict(sd, SEED)
        m.load_state_dict(sd)
        base[tag + '|keys'] = np.array(list(sd))
        base[tag + '|shapes'] = shapes_of(sd)
    start = {tag: copy.deepcopy(m.state_dict()) for tag, m in (('backbone', net), ('head', head))}
    net64, head64 = copy.deepcopy(net).double(), copy.deepcopy(head).double()
    start64 = dict(backbone=copy.deepcopy(net64.state_dict()), head=copy.deepcopy(head64.state_dict()))

    for draw in range(DRAW, DRAW + MAX_DRAWS):
        out, ok = dict(base, draw=np.array(draw)), True
        for name, (img, label) in seeded_inputs(draw).items():
            # every geometry starts from the filled state (BatchNorm's running statistics move in a training-mode forward)
            net.load_state_dict(start['backbone']), head.load_state_dict(start['head'])
            net64.load_state_dict(start64['backbone']), head64.load_state_dict(start64['head'])
            got, res = run(net, head, img, label, torch.float32)
            ref64, _ = run(net64, head64, img, label, torch.float64)
            if own_error(name, got, ref64) > OWN_ERROR_MAX:
                ok = False
                break
            # no ReLU of the network may sit on its kink within an fp32-faithful arithmetic's error: the image moved by KINK_EPS (relative,
            # either way) must leave every stored tensor inside the bound the GPU test enforces -- one flipped gate moves a gradient by
            # tens of bounds, and a golden that a rounding can move that far tests the draw, not the code
            u = torch.rand(img.shape, generator=torch.Generator().manual_seed(draw)) * 2 - 1
            moved = 0.0
            for sign in (1.0, -1.0):
                net.load_state_dict(start['backbone']), head.load_state_dict(start['head'])
                near, _ = run(net, head, img * (1 + sign * KINK_EPS * u), label, torch.float32)
                moved = max(moved, own_error(f'{name} moved {sign:+.0f}', near, {k: v.double() for k, v in got.items()}))
            if moved > 1.0:
                ok = False
                break
            assert [tuple(got[f'out{i}'].shape[2:]) for i in range(4)] == GRIDS[name]
            assert tuple(got['logits'].shape) == (N, NC) + GRIDS[name][0]
            p = name + '|'
            out[p + 'img'] = img.numpy().astype(np.float16)
            out[p + 'label'] = label.numpy().astype(np.uint8)
            out[p + 'loss_names'] = np.array(list(res))
            out[p + 'loss_values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
            for k, v in got.items():
                out[p + k] = v.numpy().copy()
            print(name, dict(zip(res, out[p + 'loss_values'])), 'max |dimg|', float(got['dimg'].abs().max()))
        if ok:
            break
        print(f'draw {draw} refused')
    assert ok, f'no draw in [{DRAW}, {DRAW + MAX_DRAWS}) keeps the reference within {OWN_ERROR_MAX} of the bound'
    print('draw', draw)
    path = os.path.join(OUT, 'hrnet.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, 'bytes')
    assert size <= MAX_BYTES, size


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_hrnet(load_reference())
