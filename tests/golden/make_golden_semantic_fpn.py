#!/usr/bin/env python3
"""Golden vectors for Semantic FPN, produced by EXECUTING the reference's necks/fpn.py and decode_heads/fpn_head.py on the CPU in fp32
through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns are stored).  What the two files import
beyond that loader is added here: an empty `rsiseg.models.necks` package and `rsiseg.ops.Upsample` from rsiseg/ops/wrappers.py.

Model: FPN(in_channels [8, 16, 24, 32] -> 16, num_outs 4: bare biased convolutions, nearest top-down path) under FPNHead(in_channels [16] * 4,
feature_strides [4, 8, 16, 32], channels 8), six classes, N = 2, BatchNorm in training mode, dropout 0, labels with a 255 region.  Three
geometries of the four backbone-level inputs:
  A  16 x 16 / 8 x 8 / 4 x 4 / 2 x 2    (labels 64 x 64): every level's last convolution on exactly half of level 0's grid, every merge exact x2;
  C  20 x 12 / 10 x 6 / 5 x 3 / 3 x 2   (labels 80 x 48): levels 1 and 2 on the half grid, level 3 ends at 24 x 16 and is resized down;
                                         the 3 x 2 -> 5 x 3 merge is no integer ratio;
  B  19 x 17 / 10 x 9 / 5 x 5 / 3 x 3   (labels 76 x 68): no level on the half grid, no merge an integer ratio.
Stored per geometry: the inputs (fp16: their values are fp16 numbers), the labels, the four neck outputs, the logits, the level sum the head
hands cls_seg ('feats'), the losses, the gradients of the four inputs and of every neck and head parameter; once: the key lists and shapes of
neck and head.

The PARAMETERS are not stored: they are pfst_amd.synthetic.fill_state_dict(state_dict, SEED) over the stored key order, neck and head each.

The top level's first BatchNorm sees 8 (A), 12 (C) or 18 (B) values per channel, so how much of a value the reference's own fp32 arithmetic
gets right depends on the draw: as in make_golden_upernet.py every stored tensor is compared with the same modules run in fp64 and the file
is refused if that error exceeds OWN_ERROR_MAX of the per-link bound the GPU test holds the project to.  The draw that passes: generator
seed DRAW = 2026 for the inputs (relu(N(0.5, 1)) per level, drawn in the order A, C, B), parameter seed 93.

Usage:  python tests/golden/make_golden_semantic_fpn.py        (writes tests/golden/semantic_fpn.npz)
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import OUT, _load, load_reference  # noqa: E402
from pfst_amd.synthetic import fill_state_dict  # noqa: E402

SEED, DRAW = 93, int(os.environ.get('SEMANTIC_FPN_GOLDEN_DRAW', 2026))
N, NC = 2, 6
IN_CHANNELS, NECK_CH, CH = [8, 16, 24, 32], 16, 8
GEOMETRIES = dict(A=[(16, 16), (8, 8), (4, 4), (2, 2)], C=[(20, 12), (10, 6), (5, 3), (3, 2)], B=[(19, 17), (10, 9), (5, 5), (3, 3)])
NORM = dict(type='BN', requires_grad=True)
NECK = dict(type='FPN', in_channels=IN_CHANNELS, out_channels=NECK_CH, num_outs=4)
HEAD = dict(type='FPNHead', in_channels=[NECK_CH] * 4, in_index=[0, 1, 2, 3], feature_strides=[4, 8, 16, 32], channels=CH, dropout_ratio=0.0,
            num_classes=NC, norm_cfg=NORM, align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
OWN_ERROR_MAX = 0.1          # the reference's fp32 error may use up to this share of the per-link bound the GPU test holds the project to
MAX_BYTES = 680 * 1024       # the size of upernet.npz at most


def seeded_inputs():
    """-> {geometry: (xs, label)}; one generator, geometries in the order A, C, B"""
    g = torch.Generator().manual_seed(DRAW)
    out = {}
    for name in ('A', 'C', 'B'):
        grids = GEOMETRIES[name]
        xs = [torch.relu(torch.randn(N, c, *hw, generator=g) + 0.5).half().float() for c, hw in zip(IN_CHANNELS, grids)]
        full = (4 * grids[0][0], 4 * grids[0][1])
        label = torch.randint(0, NC, (N, 1, *full), generator=g)
        label[:, :, 7:19, full[1] // 2 - 10:full[1] // 2 + 8] = 255
        out[name] = (xs, label)
    return out


def shapes_of(sd):
    return np.array([','.join(str(d) for d in v.shape) for v in sd.values()])


def run(neck, head, xs0, label, dtype):
    """neck -> head -> losses -> backward; -> dict of every tensor the golden stores (in `dtype`)"""
    neck.zero_grad(), head.zero_grad()
    xs = [x.to(dtype).clone().requires_grad_() for x in xs0]
    outs = neck(xs)
    seen = {}
    hook = head.conv_seg.register_forward_pre_hook(lambda m, a: seen.__setitem__('feats', a[0]))
    logits = head(list(outs))
    hook.remove()
    res = head.losses(logits, label)
    sum(v for k, v in res.items() if k.startswith('loss')).backward()
    t = dict(logits=logits, feats=seen['feats'])
    t.update({f'out{i}': o for i, o in enumerate(outs)})
    t.update({f'dx{i}': x.grad for i, x in enumerate(xs)})
    t.update({'grad|neck.' + k: p.grad for k, p in neck.named_parameters()})
    t.update({'grad|head.' + k: p.grad for k, p in head.named_parameters()})
    return {k: v.detach().clone() for k, v in t.items()}, res


def own_error(name, got32, ref64):
    """every fp32 tensor that is stored must lie within OWN_ERROR_MAX of the bound |a - b| <= 1e-4 max|b| + 1e-3 |b| around its fp64 value -- a
    golden whose own rounding error is of the size of the bound tests nothing"""
    worst = {}
    for k, b in ref64.items():
        a = got32[k].double()
        worst[k] = float(((a - b).abs() / (1e-4 * b.abs().max() + 1e-3 * b.abs())).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print(f'geometry {name}: reference fp32 against fp64, share of the per-link bound:', [(k, round(v, 4)) for k, v in top])
    assert top[0][1] <= OWN_ERROR_MAX, (name, top)


def gen_semantic_fpn(ref):
    R = sys.modules
    pkg = types.ModuleType('rsiseg.models.necks')
    pkg.__path__ = []
    R['rsiseg.models.necks'] = pkg
    R['rsiseg.ops'].Upsample = R['rsiseg.ops.wrappers'].Upsample
    _load('rsiseg.models.necks.fpn', 'rsiseg/models/necks/fpn.py')
    _load('rsiseg.models.decode_heads.fpn_head', 'rsiseg/models/decode_heads/fpn_head.py')
    neck = ref.builder.NECKS.build(dict(NECK))
    head = ref.builder.build_head(dict(HEAD))
    neck.train(), head.train()
    out = dict(seed=np.array(SEED), draw=np.array(DRAW))
    for tag, m in (('neck', neck), ('head', head)):
        sd = m.state_dict()
        fill_state_dict(sd, SEED)
        m.load_state_dict(sd)
        out[tag + '|keys'] = np.array(list(sd))
        out[tag + '|shapes'] = shapes_of(sd)
    start = {tag: copy.deepcopy(m.state_dict()) for tag, m in (('neck', neck), ('head', head))}
    neck64, head64 = copy.deepcopy(neck).double(), copy.deepcopy(head).double()
    start64 = dict(neck=copy.deepcopy(neck64.state_dict()), head=copy.deepcopy(head64.state_dict()))

    def build(full):
        for name, (xs0, label) in seeded_inputs().items():
            # every geometry starts from the filled state (BatchNorm's running statistics move in a training-mode forward)
            neck.load_state_dict(start['neck']), head.load_state_dict(start['head'])
            neck64.load_state_dict(start64['neck']), head64.load_state_dict(start64['head'])
            got, res = run(neck, head, xs0, label, torch.float32)
            ref64, _ = run(neck64, head64, xs0, label, torch.float64)
            own_error(name, got, ref64)
            assert [tuple(got[f'out{i}'].shape[2:]) for i in range(4)] == GEOMETRIES[name]
            assert tuple(got['logits'].shape) == (N, NC) + GEOMETRIES[name][0] and tuple(got['feats'].shape) == (N, CH) + GEOMETRIES[name][0]
            p = name + '|'
            out[p + 'label'] = label.numpy().astype(np.uint8)
            out[p + 'loss_names'] = np.array(list(res))
            out[p + 'loss_values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
            for i, x in enumerate(xs0):
                out[p + f'x{i}'] = x.numpy().astype(np.float16)
            for k, v in got.items():
                if k.startswith('grad|') and name == 'B' and not full:
                    continue                     # (the file-size fallback: B keeps the forward results and the input gradients)
                out[p + k] = v.numpy().copy()
            print(name, dict(zip(res, out[p + 'loss_values'])), 'max |dx|', [float(got[f'dx{i}'].abs().max()) for i in range(4)])
    path = os.path.join(OUT, 'semantic_fpn.npz')
    for full in (True, False):
        for k in [k for k in out if k[:2] in ('A|', 'B|', 'C|')]:
            del out[k]
        build(full)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(path, size, 'bytes', '(every gradient)' if full else '(B without parameter gradients)')
        if size <= MAX_BYTES:
            break
    assert os.path.getsize(path) <= MAX_BYTES


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_semantic_fpn(load_reference())
