#!/usr/bin/env python3
"""Golden vectors for UPerNet, produced by EXECUTING the reference's uper_head.py and resnet.py on the CPU in fp32 through make_golden.py's
loader (same rules: only seeded inputs and the numbers the reference returns are stored).

Head: UPerHead, in_channels [8, 16, 24, 32], channels 16, pool_scales (1, 2, 3, 6), six classes, N = 2, level grids 19 x 17 / 10 x 9 /
5 x 5 / 3 x 3 (what a 76 x 68 input gives a stride-32 backbone: no step is an exact x2), labels 76 x 68 with a 255 region, BatchNorm in
training mode, dropout 0.  Stored: the state_dict's key list and shapes, the logits, the fpn_bottleneck features, the losses, the gradient of
all four inputs and of every parameter.

Backbone: ResNetV1c(depth=50, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1), contract_dilation=True) with stem_channels = 16 and
base_channels = 4 (outputs of 16 / 32 / 64 / 128 channels: the narrowest the file size of the other head goldens leaves room for and the
kernels take) on a 2 x 3 x 76 x 68 input: the four outputs, and under the scalar sum_i <out_i, g_i> with the closed-form cotangents
g_i = cotangent(i, shape) below (not stored) the input gradient and the parameter gradients of layer3.0 and layer4.0, the two stride-2
bottlenecks no other model here runs.

The PARAMETERS are not stored: they are pfst_amd.synthetic.fill_state_dict(state_dict, SEED) over the stored key order, as for the other
goldens; the inputs are stored as fp16 (their values are fp16 numbers).

Usage:  python tests/golden/make_golden_upernet.py        (writes tests/golden/upernet.npz)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import OUT, _load, load_reference  # noqa: E402
from pfst_amd.synthetic import fill_state_dict  # noqa: E402

SEED = 91
N, NC, FULL = 2, 6, (76, 68)
IN_CHANNELS, CH = [8, 16, 24, 32], 16
GRIDS = [(19, 17), (10, 9), (5, 5), (3, 3)]
NORM = dict(type='BN', requires_grad=True)
HEAD = dict(type='UPerHead', in_channels=IN_CHANNELS, in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), channels=CH, dropout_ratio=0.0,
            num_classes=NC, norm_cfg=NORM, align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
BACKBONE = dict(type='ResNetV1c', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), dilations=(1, 1, 1, 1), strides=(1, 2, 2, 2), norm_cfg=NORM,
                norm_eval=False, style='pytorch', contract_dilation=True, in_channels=3, stem_channels=16, base_channels=4)
BACKBONE_GRAD_BLOCKS = ('layer3.0.', 'layer4.0.')
PERTURB = float(os.environ.get('UPERNET_GOLDEN_PERTURB', 2.0))          # see seeded_inputs; own_error: 0.02 of the bound at 2, 0.4 at 0.3, 7.7 at 0.02
OWN_ERROR_MAX = 0.1          # the reference's fp32 error may use up to this share of the per-link bound the GPU test holds the project to


def cotangent(i, shape):
    """the cotangent of backbone output i: cos(0.37 k + i) over the flat index k, as fp32"""
    k = np.arange(int(np.prod(shape)), dtype=np.float64)
    return torch.from_numpy(np.cos(0.37 * k + i).astype(np.float32).reshape(tuple(shape)))


def seeded_inputs():
    g = torch.Generator().manual_seed(2025)
    xs = [torch.relu(torch.randn(N, c, *hw, generator=g) + 0.5) for c, hw in zip(IN_CHANNELS, GRIDS)]     # backbone outputs: non-negative
    # The top level's second image is the first plus PERTURB standard deviations of noise.  With N = 2 the pool-scale-1 branch normalises
    # TWO values per channel, pre_1 and pre_2 = pre_1 + d: its outputs are +-1 / sqrt(1 + eps / var), var = d^2 / 4, whatever its
    # convolution's weights, and that convolution's weight gradient carries the factor 1 - 1 / (1 + eps / var) -- a difference of numbers
    # that agree to several digits when d is large, while for a small d the difference d itself is one.  How much of the value the
    # REFERENCE's own fp32 arithmetic then gets right depends on the draw, channel by channel: gen_upernet measures it against the same
    # head in fp64 (own_error) and refuses a golden whose own error is of the size of the bound the GPU test applies.  PERTURB is the
    # scale at which this draw passes that check with room to spare.
    xs[-1][1] = torch.relu(xs[-1][0] + PERTURB * torch.randn(xs[-1][0].shape, generator=g))
    xs = [x.half().float() for x in xs]
    label = torch.randint(0, NC, (N, 1, *FULL), generator=g)
    label[:, :, 7:19, 30:52] = 255
    img = torch.randn(N, 3, *FULL, generator=g).half().float()
    return xs, label, img


def shapes_of(sd):
    return np.array([','.join(str(d) for d in v.shape) for v in sd.values()])


def own_error(head, xs0, label, got32):
    """the reference head once more in fp64 on the same inputs: every fp32 tensor that is stored must lie within OWN_ERROR_MAX of the bound
    |a - b| <= 1e-4 max|b| + 1e-3 |b| around its fp64 value -- a golden whose own rounding error is of the size of the bound tests nothing"""
    import copy
    h64 = copy.deepcopy(head).double()
    h64.zero_grad()
    xs = [x.double().requires_grad_() for x in xs0]
    feats = h64._forward_feature(xs)
    logits = h64.cls_seg(feats)
    res = h64.losses(logits, label)
    sum(v for k, v in res.items() if k.startswith('loss')).backward()
    ref = dict(logits=logits, feats=feats, **{f'dx{i}': x.grad for i, x in enumerate(xs)}, **{'grad ' + k: p.grad for k, p in h64.named_parameters()})
    worst = {}
    for k, b in ref.items():
        a, b = got32[k].detach().double(), b.detach()
        worst[k] = float(((a - b).abs() / (1e-4 * b.abs().max() + 1e-3 * b.abs())).max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print('reference fp32 against fp64, share of the per-link bound:', [(k, round(v, 4)) for k, v in top])
    assert top[0][1] <= OWN_ERROR_MAX, top


def gen_upernet(ref):
    _load('rsiseg.models.decode_heads.psp_head', 'rsiseg/models/decode_heads/psp_head.py')
    _load('rsiseg.models.decode_heads.uper_head', 'rsiseg/models/decode_heads/uper_head.py')
    xs0, label, img0 = seeded_inputs()
    out = dict(seed=np.array(SEED), label=label.numpy().astype(np.uint8), img=img0.numpy().astype(np.float16))
    # ---- head
    head = ref.builder.build_head(dict(HEAD))
    head.train()
    sd = head.state_dict()
    fill_state_dict(sd, SEED)
    head.load_state_dict(sd)
    xs = [x.clone().requires_grad_() for x in xs0]
    feats = head._forward_feature(xs)
    logits = head.cls_seg(feats)
    res = head.losses(logits, label)
    sum(v for k, v in res.items() if k.startswith('loss')).backward()
    out['head|keys'] = np.array(list(sd))
    out['head|shapes'] = shapes_of(sd)
    out['head|logits'] = logits.detach().numpy()
    out['head|feats'] = feats.detach().numpy()
    out['head|loss_names'] = np.array(list(res))
    out['head|loss_values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
    for i, x in enumerate(xs):
        out[f'head|x{i}'] = xs0[i].numpy().astype(np.float16)
        out[f'head|dx{i}'] = x.grad.numpy().copy()
    for k, p in head.named_parameters():
        out['head|grad|' + k] = p.grad.numpy().copy()
    print('head', dict(zip(res, out['head|loss_values'])), 'max |dx|', [float(x.grad.abs().max()) for x in xs])
    own_error(head, xs0, label, dict(logits=logits, feats=feats, **{f'dx{i}': x.grad for i, x in enumerate(xs)},
                                     **{'grad ' + k: p.grad for k, p in head.named_parameters()}))
    # ---- backbone
    net = ref.builder.build_backbone(dict(BACKBONE))
    net.train()
    sd = net.state_dict()
    fill_state_dict(sd, SEED)
    net.load_state_dict(sd)
    img = img0.clone().requires_grad_()
    outs = net(img)
    assert [tuple(o.shape[2:]) for o in outs] == GRIDS and [o.shape[1] for o in outs] == [16, 32, 64, 128], [tuple(o.shape) for o in outs]
    sum((o * cotangent(i, o.shape)).sum() for i, o in enumerate(outs)).backward()
    out['backbone|keys'] = np.array(list(sd))
    out['backbone|shapes'] = shapes_of(sd)
    for i, o in enumerate(outs):
        out[f'backbone|out{i}'] = o.detach().numpy()
    out['backbone|dimg'] = img.grad.numpy().copy()
    for k, p in net.named_parameters():
        if k.startswith(BACKBONE_GRAD_BLOCKS):
            out['backbone|grad|' + k] = p.grad.numpy().copy()
    print('backbone', [tuple(o.shape) for o in outs], 'max |dimg|', float(img.grad.abs().max()))
    path = os.path.join(OUT, 'upernet.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= 680 * 1024           # the size of decode_heads.npz at most


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_upernet(load_reference())
