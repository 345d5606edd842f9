#!/usr/bin/env python3
"""Golden vectors for the comparison decode heads, produced by EXECUTING the reference's psp_head.py, aspp_head.py and fcn_head.py on the
CPU in fp32 through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns are stored).

Every head: in_channels = 32, channels = 16, six classes, N = 2, a 19 x 17 feature grid, labels 76 x 68 with a 255 region, BatchNorm in
training mode, dropout 0.  PSPHead pool_scales (1, 2, 3, 6); ASPPHead dilations (1, 2, 3, 5); FCNHead num_convs = 2, concat_input.
Stored per head: the state_dict's key list and shapes, the logits, the bottleneck / conv_cat features, the losses, the gradient of the
input and of every parameter.  The PARAMETERS are not stored: they are pfst_amd.synthetic.fill_state_dict(state_dict, SEED) over the
stored key order, as for the other goldens (the input is stored, as fp16 -- its values are fp16 numbers), which keeps the file within the
size of the existing loss goldens.

Usage:  python tests/golden/make_golden_heads.py        (writes tests/golden/decode_heads.npz)
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

SEED = 77
N, CIN, CH, NC, GRID, FULL = 2, 32, 16, 6, (19, 17), (76, 68)
COMMON = dict(in_channels=CIN, in_index=0, channels=CH, dropout_ratio=0.0, num_classes=NC, norm_cfg=dict(type='BN', requires_grad=True),
              align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
HEADS = {
    'psp': dict(type='PSPHead', pool_scales=(1, 2, 3, 6)),
    'aspp': dict(type='ASPPHead', dilations=(1, 2, 3, 5)),
    'fcn': dict(type='FCNHead', num_convs=2, kernel_size=3, concat_input=True),
}


def seeded_inputs():
    g = torch.Generator().manual_seed(2024)
    x = torch.relu(torch.randn(N, CIN, *GRID, generator=g) + 0.5).half().float()          # a backbone output: non-negative
    label = torch.randint(0, NC, (N, 1, *FULL), generator=g)
    label[:, :, 7:19, 30:52] = 255
    return x, label


def gen_heads(ref):
    _load('rsiseg.models.decode_heads.psp_head', 'rsiseg/models/decode_heads/psp_head.py')
    x0, label = seeded_inputs()
    out = dict(heads=np.array(list(HEADS)), seed=np.array(SEED), x=x0.numpy().astype(np.float16), label=label.numpy().astype(np.uint8))
    for name, extra in HEADS.items():
        head = ref.builder.build_head(dict(extra, **COMMON))
        head.train()
        sd = head.state_dict()
        fill_state_dict(sd, SEED)
        head.load_state_dict(sd)
        x = x0.clone().requires_grad_()
        feats = head._forward_feature([x])
        logits = head.cls_seg(feats)
        res = head.losses(logits, label)
        sum(v for k, v in res.items() if k.startswith('loss')).backward()
        out[name + '|keys'] = np.array(list(sd))
        out[name + '|shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
        out[name + '|logits'] = logits.detach().numpy()
        out[name + '|feats'] = feats.detach().numpy()
        out[name + '|loss_names'] = np.array(list(res))
        out[name + '|loss_values'] = np.array([float(v.detach().reshape(-1)[0]) for v in res.values()], dtype=np.float64)
        out[name + '|dx'] = x.grad.numpy().copy()
        for k, p in head.named_parameters():
            out[name + '|grad|' + k] = p.grad.numpy().copy()
        print(name, dict(zip(res, out[name + '|loss_values'])), 'max |dx|', float(x.grad.abs().max()))
    path = os.path.join(OUT, 'decode_heads.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) <= 680 * 1024


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_heads(load_reference())
