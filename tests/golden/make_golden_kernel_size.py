#!/usr/bin/env python3
"""Golden vectors for PFGSTLoss at kernel_size 5 and 7 and for top_k beyond 4 (overlapping top / bottom sets), produced by
EXECUTING the reference's PFGSTLoss on CPU through make_golden.py's loader (same rules: only seeded inputs and the numbers the
reference returns are stored).  Inputs are gen_pfgst_options' seeded set.

Usage:  python tests/golden/make_golden_kernel_size.py        (writes tests/golden/pfgst_kernel_size.npz)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, load_reference, uda_cfg  # noqa: E402

# name -> overrides of the PFGSTLoss config.  At S = 128 with downscale 0.5 the loss grid is 16 x 16: dilation 1 for K = 5 / 7
# (K = 7 leaves 56 valid target pixels), dilation 2 only at full resolution (32 x 32)
KERNEL_SIZE_VARIANTS = {
    'k5_d1_top3': dict(kernel_size=5, dilation=1, top_k=3),
    'k5_d1_top16_gaussian': dict(kernel_size=5, dilation=1, top_k=16, sim_type='gaussian', sigma=8.0),
    'k7_d1_all_unfold_margin2': dict(kernel_size=7, dilation=1, top_k=None, detach_unfold=False, src_loss_type='margin2',
                                     margin=[0.6, 0.0]),
    'k5_d2_full_res': dict(kernel_size=5, dilation=2, top_k=3, downscale=None),
    'k3_top6': dict(kernel_size=3, top_k=6),
    'k5_d1_src_perc_proj': dict(kernel_size=5, dilation=1, top_k=8, src_perc=0.6, proj_net_cfg=dict(in_channels=32, out_channels=16)),
}


def seeded_inputs():
    """gen_pfgst_options' inputs (same generator seed and draw order)"""
    g = torch.Generator().manual_seed(21)
    B, C, S = 2, 6, 128
    lt0 = torch.randn(B, C, S // 4, S // 4, generator=g) * 2
    xe = torch.randn(B, 32, S // 8, S // 8, generator=g)
    xs0 = torch.randn(B, 32, S // 8, S // 8, generator=g)
    gts = torch.randint(0, C, (B, 1, 4, 4), generator=g).repeat_interleave(S // 4, 2).repeat_interleave(S // 4, 3)
    gts[:, :, :8, :8] = 255
    mm = (torch.rand(B, 1, 2, 2, generator=g) > 0.6).long().repeat_interleave(S // 2, 2).repeat_interleave(S // 2, 3)
    return lt0, xe, xs0, gts, mm


def gen_pfgst_kernel_size(ref):
    lt0, xe, xs0, gts, mm = seeded_inputs()
    out = dict(logits_trg=lt0.numpy(), x_ema=xe.numpy(), x_src=xs0.numpy(), gt_src=gts.numpy(), mix_masks=mm.numpy(),
               variants=np.array(list(KERNEL_SIZE_VARIANTS)))
    for i, (name, over) in enumerate(KERNEL_SIZE_VARIANTS.items()):
        cfg = dict(uda_cfg()['aux_losses'][0])
        cfg.update(over)
        torch.manual_seed(200 + i)                         # nn.Conv2d's default initialisation of proj_net
        PL = ref.builder.build_loss(cfg)
        lt, xs = lt0.clone().requires_grad_(), xs0.clone().requires_grad_()
        res = PL(dict(logits_trg=lt, logits_ema=None, gt_src=gts, x_ema=xe, x_src=xs, img_trg=None, mix_masks=mm))
        names = [k for k in res if not k.startswith('vis|')]
        tot = sum(res[n].sum() for n in names)
        tot.backward()
        vals = {n: float(res[n].detach().sum()) for n in names}
        # the target side must be live: more than one valid pixel (all k^2 neighbours un-mixed, source label != 255 at the centre
        # -- the loss grid's labels are the nearest-down-sampled gt_src) and non-zero similarity losses
        unmixed = res['vis|density_sim_feat'][2]
        H, W = unmixed.shape[-2:]
        ctr_ok = torch.nn.functional.interpolate(gts.float(), size=(H, W), mode='nearest') != 255
        n_valid = int((unmixed & ctr_ok).sum())
        assert n_valid > 1 and vals['loss_sim_pos'] != 0.0 and vals['loss_sim_neg'] != 0.0, (name, n_valid, vals)
        out[name + '|names'] = np.array(names)
        out[name + '|losses'] = np.array([vals[n] for n in names], dtype=np.float64)
        out[name + '|grad_logits'] = lt.grad.numpy().copy()
        out[name + '|grad_xsrc'] = xs.grad.numpy().copy()
        out[name + '|density'] = res['vis|density_sim_feat'][1].numpy().copy()
        out[name + '|n_valid'] = np.array(n_valid)
        if PL.proj_net is not None:
            out[name + '|proj_weight'] = PL.proj_net.weight.detach().numpy().copy()
            out[name + '|proj_bias'] = PL.proj_net.bias.detach().numpy().copy()
            out[name + '|grad_proj_weight'] = PL.proj_net.weight.grad.numpy().copy()
            out[name + '|grad_proj_bias'] = PL.proj_net.bias.grad.numpy().copy()
        print(name, n_valid, 'valid target pixels', vals)
    path = os.path.join(OUT, 'pfgst_kernel_size.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_pfgst_kernel_size(load_reference())
