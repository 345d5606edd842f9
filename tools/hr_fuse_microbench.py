#!/usr/bin/env python3
"""Times HRNet's fused exchange unit (csrc/hrnet.hip) at the stage-4 i = 0 output of HRNet-W18 for the 8 x 1024^2 tile --
8 x 18 x 256 x 256 with three coarser members on 128^2 / 64^2 / 32^2, a [C, 4] table on each -- beside the composition of library ops it
replaces (three bn_apply(relu=False), three resize_bilinear that each write a fine map, three adds -- the last one fused with the ReLU in a
bn_apply with identity coefficients), and the backward (gate + one gather) beside gate + three resize_bilinear_bwd.  Variants alternate inside every round; per variant
the median, minimum and maximum over the rounds of the mean of --inner back-to-back runs between two device events; achieved bytes per second
from the bytes the shapes say must move.  One JSON line (and --out FILE).

  python tools/hr_fuse_microbench.py [--tiles 8] [--width 18] [--grid 256] [--rounds 7] [--inner 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--tiles', type=int, default=8)
    p.add_argument('--width', type=int, default=18)
    p.add_argument('--grid', type=int, default=256)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--inner', type=int, default=5)
    p.add_argument('--out')
    args = p.parse_args(argv)
    import torch
    from heads_bench import alternate, verdict
    from pfst_amd import hip_ops as ops
    n, c, g = args.tiles, args.width, args.grid
    gen = torch.Generator().manual_seed(0)
    x0 = torch.randn(n, c, g, g, generator=gen).cuda()
    members = [torch.randn(n, c, g >> k, g >> k, generator=gen).cuda() for k in (1, 2, 3)]
    tables = [torch.stack([torch.zeros(c), torch.ones(c), torch.rand(c, generator=gen) + 0.5, torch.randn(c, generator=gen)], 1).contiguous().cuda()
              for _ in members]
    out = torch.empty_like(x0)
    one, zero = torch.ones(c, device='cuda'), torch.zeros(c, device='cuda')
    slots = ops.amax_slots('cuda')

    def fused():
        ops.hr_fuse([x0] + members, [None] + tables, out=out, amax=slots)

    def composed():
        # the issue's composition: three bn_apply, three resize_bilinear that each write a fine map, three adds, a ReLU -- the first add out of
        # place (an identity-coefficient bn_apply with x0 as its residual), the last add and the ReLU in one pass: no pass beyond the list
        ts = [ops.resize_bilinear(ops.bn_apply(m, t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(), t[:, 3].contiguous(), False),
                                  (g, g)) for m, t in zip(members, tables)]
        part = ops.bn_apply(ts[0], zero, one, one, zero, False, residual=x0)
        ops.axpy_(part, ts[1])
        ops.bn_apply(ts[2], zero, one, one, zero, True, residual=part, out=out, amax=slots)
    fused()
    want = out.clone()
    composed()
    assert torch.equal(out, want), 'the fused launch and the composition differ'
    fine, coarse = 4 * x0.numel(), sum(4 * m.numel() for m in members)
    res = dict(shape=[n, c, g, g])
    fwd = alternate(dict(fused=fused, composed=composed), args.rounds, args.inner)
    verdict(fwd, 'fused', ['composed'], 2 * fine + coarse)
    res['forward'] = fwd
    d_out = torch.randn(n, c, g, g, generator=gen).cuda()
    gy = torch.empty_like(d_out)
    grads = [torch.empty_like(m) for m in members]

    def fused_bwd():
        ops.hr_fuse_bwd(d_out, want, grads, gy=gy)

    def composed_bwd():
        ops.hr_fuse_bwd(d_out, want, gy=gy)
        for m, gm in zip(members, grads):
            ops.resize_bilinear_bwd(gy, m.shape[-2:], out=gm)
    bwd = alternate(dict(fused=fused_bwd, composed=composed_bwd), args.rounds, args.inner)
    verdict(bwd, 'fused', ['composed'], 4 * fine + coarse)          # d_out, out read, gy written, gy read by the gather; the coarse gradients written
    res['backward'] = bwd
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
