"""PFGSTLoss forward + backward kernels at the bench workload's shapes (b = 8, 1024^2 tiles: 512 x 128 x 128 decoded features,
6-class logits at 256 x 256, downscale 0.5, dilation 2, cosine, top_k 3, detach_unfold) for kernel_size 3 / 5 / 7, timed on device
events.  One line per kernel size: the whole loss (the module's forward + its backward closure), and the similarity map and its
adjoint alone with the bytes they move (the feature map is read once per map; the adjoint also writes d features).

    python tools/pfgst_loss_microbench.py [--reps N]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e))
    t.sort()
    return t[len(t) // 2]                       # median, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--ksizes', default='3,5,7')
    args = ap.parse_args()
    from pfst_amd import hip_ops as ops
    from pfst_amd.engine import Tape, Var
    from pfst_amd.uda import PFGSTLoss
    b, c, S, ncls, dil = 8, 512, 1024, 6, 2
    g = torch.Generator(device='cuda').manual_seed(0)
    x_src = torch.randn(b, c, S // 8, S // 8, device='cuda', generator=g)
    x_ema = torch.randn(b, c, S // 8, S // 8, device='cuda', generator=g)
    logits = torch.randn(b, ncls, S // 4, S // 4, device='cuda', generator=g)
    gt = torch.randint(0, ncls, (b, 1, S // 64, S // 64), device='cuda', generator=g)
    gt = ops.to_u8(gt.repeat_interleave(64, 2).repeat_interleave(64, 3).contiguous())
    mm = ops.to_u8((torch.rand(b, 1, 2, 2, device='cuda', generator=g) > 0.5).long().repeat_interleave(S // 2, 2).repeat_interleave(S // 2, 3)
                   .contiguous())
    fbytes = x_src.numel() * 4
    weights = {k: 0.1 for k in ('src_pos', 'src_neg', 'sim_pos', 'sim_neg', 'src_pos_std', 'src_neg_std')}
    for ks in [int(k) for k in args.ksizes.split(',')]:
        loss = PFGSTLoss(top_k=3, dilation=dil, kernel_size=ks, weights=weights, sim_type='cosine', feat_level=None,
                         detach_unfold=True, downscale=0.5)
        fd = dil                                   # features at 1/8 = the loss grid of downscale 0.5: no replication

        def step():
            lt, xs, xe = Var(logits, True), Var(x_src, True), Var(x_ema, False)
            tape = Tape()
            loss(dict(logits_trg=lt, x_ema=xe, x_src=xs, gt_src=gt, mix_masks=mm), tape)
            tape.backward()

        t_step = timeit(step, args.reps)
        sim, norm = ops.sim_map(x_src, fd, ksize=ks)
        gsim = torch.randn_like(sim)
        dx = torch.empty_like(x_src)
        t_map = timeit(lambda: ops.sim_map(x_src, fd, ksize=ks), args.reps)
        t_adj = timeit(lambda: ops.sim_map_bwd(x_src, sim, norm, gsim, fd, out=dx, ksize=ks), args.reps)
        row = dict(kernel_size=ks, loss_fwd_bwd_ms=round(t_step, 3), sim_map_us=round(t_map * 1e3, 1),
                   sim_map_read_MB=round(fbytes / 1e6, 1), sim_map_GBps=round(fbytes / t_map / 1e6),
                   sim_map_bwd_us=round(t_adj * 1e3, 1), sim_map_bwd_read_write_MB=round(2 * fbytes / 1e6, 1),
                   sim_map_bwd_GBps=round(2 * fbytes / t_adj / 1e6))
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
