"""The sigmoid loss kernels (FocalLoss, CrossEntropyLoss(use_sigmoid)) beside their CE counterparts at the bench workload's two head shapes
(8 x 6 x 256^2 -> 1024^2, the decode head; 8 x 6 x 128^2 -> 1024^2, the auxiliary head), in ONE process, timed on device events (median).
Per shape one JSON line: ce_upsample_fwd / ce_upsample_bwd, then sigloss_upsample_fwd / sigloss_finalize / sigloss_upsample_bwd at gamma = 2
with a scalar alpha (the FocalLoss default), at a general gamma (--gamma, default 1.5) and at gamma = 0 (the BCE form), and each kernel's time
over its CE counterpart.  The bars of DESIGN.md section 8k: 2x at gamma = 2, 3x at a general gamma.  --weights times every kernel with a
pixel-weight map (a quarter of it exact zeros, in 4 x 4 blocks).  The wrappers' small allocations are inside every figure, as in
tools/dice_loss_microbench.py.

    python tools/sigmoid_loss_microbench.py [--reps N] [--gamma G] [--weights]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def timeit(fn, reps):
    for _ in range(3):
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
    return round(1e3 * t[len(t) // 2], 1)          # median, us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--gamma', type=float, default=1.5, help='the general-gamma point (neither 0 nor 2)')
    ap.add_argument('--weights', action='store_true')
    args = ap.parse_args()
    from pfst_amd import hip_ops as ops
    b, C, S = 8, 6, 1024
    g = torch.Generator(device='cuda').manual_seed(0)
    lab = torch.randint(0, C, (b, 1, S // 64, S // 64), device='cuda', generator=g)
    lab = ops.to_u8(lab.repeat_interleave(64, 2).repeat_interleave(64, 3).contiguous())
    lab[:, :, :32, :] = 255
    pw = None
    if args.weights:
        blocks = torch.rand(b, S // 4, S // 4, device='cuda', generator=g)
        blocks[torch.rand(blocks.shape, device='cuda', generator=g) < 0.25] = 0.0
        pw = blocks.repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    focal = torch.tensor([[0.5, 0.5]] * C, device='cuda')              # alpha = 0.5, no class weights
    bce = torch.tensor([[1.0, 1.0]] * C, device='cuda')
    for lo in (S // 4, S // 8):
        lg = torch.randn(b, C, lo, lo, device='cuda', generator=g)
        lse, _ = ops.ce_upsample_fwd(lg, lab, pw)
        out = torch.empty_like(lg)
        D = float(b * C * S * S)
        row = dict(shape=f'{b} x {C} x {lo}^2 -> {S}^2', weights=bool(args.weights), form=ops.sigloss_form(lg, lab, pw)[0])
        row['ce_fwd_us'] = timeit(lambda: ops.ce_upsample_fwd(lg, lab, pw), args.reps)
        row['ce_bwd_us'] = timeit(lambda: ops.ce_upsample_bwd(lg, lab, lse, 1e-3, pw, out=out), args.reps)
        for tag, coef, gamma, bar in (('g2', focal, 2.0, 2.0), ('general', focal, args.gamma, 3.0), ('g0', bce, 0.0, 2.0)):
            slab, counts, _ = ops.sigloss_upsample_fwd(lg, lab, coef, gamma, pw)
            row[f'{tag}_gamma'] = gamma
            row[f'{tag}_fwd_us'] = timeit(lambda: ops.sigloss_upsample_fwd(lg, lab, coef, gamma, pw), args.reps)
            row[f'{tag}_finalize_us'] = timeit(lambda: ops.sigloss_finalize(slab, counts, D, 1.0), args.reps)
            row[f'{tag}_bwd_us'] = timeit(lambda: ops.sigloss_upsample_bwd(lg, lab, coef, 1e-3, gamma, pw, out=out), args.reps)
            row[f'{tag}_fwd_over_ce_fwd'] = round(row[f'{tag}_fwd_us'] / row['ce_fwd_us'], 2)
            row[f'{tag}_bwd_over_ce_bwd'] = round(row[f'{tag}_bwd_us'] / row['ce_bwd_us'], 2)
            row[f'{tag}_bar'] = bar
            row[f'{tag}_within_bar'] = max(row[f'{tag}_fwd_over_ce_fwd'], row[f'{tag}_bwd_over_ce_bwd']) <= bar
        row['partial_rows_per_image'] = slab.shape[1]
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
