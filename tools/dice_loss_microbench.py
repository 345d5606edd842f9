"""The Dice loss kernels beside their CE counterparts at the bench workload's two head shapes (8 x 6 x 256^2 -> 1024^2, the decode head; 8 x 6 x
128^2 -> 1024^2, the auxiliary head), in ONE process, timed on device events (median).  Per shape one JSON line: ce_upsample_fwd /
ce_upsample_bwd, then dice_upsample_fwd / dice_finalize / dice_upsample_bwd reading the CE term's log-sum-exp ("shared") and forming their own
("own": 4 B per pixel more, written by the forward kernel).  The wrappers' small allocations are inside every figure, as in
tools/small_kernel_probe.py.

    python tools/dice_loss_microbench.py [--reps N] [--exponent E]"""
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
    ap.add_argument('--exponent', type=float, default=2.0)
    args = ap.parse_args()
    from pfst_amd import hip_ops as ops
    b, C, S, e = 8, 6, 1024, args.exponent
    g = torch.Generator(device='cuda').manual_seed(0)
    lab = torch.randint(0, C, (b, 1, S // 64, S // 64), device='cuda', generator=g)
    lab = ops.to_u8(lab.repeat_interleave(64, 2).repeat_interleave(64, 3).contiguous())
    lab[:, :, :32, :] = 255
    for lo in (S // 4, S // 8):
        lg = torch.randn(b, C, lo, lo, device='cuda', generator=g)
        lse, _ = ops.ce_upsample_fwd(lg, lab)
        out = torch.empty_like(lg)
        row = dict(shape=f'{b} x {C} x {lo}^2 -> {S}^2', exponent=e, form=ops.dice_form(lg, lab, lse)[0])
        row['ce_fwd_us'] = timeit(lambda: ops.ce_upsample_fwd(lg, lab), args.reps)
        row['ce_bwd_us'] = timeit(lambda: ops.ce_upsample_bwd(lg, lab, lse, 1e-3, out=out), args.reps)
        for tag, shared in (('shared', lse), ('own', None)):
            slab, counts, ls, _ = ops.dice_upsample_fwd(lg, lab, 255, 255, e, lse=shared)
            _, coef, _ = ops.dice_finalize(slab, counts, None, 255, 1.0, e, 1.0)
            row[f'dice_fwd_{tag}_us'] = timeit(lambda: ops.dice_upsample_fwd(lg, lab, 255, 255, e, lse=shared), args.reps)
            row[f'dice_finalize_{tag}_us'] = timeit(lambda: ops.dice_finalize(slab, counts, None, 255, 1.0, e, 1.0), args.reps)
            row[f'dice_bwd_{tag}_us'] = timeit(lambda: ops.dice_upsample_bwd(lg, lab, ls, coef, 1e-3, 255, e, out=out), args.reps)
        row['dice_fwd_over_ce_fwd'] = round(row['dice_fwd_shared_us'] / row['ce_fwd_us'], 2)
        row['dice_bwd_over_ce_bwd'] = round(row['dice_bwd_shared_us'] / row['ce_bwd_us'], 2)
        row['partial_rows_per_image'] = slab.shape[1]
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
