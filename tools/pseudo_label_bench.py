#!/usr/bin/env python3
"""Times the three kernels of csrc/entropy_labels.hip at a user's size -- 16 tiles, 6 classes, 256^2 logits to 1024^2 pixels
-- beside the composition the library offered for the same numbers before them: `resize_bilinear` + `softmax_nchw` + torch's entropy and
arg-max over the full-resolution tensors + `torch.sort` per class.  Device events, the median of --repeat timed runs after --warmup
untimed ones; one JSON line (and --out FILE).

  python tools/pseudo_label_bench.py [--tiles 16] [--classes 6] [--low 256] [--size 1024] [--repeat 20] [--warmup 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeat, warmup):
    """median milliseconds of fn() between two device events"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--tiles', type=int, default=16)
    p.add_argument('--classes', type=int, default=6)
    p.add_argument('--low', type=int, default=256)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--repeat', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    import numpy as np
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd import hip_ops as ops
    from pfst_amd.pseudo_labels import ClassEntropyThresholds, label_maps, radix_levels
    N, C, size = args.tiles, args.classes, (args.size, args.size)
    logits = (torch.randn(N, C, args.low, args.low, generator=torch.Generator().manual_seed(0)) * 3).cuda()
    levels = radix_levels(C)
    acc = ClassEntropyThresholds(C).add(logits, size)
    table, n_c = acc.thresholds([0.5])
    thr = torch.from_numpy(table[0]).cuda()
    prefix = (torch.from_numpy(table[0]).view(torch.int32) >> levels[1][0] + levels[1][1]).to(torch.int32).cuda()
    hists = [torch.zeros(C, 1 << b, dtype=torch.int64, device='cuda') for _, b in levels]
    counts = torch.zeros(C, 2, dtype=torch.int64, device='cuda')
    res = dict(tiles=N, classes=C, low=args.low, size=args.size, pixels=N * args.size ** 2, radix_levels=[list(l) for l in levels],
               repeat=args.repeat, device=torch.cuda.get_device_name(0))
    res['entropy_upsample_mode0'] = timed(lambda: ops.entropy_upsample(logits, size, 0), args.repeat, args.warmup)
    res['entropy_upsample_mode1_entropy_only'] = timed(lambda: ops.entropy_upsample(logits, size, 1, want_pred=False), args.repeat, args.warmup)
    res['class_hist_top_level'] = timed(lambda: ops.entropy_class_hist(logits, size, *levels[0], hists[0]), args.repeat, args.warmup)
    res['class_hist_second_level'] = timed(lambda: ops.entropy_class_hist(logits, size, *levels[1], hists[1], prefix), args.repeat, args.warmup)
    res['pseudo_label'] = timed(lambda: label_maps(logits, size, thr, counts=counts), args.repeat, args.warmup)
    res['thresholds_one_ratio_with_reads'] = timed(lambda: acc.thresholds([0.5]), args.repeat, args.warmup)
    res['thresholds_seven_ratios_with_reads'] = timed(lambda: acc.thresholds([0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5]), args.repeat, args.warmup)

    # the composition: full-resolution logits, probabilities, entropy and arg-max in HBM, then one sort per class
    def composed_entropy():
        up = ops.resize_bilinear(logits, size)
        pr = ops.softmax_nchw(up)
        ent = -(pr * torch.log(pr)).sum(dim=1)
        return ent, pr.argmax(dim=1)

    def composed_thresholds():
        ent, pred = composed_entropy()
        out = []
        for c in range(C):
            s = torch.sort(ent[pred == c]).values
            out.append(s[int(s.numel() * 0.5)] if s.numel() else ent.new_zeros(()))
        return torch.stack(out)

    res['composed_entropy_and_argmax'] = timed(composed_entropy, args.repeat, args.warmup)
    res['composed_thresholds_one_ratio'] = timed(composed_thresholds, args.repeat, args.warmup)
    got = composed_thresholds().cpu().numpy()
    res['composed_vs_select_max_abs_diff'] = float(np.abs(got - table[0]).max())
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
