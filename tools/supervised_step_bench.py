#!/usr/bin/env python3
"""The supervised step (EncoderDecoder.train_step under SGD) beside the PFGST step (under AdamW) in ONE process on one box, the flagship
workload's size (b = 8 x 1024^2 unless --batch / --size): blocks of steps of the two alternate, every block starts and ends with a device synchronise and
every step in it is timed by the host clock, the median per kind over all blocks is printed as one JSON line.

    python tools/supervised_step_bench.py [--steps 24] [--blocks 3] [--warmup 3] [--batch 8] [--size 1024]

The supervised step runs a strict subset of the PFGST step's launches (one student pass of its two, no teacher, no class mix, no PFGSTLoss):
a supervised median above the PFGST median on the same box is a defect.  Under `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/supervised_step_bench.py --steps 4 --blocks 1` the trace holds `sgd_kernel` and `adamw_kernel` side by side; `--rates CSV` reads the
kernel-stats file of such a run and prints both kernels' average duration and achieved HBM rate (SGD with momentum: 5 arrays of
n floats per step -- 3 read, 2 written; 4 on the first step, which does not read the buffer; AdamW: 7 -- 4 read, 3 written)."""
import argparse
import csv
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


def rates(path, n):
    """kernel_stats.csv of rocprofv3 --kernel-trace --stats -> {kernel: calls, average us, TB/s}"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row.get('Name') or row.get('KernelName') or ''
        for key, arrays in (('sgd_kernel', 5), ('adamw_kernel', 7)):
            if key in name:
                avg_ns = float(row.get('AverageNs') or row.get('Average') or 0.0)
                out[name] = dict(calls=int(float(row.get('Calls') or 0)), average_us=round(avg_ns / 1e3, 2), arrays=arrays,
                                 min_us=round(float(row.get('MinNs') or 0.0) / 1e3, 2), max_us=round(float(row.get('MaxNs') or 0.0) / 1e3, 2),
                                 TB_per_s=round(arrays * 4 * n / max(avg_ns, 1e-9) / 1e3, 3))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=24, help='timed steps per kind, over all blocks')
    ap.add_argument('--blocks', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--size', type=int, default=None)
    ap.add_argument('--rates', help='kernel_stats.csv of a rocprofv3 run of this tool: print the optimizer kernels\' rates and exit')
    args = ap.parse_args()
    import numpy as np
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import OPTIMIZER, SGD_OPTIMIZER, model_cfg, workload_cfg
    from pfst_amd.registry import UDA, build_segmentor
    cfg, w = workload_cfg(NAME)
    if args.rates:
        n = sum((p.numel() + 3) // 4 * 4 for p in build_segmentor(model_cfg(w['num_classes'], w['in_channels'])).parameters())
        print(json.dumps(dict(arena_floats=n, kernels=rates(args.rates, n))))
        return
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    b, size = args.batch or w['per_gpu_batch'], args.size or w['size']
    batch = synth_batch(b, size, w['num_classes'], w['in_channels'], seed=1234, device='cuda')
    sup_batch = {k: v for k, v in batch.items() if not k.startswith('target_')}
    random.seed(0); np.random.seed(0); torch.manual_seed(0); torch.cuda.manual_seed_all(0)
    uda = UDA.build(cfg)
    fill_state_dict(uda.state_dict(), 0)
    uda.cuda()
    sup = build_segmentor(cfg['model'])
    fill_state_dict(sup.state_dict(), 0)
    sup.cuda()
    # AdamW's 6e-5 for both: the steps are timed, not trained, and the supervised schedule's 0.01 on a random-init network would leave
    # later steps with other (overflowing) operand ranges than the PFGST leg's
    kinds = dict(pfgst=(uda, build_optimizer(uda, OPTIMIZER), batch),
                 supervised=(sup, build_optimizer(sup, dict(SGD_OPTIMIZER, lr=6e-5)), sup_batch))
    times = {k: [] for k in kinds}

    def run(kind, n, keep):
        # a block: synchronise, n steps back to back (a step returns after its blocking read of the forward results, while its backward sweep
        # and update are still queued: the product's step-boundary overlap stays in the measurement), synchronise; a step's time is the host
        # clock between two returns, the last one's includes the drain
        model, opt, data = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            model.train_step(data, opt)
            if i == n - 1:
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            if keep:
                times[kind].append(1000.0 * (t1 - t0))
            t0 = t1

    for kind in kinds:
        run(kind, args.warmup, False)
    per_block = -(-args.steps // args.blocks)
    for blk in range(args.blocks):
        for kind in (list(kinds) if blk % 2 == 0 else list(kinds)[::-1]):          # alternate, rotating the order
            run(kind, per_block, True)
    res = dict(batch=b, size=size, steps_per_kind=len(times['pfgst']), blocks=args.blocks)
    for kind, v in times.items():
        res[kind] = dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2))
    res['supervised_over_pfgst'] = round(res['supervised']['median_ms'] / res['pfgst']['median_ms'], 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
