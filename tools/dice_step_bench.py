#!/usr/bin/env python3
"""The supervised step with CrossEntropyLoss heads beside the same step with [CrossEntropyLoss, DiceLoss] in both heads, in ONE process on one
box at the flagship workload's size (b = 8 x 1024^2 unless --batch / --size): blocks of steps of the two alternate as in
tools/supervised_step_bench.py (every block starts and ends with a device synchronise, every step is timed by the host clock), the median
per kind over all blocks is printed as one JSON line.  --terms chooses what the second step lists after its CE term: any of dice, focal (the
FocalLoss defaults) and bce (CrossEntropyLoss(use_sigmoid=True)), comma-separated, in that order -- `--terms focal` is the cost of a Focal term.

    python tools/dice_step_bench.py [--steps 24] [--blocks 4] [--warmup 3] [--batch 8] [--size 1024] [--terms dice]"""
import argparse
import copy
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAME = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', type=int, default=24, help='timed steps per kind, over all blocks')
    ap.add_argument('--blocks', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--size', type=int, default=None)
    ap.add_argument('--terms', default='dice', help='the terms listed after CE in the second step: dice, focal, bce (comma-separated)')
    args = ap.parse_args()
    extra = {'dice': lambda lw: dict(type='DiceLoss', loss_weight=lw), 'focal': lambda lw: dict(type='FocalLoss', loss_weight=lw),
             'bce': lambda lw: dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=lw, loss_name='loss_bce')}
    terms = [t.strip() for t in args.terms.split(',') if t.strip()]
    if not terms or any(t not in extra for t in terms):
        ap.error(f'--terms takes a comma-separated list of {sorted(extra)}, got {args.terms!r}')
    listed = 'ce_' + '_'.join(terms)
    import numpy as np
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import SGD_OPTIMIZER, workload_cfg
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    cfg, w = workload_cfg(NAME)
    b, size = args.batch or w['per_gpu_batch'], args.size or w['size']
    batch = {k: v for k, v in synth_batch(b, size, w['num_classes'], w['in_channels'], seed=1234, device='cuda').items() if not k.startswith('target_')}
    random.seed(0); np.random.seed(0); torch.manual_seed(0); torch.cuda.manual_seed_all(0)
    kinds = {}
    for kind in ('ce', listed):
        mcfg = copy.deepcopy(cfg['model'])
        if kind == listed:
            for head, lw in (('decode_head', 3.0), ('auxiliary_head', 1.2)):
                mcfg[head]['loss_decode'] = [dict(mcfg[head]['loss_decode'])] + [extra[t](lw) for t in terms]
        model = build_segmentor(mcfg)
        fill_state_dict(model.state_dict(), 0)
        model.cuda()
        kinds[kind] = (model, build_optimizer(model, dict(SGD_OPTIMIZER, lr=6e-5)))      # timed, not trained: supervised_step_bench.py's rate
    times = {k: [] for k in kinds}

    def run(kind, n, keep):
        model, opt = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            model.train_step(batch, opt)
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
    res = dict(batch=b, size=size, steps_per_kind=len(times['ce']), blocks=args.blocks)
    for kind, v in times.items():
        res[kind] = dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2))
    res['_'.join(terms) + '_adds_ms'] = round(res[listed]['median_ms'] - res['ce']['median_ms'], 2)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
