#!/usr/bin/env python3
"""Times EntropyLoss (csrc/entropy_loss.hip) at the flagship workload's shape -- the mixed pass's logits of the bench step:
8 tiles, 6 classes, 256 x 256 -- forward (two launches) and backward (one launch, accumulating), each as the mean over --iters calls between
two device events, the median over --rounds; both loss types.  Then the bench-size self-training steps on seeded synthetic tiles: PFGST as
shipped (auxiliary losses [PFGSTLoss]), PFGST with [PFGSTLoss, EntropyLoss] and DACS, alternating blocks in one process, host clock between
device synchronisations.  One JSON line (and --out FILE).

  python tools/entropy_loss_bench.py [--tiles 8] [--classes 6] [--size 1024] [--iters 200] [--rounds 9] [--steps 12] [--no-step] [--out FILE]

Bytes, from the shapes (L = tiles x classes x (size / 4)^2 x 4 bytes of logits, 12.6 MB at the defaults): the forward reads L; the backward
reads L and reads, modifies and writes L of gradient.  L is smaller than the last-level cache, so repeated calls on one buffer need not go to
HBM: the rates are what the calls achieve on resident data, as in the step, where the logits were written a moment earlier.
The per-call figures include the launch path (a call is two allocations and two launches forward, one launch backward: at 5 - 8 us per
launch the host, not the device, can set them); the kernels' own durations come from a trace run of its own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/entropy_loss_bench.py --no-step --iters 50 --rounds 3`."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--tiles', type=int, default=8)
    p.add_argument('--classes', type=int, default=6)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--iters', type=int, default=200, help='calls between two device events')
    p.add_argument('--rounds', type=int, default=9)
    p.add_argument('--steps', type=int, default=12, help='timed steps per kind')
    p.add_argument('--weight', type=float, default=0.01, help='EntropyLoss weight of the step with the term (the timing does not depend on it)')
    p.add_argument('--no-step', action='store_true')
    p.add_argument('--no-term', action='store_true')
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    import torch
    import pfst_amd  # noqa: F401
    res = dict(tiles=args.tiles, classes=args.classes, size=args.size, rounds=args.rounds, iters=args.iters, device=torch.cuda.get_device_name(0))
    if not args.no_term:
        res['kernels'] = term_bench(args)
    if not args.no_step:
        res['steps'] = step_bench(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


def term_bench(args):
    import torch
    from pfst_amd import hip_ops as ops
    N, C, s = args.tiles, args.classes, args.size // 4
    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(N, C, s, s, generator=g) * 2).cuda()
    grad = torch.zeros_like(logits)
    L = logits.numel() * 4
    out = dict(logit_MB=round(L / 1e6, 2), forward_read_MB=round(L / 1e6, 2), backward_read_MB=round(2 * L / 1e6, 2),
               backward_write_MB=round(L / 1e6, 2))
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / args.iters           # microseconds per call

    for kind in ('entropy', 'max_square'):
        fwd = lambda: ops.softmax_entropy(logits, kind, 1.0)
        bwd = lambda: ops.softmax_entropy_bwd_(grad, logits, kind, 1.0, grad_scale=0.0, accumulate=True)      # read-modify-write, values kept
        t = dict(forward=[], backward=[])
        for i in range(2 + args.rounds):
            for name, fn in ((('forward', fwd), ('backward', bwd)) if i % 2 == 0 else (('backward', bwd), ('forward', fwd))):
                v = timed(fn)
                if i >= 2:
                    t[name].append(v)
        r = dict(loss=float(ops.softmax_entropy(logits, kind, 1.0)))
        for name, v in t.items():
            r[name + '_us'] = dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
        r['forward_TB_per_s'] = round(L / (r['forward_us']['median'] * 1e-6) / 1e12, 3)
        r['backward_TB_per_s'] = round(3 * L / (r['backward_us']['median'] * 1e-6) / 1e12, 3)
        out[kind] = r
    return out


def step_bench(args):
    """PFGST [PFGSTLoss] (the step bench.py times), PFGST [PFGSTLoss, EntropyLoss] and DACS at the workload's size: blocks of steps alternate, a
    block starts and ends with a device synchronise"""
    import torch
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import OPTIMIZER, dacs_uda_cfg, workload_cfg
    from pfst_amd.registry import UDA
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    cfg, w = workload_cfg(NAME)
    batch = synth_batch(args.tiles, args.size, w['num_classes'], w['in_channels'], seed=1234, device='cuda')
    with_term = workload_cfg(NAME)[0]
    with_term['aux_losses'].append(dict(type='EntropyLoss', loss_type='entropy', weights={'loss_ent': args.weight}))
    kinds = {}
    for kind, c in (('pfgst', cfg), ('pfgst_entropy', with_term), ('dacs', dacs_uda_cfg(w['num_classes'], w['in_channels']))):
        torch.manual_seed(0)
        model = UDA.build(c)
        fill_state_dict(model.state_dict(), 0)
        model.cuda()
        kinds[kind] = (model, build_optimizer(model, dict(OPTIMIZER)))
    times = {k: [] for k in kinds}
    logs = {}

    def run(kind, n, keep):
        model, opt = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            logs[kind] = model.train_step(batch, opt)['log_vars']
        torch.cuda.synchronize()
        if keep:
            times[kind].append(1000.0 * (time.perf_counter() - t0) / n)

    for kind in kinds:
        run(kind, 3, False)
    blocks, per_block = 4, -(-args.steps // 4)
    order = list(kinds)
    for blk in range(blocks):
        for kind in order[blk % 3:] + order[:blk % 3]:
            run(kind, per_block, True)
    out = dict(steps_per_block=per_block, blocks=blocks)
    for kind, v in times.items():
        out[kind] = dict(median_ms_per_step=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
    out['entropy_term_ms'] = round(out['pfgst_entropy']['median_ms_per_step'] - out['pfgst']['median_ms_per_step'], 2)
    out['last_log'] = {k: {n: float(v) for n, v in logs[k].items()} for k in kinds}
    return out


if __name__ == '__main__':
    main()
