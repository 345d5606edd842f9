#!/usr/bin/env python3
"""Same-box A/B of layers.WINO_SHARE_DY (the data gradient of the f16x3 Winograd layers from the weight gradient's dM):
the recipe behind profiles/wino_shared_dy_ab.txt and the two kernel tables beside it.  The switch is a module constant, not an
environment variable, so every leg is a fresh process that sets it and then runs bench.main with the given bench.py arguments.

  python tools/ab_wino_shared_dy.py --pairs 4
      off / on alternating, each leg `bench.py --gpus 1 --steps 8 --warmup 3 --full --no-cpu-baseline --no-alt-math --dump-outputs DIR`:
      one line per leg (images/s, ms per step, the touched kernels' ms and launches per step from the table pass, peak memory), then the
      largest differences between the dumped outputs of legs and of repeated runs of one leg
  python tools/ab_wino_shared_dy.py --leg off -- --gpus 1 --steps 15 --warmup 5
      ONE leg with bench.py's own output: the command to put behind `rocprofv3 --kernel-trace --stats --` for a leg's kernel table"""
import argparse
import contextlib
import glob
import io
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ('pfst_wino_input', 'pfst_wino_dy', 'pfst_bn_backward', 'pfst_wino_dx', 'pfst_wino_output')
AB_ARGS = ['--gpus', '1', '--steps', '8', '--warmup', '3', '--full', '--no-cpu-baseline', '--no-alt-math']


def run_leg(leg, bench_args, summary):
    """this process becomes the leg: set the switch, run bench.main; summary: print the A/B line instead of bench.py's JSON line"""
    from pfst_amd import layers
    layers.WINO_SHARE_DY = leg == 'on'
    import bench
    table = {}
    inner = bench.KernelTimer.summary

    def capture(self):                       # the table pass's full per-kernel table (bench.py's JSON line keeps the top 14 only)
        agg = inner(self)
        if len(agg) > 20:
            table.clear()
            table.update({k: (v[0], v[1]) for k, v in agg.items()})
        return agg
    bench.KernelTimer.summary = capture
    sys.argv = ['bench.py'] + bench_args
    if not summary:
        return bench.main()
    steps = int(bench_args[bench_args.index('--steps') + 1])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        bench.main()
    d = json.loads(out.getvalue().strip().splitlines()[-1])
    ms = {n: round(sum(v[1] for k, v in table.items() if k.split(' ')[0] == n) / steps, 3) for n in KERNELS}
    calls = {n: sum(v[0] for k, v in table.items() if k.split(' ')[0] == n) / steps for n in KERNELS}
    print(leg, round(d['value'], 3), round(d['ms_per_step'], 2), ms, 'calls/step', calls, 'hbm_peak_allocated_GB', d.get('hbm_peak_allocated_GB'),
          flush=True)


def compare(a, b):
    """largest relative difference between two --dump-outputs directories: log values |a - b| / max(|b|, 1e-2); sampled weights norm-wise"""
    import numpy as np
    log, wts = (0.0, ''), (0.0, '')
    for p in sorted(glob.glob(os.path.join(a, '*.npy'))):
        name = os.path.basename(p)
        x, y = np.load(p).astype(np.float64), np.load(os.path.join(b, name)).astype(np.float64)
        if name.startswith('log_vars'):
            log = max(log, (float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-2)), name))
        else:
            wts = max(wts, (float(np.linalg.norm(x - y) / (np.linalg.norm(y) + 1e-30)), name))
    return f'log values {log[0]:.1e} ({log[1]})  weights {wts[0]:.1e} ({wts[1]})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=4)
    ap.add_argument('--leg', choices=['on', 'off'], default=None, help='run this one leg in this process')
    ap.add_argument('--summary', action='store_true', help='with --leg: the A/B line instead of bench.py\'s output')
    ap.add_argument('bench_args', nargs='*', help='with --leg, after `--`: bench.py\'s arguments')
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.leg, args.bench_args or AB_ARGS, args.summary)
    with tempfile.TemporaryDirectory() as tmp:
        dumps = {'on': [], 'off': []}
        for i in range(args.pairs):
            for leg in ('off', 'on'):
                d = os.path.join(tmp, f'{leg}{i}')
                # a leg that fails ends the A/B: nothing more is started on the device behind it
                subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg, '--summary', '--'] + AB_ARGS + ['--dump-outputs', d],
                               check=True, stderr=subprocess.DEVNULL, timeout=600)
                dumps[leg].append(d)
        print('# largest relative difference of the last timed step\'s outputs (bound between arithmetics in tests/test_train_step_gpu.py: 1e-3)')
        for i in range(args.pairs):
            print(f'# on  run {i} vs off run {i}:', compare(dumps['on'][i], dumps['off'][i]))
        if args.pairs > 1:
            print('# off run 1 vs off run 0:', compare(dumps['off'][1], dumps['off'][0]))
            print('# on  run 1 vs on  run 0:', compare(dumps['on'][1], dumps['on'][0]))


if __name__ == '__main__':
    main()
