#!/usr/bin/env python3
"""Times the adversarial baseline at the flagship workload's shape -- 8 tiles, 6 classes, logits 256 x 256: every layer of
the FCDiscriminator (ndf 64) each way (forward with its LeakyReLU, data gradient with the gate, weight + bias gradient), the entropy map and
its adjoint, each as the mean over --iters calls between two device events, the median over --rounds; for the three layers with Cin, Cout
>= 64 the achieved fp32-MFMA rate beside the rate that the project's generic implicit GEMM (pfst_conv_igemm, 3x3) reaches on a layer of
similar MACs in the same run.  Then the bench-size steps on seeded synthetic tiles: `--adversarial advent`, `--supervised` and DACS, alternating
blocks in one process, host clock between device synchronisations.  One JSON line (and --out FILE).

  python tools/advent_bench.py [--tiles 8] [--classes 6] [--size 1024] [--iters 50] [--rounds 7] [--steps 12] [--no-step] [--no-kernels] [--out FILE]"""
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
    p.add_argument('--ndf', type=int, default=64)
    p.add_argument('--iters', type=int, default=50, help='calls between two device events')
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--steps', type=int, default=12, help='timed steps per kind')
    p.add_argument('--no-step', action='store_true')
    p.add_argument('--no-kernels', action='store_true')
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    import torch
    import pfst_amd  # noqa: F401
    res = dict(tiles=args.tiles, classes=args.classes, size=args.size, ndf=args.ndf, rounds=args.rounds, iters=args.iters,
               device=torch.cuda.get_device_name(0))
    if not args.no_kernels:
        res['kernels'] = kernel_bench(args)
    if not args.no_step:
        res['steps'] = step_bench(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


def kernel_bench(args):
    import torch
    from pfst_amd import hip_ops as ops
    N, C, s = args.tiles, args.classes, args.size // 4
    g = torch.Generator().manual_seed(0)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return 1000.0 * a.elapsed_time(b) / args.iters           # microseconds per call

    def bench(fns):
        """fns: {name: callable}; rounds alternate the order -> {name: dict(median, min, max)} in microseconds"""
        t = {k: [] for k in fns}
        names = list(fns)
        for i in range(2 + args.rounds):
            for k in (names if i % 2 == 0 else names[::-1]):
                v = timed(fns[k])
                if i >= 2:
                    t[k].append(v)
        return {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in t.items()}

    out = {}
    logits = (torch.randn(N, C, s, s, generator=g) * 2).cuda()
    ent, gl = ops.entropy_map(logits), torch.zeros_like(logits)
    out['entropy_map'] = bench(dict(forward=lambda: ops.entropy_map(logits, out=ent),
                                    backward=lambda: ops.entropy_map_bwd_(gl, logits, ent, accumulate=False)))
    widths = [C, args.ndf, args.ndf * 2, args.ndf * 4, args.ndf * 8, 1]
    x, layers = ent, []
    for i in range(5):
        cin, cout = widths[i], widths[i + 1]
        w = (torch.randn(cout, cin, 4, 4, generator=g) / (cin * 16) ** 0.5).cuda()
        b = torch.zeros(cout, device='cuda')
        y = ops.adv_conv(x, w, b, slope=0.2 if i < 4 else None)
        dy, dx, dw, db = torch.randn_like(y), torch.empty_like(x), torch.zeros_like(w), torch.zeros_like(b)
        r = bench(dict(forward=lambda x=x, w=w, b=b, y=y, i=i: ops.adv_conv(x, w, b, slope=0.2 if i < 4 else None, out=y),
                       dgrad=lambda dx=dx, dy=dy, w=w, x=x: ops.adv_conv_dgrad_(dx, dy, w, x_gate=x, slope=0.2),
                       wgrad=lambda dw=dw, db=db, x=x, dy=dy: ops.adv_conv_wgrad_(dw, db, x, dy)))
        macs = N * cout * y.shape[2] * y.shape[3] * cin * 16
        r.update(cin=cin, cout=cout, h=x.shape[2], w=x.shape[3], gmacs=round(macs / 1e9, 3))
        for k in ('forward', 'dgrad', 'wgrad'):
            r[k + '_tflops'] = round(2 * macs / (r[k]['median'] * 1e-6) / 1e12, 2)
        layers.append(r)
        x = y
    out['layers'] = layers
    # the project's generic fp32-MFMA implicit GEMM on a 3x3 layer of similar MACs to layer 2 (N x 128 x 64 x 64 from 64 channels x 16 taps):
    # 112 -> 128 channels, 3x3, 64 x 64 -- 112 is no multiple of 16, so pfst_conv_igemm takes the generic kernel of conv_mfma.hip
    from pfst_amd._lib import call
    cin, cout, hw = 112, 128, 64
    xi = torch.randn(N, cin, hw, hw, generator=g).cuda()
    wk = torch.randn(9 * cin, cout, generator=g).cuda()
    yo = torch.empty(N, cout, hw, hw, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    ref = bench(dict(forward=lambda: call('pfst_conv_igemm', xi.data_ptr(), cin * hw * hw, wk.data_ptr(), 0, yo.data_ptr(), cout * hw * hw, N, cin, hw, hw,
                                          cout, hw, hw, 3, 1, 1, 1, 0, 0, 0, 0, stream)))
    macs = N * cout * hw * hw * cin * 9
    out['generic_igemm_3x3'] = dict(cin=cin, cout=cout, h=hw, w=hw, gmacs=round(macs / 1e9, 3), forward=ref['forward'],
                                    forward_tflops=round(2 * macs / (ref['forward']['median'] * 1e-6) / 1e12, 2))
    for r in layers[1:4]:
        r['forward_fraction_of_generic_igemm'] = round(r['forward_tflops'] / out['generic_igemm_3x3']['forward_tflops'], 3)
    return out


def step_bench(args):
    """`--adversarial advent`, `--supervised` and DACS at the workload's size: blocks of steps alternate, a block starts and ends with a device
    synchronise"""
    import torch
    from pfst_amd.optim import build_optimizers
    from pfst_amd.presets import OPTIMIZER, advent_cfg, dacs_uda_cfg, model_cfg, workload_cfg
    from pfst_amd.registry import UDA, build_segmentor
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    _, w = workload_cfg(NAME)
    batch = synth_batch(args.tiles, args.size, w['num_classes'], w['in_channels'], seed=1234, device='cuda')
    sup_batch = {k: v for k, v in batch.items() if not k.startswith('target_')}
    adv = advent_cfg(model_cfg(w['num_classes'], w['in_channels']), ndf=args.ndf)
    kinds = {}
    for kind, build, opt_cfg, b in (('advent', lambda: build_segmentor(adv['model']), adv['optimizer'], batch),
                                    ('supervised', lambda: build_segmentor(model_cfg(w['num_classes'], w['in_channels'])), dict(OPTIMIZER), sup_batch),
                                    ('dacs', lambda: UDA.build(dacs_uda_cfg(w['num_classes'], w['in_channels'])), dict(OPTIMIZER), batch)):
        torch.manual_seed(0)
        model = build()
        disc = {k: v.clone() for k, v in model.state_dict().items() if k.startswith('discriminator.')}
        fill_state_dict(model.state_dict(), 0)
        model.load_state_dict(disc, strict=False)          # the discriminator keeps its default initialisation
        model.cuda()
        kinds[kind] = (model, build_optimizers(model, opt_cfg), b)
    times = {k: [] for k in kinds}
    logs = {}

    def run(kind, n, keep):
        model, opt, b = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            logs[kind] = model.train_step(b, opt)['log_vars']
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
    out['last_log'] = {k: {n: float(v) for n, v in logs[k].items()} for k in kinds}
    return out


if __name__ == '__main__':
    main()
