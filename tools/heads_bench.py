#!/usr/bin/env python3
"""Times the four pyramid operations of PSPHead (csrc/pyramid.hip) at the flagship tile's shape -- N = 8, a 128 x 128 grid,
scales (1, 2, 3, 6), 2048 channels pooled and 512 channels per scale resized -- beside (a) the same operations composed from torch's own
device ops in the same process (four adaptive_avg_pool2d; four interpolate + cat; their autograd backward, the graph built outside the
timed region), (b) the resize halves through the library's generic pfst_resize_bilinear / _bwd, one launch per scale, and (c) the bytes each
launch must move at the measured copy rate.  Variants alternate inside every round; per variant the median, minimum and maximum over the
rounds of the mean of --inner back-to-back runs between two device events.  Then a supervised step (EncoderDecoder.train_step under SGD) of
the comparison models (--models, default all: pspnet, deeplabv3, fcn, upernet, fpn, hrnet) and the flagship at 8 x 1024^2, alternating blocks, host clock
between device synchronisations, with the peak device allocation of each.  One JSON line (and --out FILE).

The feature-pyramid kernels of UPerHead (csrc/fpn.hip) at its grids for that tile -- 512 channels, 256^2 / 128^2 / 64^2 /
32^2 maps -- each beside the composition of library ops it replaces, alternated in the same way: topdown_merge against resize_bilinear into a
temporary + axpy_ + absmax, fpn_resize_concat against one resize_bilinear(out=slice) per level + absmax of the slices,
fpn_resize_concat_bwd against one resize_bilinear_bwd per level; achieved bytes per second from the bytes the shapes say must move.

The Semantic FPN kernels (csrc/fpn.hip) at the grids of that tile -- the neck's nearest merges at 256 channels, the head's
upsample2x_norm and fpn_level_sum at 128 -- each beside the composition of library ops it replaces: upsample_nearest + axpy_ + absmax;
bn_apply + resize_bilinear + absmax; bn_apply x 4 + three resize_bilinear + three axpy_ + absmax; one adjoint resize against three.

  python tools/heads_bench.py [--tiles 8] [--grid 128] [--rounds 7] [--inner 5] [--steps 12] [--models a,b] [--no-step] [--no-ops] [--no-fpn]
                              [--no-sfpn] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
COPY_TB_S = 6.29          # the device-to-device copy rate measured on the MI355X (read + write bytes per second)
SCALES = (1, 2, 3, 6)


def alternate(variants, rounds, inner):
    """variants: {name: fn}.  -> {name: dict(median_ms, min_ms, max_ms)} of the per-round mean over `inner` runs; the order flips every round"""
    import torch
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    names = list(variants)
    for r in range(rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                variants[k]()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in ms.items()}


def verdict(r, ours, others, moved_bytes):
    """ours beats another variant when its slowest round is faster than the other's fastest"""
    r['bytes_MB'] = round(moved_bytes / 1e6, 1)
    r['floor_ms_at_copy_rate'] = round(moved_bytes / (COPY_TB_S * 1e12) * 1e3, 4)
    r['fraction_of_copy_rate'] = round(r['floor_ms_at_copy_rate'] / r[ours]['median_ms'], 3)
    for o in others:
        r[f'{o}_over_{ours}'] = round(r[o]['median_ms'] / r[ours]['median_ms'], 2)
        r[f'beats_{o}_beyond_spread'] = r[ours]['max_ms'] < r[o]['min_ms']
    return r


def ops_bench(args):
    import torch
    import torch.nn.functional as F
    from pfst_amd import hip_ops as ops
    N, G, K = args.tiles, args.grid, len(SCALES)
    CI, CH = 2048, 512
    torch.manual_seed(0)
    cells = sum(s * s for s in SCALES)
    x = torch.randn(N, CI, G, G, device='cuda')
    res = dict(tiles=N, grid=G, scales=list(SCALES), rounds=args.rounds, inner=args.inner)
    plane_in, plane_up = 4 * N * CI * G * G, 4 * N * K * CH * G * G

    # ---- pooling forward: x read once; torch: four passes
    res['pool'] = verdict(alternate(dict(pyramid=lambda: ops.pyramid_pool(x, SCALES),
                                         torch=lambda: [F.adaptive_avg_pool2d(x, s) for s in SCALES]), args.rounds, args.inner),
                          'pyramid', ['torch'], plane_in + 4 * N * CI * cells)
    # ---- pooling backward: dL/dx written once; torch: autograd over the four pools (four passes + three accumulations)
    gs = [torch.randn(N, CI, s, s, device='cuda') for s in SCALES]
    xr = x.detach().requires_grad_(True)
    pooled = [F.adaptive_avg_pool2d(xr, s) for s in SCALES]
    dx = torch.empty_like(x)
    res['pool_bwd'] = verdict(alternate(dict(pyramid=lambda: ops.pyramid_pool_bwd(gs, SCALES, dx),
                                             torch=lambda: torch.autograd.grad(pooled, xr, gs, retain_graph=True)), args.rounds, args.inner),
                              'pyramid', ['torch'], plane_in + 4 * N * CI * cells)
    del pooled, xr, dx, gs
    # ---- resize forward into the concat slices
    grids = [torch.randn(N, CH, s, s, device='cuda').relu_() for s in SCALES]
    cat = torch.empty(N, CI + K * CH, G, G, device='cuda')
    up = cat[:, CI:]
    dense = torch.empty(N, K * CH, G, G, device='cuda')

    def generic_up():
        for k, gk in enumerate(grids):
            ops.resize_bilinear(gk, (G, G), out=up[:, k * CH:(k + 1) * CH])
    res['upsample'] = verdict(alternate(dict(pyramid=lambda: ops.pyramid_upsample(grids, SCALES, up),
                                             torch=lambda: torch.cat([F.interpolate(gk, (G, G), mode='bilinear', align_corners=False) for gk in grids], 1, out=dense),
                                             generic=generic_up), args.rounds, args.inner),
                              'pyramid', ['torch', 'generic'], plane_up + 4 * N * CH * cells)
    # ---- resize backward out of the concat gradient
    dcat = torch.randn(N, CI + K * CH, G, G, device='cuda')
    dy = dcat[:, CI:]
    gr = [gk.detach().requires_grad_(True) for gk in grids]
    ups = torch.cat([F.interpolate(gk, (G, G), mode='bilinear', align_corners=False) for gk in gr], 1)
    dyd = dy.contiguous()

    def generic_up_bwd():
        return [ops.resize_bilinear_bwd(dy[:, k * CH:(k + 1) * CH], (s, s)) for k, s in enumerate(SCALES)]
    res['upsample_bwd'] = verdict(alternate(dict(pyramid=lambda: ops.pyramid_upsample_bwd(dy, SCALES),
                                                 torch=lambda: torch.autograd.grad(ups, gr, dyd, retain_graph=True), generic=generic_up_bwd),
                                            args.rounds, args.inner),
                                  'pyramid', ['torch', 'generic'], plane_up + 4 * N * CH * cells)
    return res


def fpn_bench(args):
    import torch
    from pfst_amd import hip_ops as ops
    N, CH, G0 = args.tiles, 512, args.size // 4
    grids = [G0 >> i for i in range(4)]
    torch.manual_seed(0)
    res = dict(tiles=N, channels=CH, grids=grids, rounds=args.rounds, inner=args.inner)

    def rate(r, ours, others, moved):
        verdict(r, ours, others, moved)
        r['achieved_TB_s'] = round(moved / (r[ours]['median_ms'] * 1e-3) / 1e12, 3)
        for o in others:
            r[f'not_slower_than_{o}_beyond_spread'] = r[ours]['median_ms'] <= r[o]['median_ms'] or r[ours]['min_ms'] <= r[o]['max_ms']
        return r
    # ---- the three merges: lateral + resize(coarser), max |out| published
    for i in (2, 1, 0):
        hf, hc = grids[i], grids[i + 1]
        lat = torch.randn(N, CH, hf, hf, device='cuda')
        coarse = torch.randn(N, CH, hc, hc, device='cuda')
        out, tmp = torch.empty_like(lat), torch.empty_like(lat)
        slots = ops.amax_slots(lat.device, 2)

        def composed():
            ops.resize_bilinear(coarse, (hf, hf), out=tmp)
            ops.axpy_(tmp, lat)
            ops.absmax(tmp, out=slots[:ops.AMAX_SUB])
        res[f'merge_{hc}_to_{hf}'] = rate(alternate(dict(fused=lambda: ops.topdown_merge(lat, coarse, out=out, amax=slots[ops.AMAX_SUB:]),
                                                         composed=composed), args.rounds, args.inner),
                                          'fused', ['composed'], 4 * N * CH * (2 * hf * hf + hc * hc))
        del lat, coarse, out, tmp
    # ---- the three coarser levels into their slices of the concat, and back
    hf = grids[0]
    srcs = [torch.randn(N, CH, g, g, device='cuda').relu_() for g in grids[1:]]
    cat = torch.empty(N, 4 * CH, hf, hf, device='cuda')
    up = cat[:, CH:]
    slots = ops.amax_slots(cat.device, 2)
    moved = 4 * N * CH * (3 * hf * hf + sum(g * g for g in grids[1:]))

    def per_level():
        for k, s in enumerate(srcs):
            ops.resize_bilinear(s, (hf, hf), out=up[:, k * CH:(k + 1) * CH])
        ops.absmax(up, out=slots[:ops.AMAX_SUB])
    res['concat'] = rate(alternate(dict(fused=lambda: ops.fpn_resize_concat(srcs, up, amax=slots[ops.AMAX_SUB:]), per_level=per_level),
                                   args.rounds, args.inner), 'fused', ['per_level'], moved)
    cat.normal_()
    outs = [torch.empty_like(s) for s in srcs]

    def per_level_bwd():
        for k, o in enumerate(outs):
            ops.resize_bilinear_bwd(up[:, k * CH:(k + 1) * CH], tuple(o.shape[2:]), out=o)
    res['concat_bwd'] = rate(alternate(dict(fused=lambda: ops.fpn_resize_concat_bwd(up, outs), per_level=per_level_bwd), args.rounds, args.inner),
                             'fused', ['per_level'], moved)
    return res


def sfpn_bench(args):
    import torch
    from pfst_amd import hip_ops as ops
    N, CN, CH, G0 = args.tiles, 256, 128, args.size // 4
    grids = [G0 >> i for i in range(4)]
    torch.manual_seed(0)
    res = dict(tiles=N, neck_channels=CN, head_channels=CH, grids=grids, rounds=args.rounds, inner=args.inner)

    def rate(r, ours, others, moved):
        verdict(r, ours, others, moved)
        r['achieved_TB_s'] = round(moved / (r[ours]['median_ms'] * 1e-3) / 1e12, 3)
        return r

    def table(c):            # (mean, invstd, sc, sh) rows as bn_apply forms them from (0, 1, gamma, beta)
        gamma, beta = torch.rand(c, device='cuda') + 0.5, torch.randn(c, device='cuda') * 0.2
        return torch.stack([torch.zeros_like(gamma), torch.ones_like(gamma), gamma, beta], 1).contiguous()

    def norm(x, t, out=None):
        return ops.bn_apply(x, t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous(), t[:, 3].contiguous(), True, out=out)
    # ---- the neck's three nearest merges (exact x2 at these grids), max |out| published
    for i in (2, 1, 0):
        hf, hc = grids[i], grids[i + 1]
        lat = torch.randn(N, CN, hf, hf, device='cuda')
        coarse = torch.randn(N, CN, hc, hc, device='cuda')
        out = torch.empty_like(lat)
        slots = ops.amax_slots(lat.device, 2)

        def composed():
            tmp = ops.upsample_nearest(coarse, 2)
            ops.axpy_(tmp, lat)
            ops.absmax(tmp, out=slots[:ops.AMAX_SUB])
        res[f'merge_nearest_{hc}_to_{hf}'] = rate(alternate(dict(fused=lambda: ops.topdown_merge_nearest(lat, coarse, out=out, amax=slots[ops.AMAX_SUB:]),
                                                                 composed=composed), args.rounds, args.inner),
                                                  'fused', ['composed'], 4 * N * CN * (2 * hf * hf + hc * hc))
        dc = torch.empty_like(coarse)
        res[f'nearest_bwd_{hf}_to_{hc}'] = rate(alternate(dict(fused=lambda: ops.nearest_resize_bwd(lat, (hc, hc), out=dc),
                                                               composed=lambda: ops.upsample_nearest_bwd(lat, 2)), args.rounds, args.inner),
                                                'fused', ['composed'], 4 * N * CN * (hf * hf + hc * hc))
        del lat, coarse, out, dc
    # ---- conv -> BN -> ReLU -> x2 of the head's deeper levels: the pre-BN tensor normalised on load
    for hc in (grids[3], grids[2]):
        pre, t = torch.randn(N, CH, hc, hc, device='cuda'), table(CH)
        out, tmp = torch.empty(N, CH, 2 * hc, 2 * hc, device='cuda'), torch.empty(N, CH, hc, hc, device='cuda')
        slots = ops.amax_slots(pre.device, 2)

        def composed():
            norm(pre, t, out=tmp)
            ops.resize_bilinear(tmp, (2 * hc, 2 * hc), out=out)
            ops.absmax(out, out=slots[:ops.AMAX_SUB])
        res[f'upsample2x_norm_{hc}'] = rate(alternate(dict(fused=lambda: ops.upsample2x_norm(pre, t, out=out, amax=slots[ops.AMAX_SUB:]),
                                                           composed=composed), args.rounds, args.inner),
                                            'fused', ['composed'], 4 * N * CH * 5 * hc * hc)
        del pre, out, tmp
    # ---- the level sum: level 0's last map and three maps on half of its grid
    h0, hh = grids[0], grids[1]
    pre0, members = torch.randn(N, CH, h0, h0, device='cuda'), [torch.randn(N, CH, hh, hh, device='cuda') for _ in range(3)]
    tabs = [table(CH) for _ in range(4)]
    out, acc, full, half = torch.empty_like(pre0), torch.empty_like(pre0), torch.empty_like(pre0), torch.empty_like(members[0])
    slots = ops.amax_slots(pre0.device, 2)

    def composed_sum():
        norm(pre0, tabs[0], out=acc)
        for m, t in zip(members, tabs[1:]):
            norm(m, t, out=half)
            ops.resize_bilinear(half, (h0, h0), out=full)
            ops.axpy_(acc, full)
        ops.absmax(acc, out=slots[:ops.AMAX_SUB])
    res['level_sum'] = rate(alternate(dict(fused=lambda: ops.fpn_level_sum(pre0, tabs[0], members, tabs[1:], out=out, amax=slots[ops.AMAX_SUB:]),
                                           composed=composed_sum), args.rounds, args.inner),
                            'fused', ['composed'], 4 * N * CH * (2 * h0 * h0 + 3 * hh * hh))
    # ---- its backward: one adjoint resize serves the three half-grid members
    g = torch.randn(N, CH, h0, h0, device='cuda')
    ds = [torch.empty_like(m) for m in members]
    res['level_sum_bwd'] = rate(alternate(dict(fused=lambda: ops.resize_bilinear_bwd(g, (hh, hh), out=ds[0]),
                                               composed=lambda: [ops.resize_bilinear_bwd(g, (hh, hh), out=d) for d in ds]), args.rounds, args.inner),
                                'fused', ['composed'], 4 * N * CH * (h0 * h0 + hh * hh))
    return res


def step_bench(args):
    import torch
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import SGD_OPTIMIZER, baseline_model_cfg, model_cfg
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import synth_batch
    batch = synth_batch(args.tiles, args.size, 6, 3, seed=1234, device='cuda')
    batch = {k: v for k, v in batch.items() if not k.startswith('target_')}
    cfgs = dict(deeplabv3plus=model_cfg(6, 3), pspnet=baseline_model_cfg('pspnet', 6, 3), deeplabv3=baseline_model_cfg('deeplabv3', 6, 3),
                fcn=baseline_model_cfg('fcn', 6, 3), upernet=baseline_model_cfg('upernet', 6, 3), fpn=baseline_model_cfg('fpn', 6, 3),
                hrnet=baseline_model_cfg('hrnet', 6, 3))
    if args.models:
        cfgs = {k: cfgs[k] for k in args.models.split(',')}
    times = {k: [] for k in cfgs}
    peak = {k: 0 for k in cfgs}
    blocks, per_block = 3, -(-args.steps // 3)
    # one model resident at a time (activations of an 8 x 1024^2 step are tens of GB): blocks of one kind run back to back, kinds in turn
    for blk in range(blocks):
        for kind in (list(cfgs) if blk % 2 == 0 else list(cfgs)[::-1]):
            torch.manual_seed(0)
            model = build_segmentor(cfgs[kind])
            model.init_weights()
            model.cuda()
            opt = build_optimizer(model, dict(SGD_OPTIMIZER, lr=6e-5))
            torch.cuda.reset_peak_memory_stats()
            for _ in range(2):
                model.train_step(batch, opt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_block):
                model.train_step(batch, opt)
            torch.cuda.synchronize()
            times[kind].append(1000.0 * (time.perf_counter() - t0) / per_block)
            peak[kind] = max(peak[kind], torch.cuda.max_memory_allocated())
            del model, opt
    out = dict(tiles=args.tiles, size=args.size, steps_per_block=per_block, blocks=blocks)
    for kind, v in times.items():
        out[kind] = dict(median_ms_per_step=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2),
                         peak_allocated_GB=round(peak[kind] / 1e9, 2))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--tiles', type=int, default=8)
    p.add_argument('--grid', type=int, default=128)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--rounds', type=int, default=7)
    p.add_argument('--inner', type=int, default=5)
    p.add_argument('--steps', type=int, default=12, help='timed supervised steps per model')
    p.add_argument('--models', default=None, help='comma-separated kinds of the supervised-step part (deeplabv3plus,pspnet,deeplabv3,fcn,upernet,fpn,hrnet); default all')
    p.add_argument('--no-step', action='store_true')
    p.add_argument('--no-fpn', action='store_true')
    p.add_argument('--no-ops', action='store_true')
    p.add_argument('--no-sfpn', action='store_true')
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    import torch
    import pfst_amd  # noqa: F401
    res = dict(device=torch.cuda.get_device_name(0))
    if not args.no_ops:
        res['ops'] = ops_bench(args)
        torch.cuda.empty_cache()
    if not args.no_fpn:
        res['fpn'] = fpn_bench(args)
        torch.cuda.empty_cache()
    if not args.no_sfpn:
        res['semantic_fpn'] = sfpn_bench(args)
        torch.cuda.empty_cache()
    if not args.no_step:
        res['supervised_step'] = step_bench(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


if __name__ == '__main__':
    main()
