#!/usr/bin/env python3
"""Times OHEMPixelSampler's launches (csrc/ohem.hip) at the flagship workload's shape -- 8 tiles, 6 classes, the decode head's
256^2 logits and the auxiliary head's 128^2 to 1024^2 labels -- in both modes and for both outcomes of the threshold mode's early-out, beside
the reference's own method on the same device in the same process: materialise the up-sampled logits with torch, softmax, gather, `sort`
(threshold mode) / unreduced cross-entropy and a descending `sort` (top-k mode).  Device events, the median of --repeat timed runs after
--warmup untimed ones.  Then a supervised step (EncoderDecoder.train_step under SGD) with and without samplers on both heads, alternating
blocks, host clock between device synchronisations.  One JSON line (and --out FILE).

  python tools/ohem_bench.py [--tiles 8] [--classes 6] [--size 1024] [--repeat 20] [--warmup 3] [--steps 12] [--no-step] [--out FILE]

Bytes the sampler moves per call, from the shapes: the key map (4 N H W bytes) is written once, read by each of the three histogram levels
and read and rewritten by the weight pass -- five passes and one (33.5 MB each at 8 x 1024^2), plus the labels once; an early-out skips the three
level reads; a partial tie fill in top-k mode reads the map once more."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


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


def torch_sampler(logits, label, thresh, batch_kept, ignore_index=255):
    """ohem_pixel_sampler.py:42-85 behind decode_head.py:253-257, statement for statement, on the device"""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        seg_logit = F.interpolate(logits, size=label.shape[-2:], mode='bilinear', align_corners=False)
        seg_label = label.long()
        valid_mask = seg_label != ignore_index
        seg_weight = seg_logit.new_zeros(size=seg_label.size())
        valid_seg_weight = seg_weight[valid_mask]
        if thresh is not None:
            seg_prob = F.softmax(seg_logit, dim=1)
            tmp = seg_label.clone().unsqueeze(1)
            tmp[tmp == ignore_index] = 0
            seg_prob = seg_prob.gather(1, tmp).squeeze(1)
            sort_prob, _ = seg_prob[valid_mask].sort()
            min_threshold = sort_prob[min(batch_kept, sort_prob.numel() - 1)] if sort_prob.numel() > 0 else 0.0      # .numel(): no device read
            threshold = torch.clamp(torch.as_tensor(min_threshold, device=logits.device), min=thresh)              # max() without the host read
            valid_seg_weight[seg_prob[valid_mask] < threshold] = 1.
        else:
            losses = F.cross_entropy(seg_logit, seg_label, ignore_index=ignore_index, reduction='none')
            _, sort_indices = losses[valid_mask].sort(descending=True)
            valid_seg_weight[sort_indices[:batch_kept]] = 1.
        seg_weight[valid_mask] = valid_seg_weight
        return seg_weight


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--tiles', type=int, default=8)
    p.add_argument('--classes', type=int, default=6)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--repeat', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--steps', type=int, default=12, help='timed supervised steps per kind')
    p.add_argument('--no-step', action='store_true')
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd import hip_ops as ops
    N, C, S = args.tiles, args.classes, args.size
    g = torch.Generator().manual_seed(0)
    label = torch.randint(0, C, (N, S // 16, S // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    label[:, : S // 8, : S // 4] = 255
    label = label.to(torch.uint8).cuda()
    coef = torch.ones(C, device='cuda')
    min_kept = 100000
    res = dict(tiles=N, classes=C, size=S, pixels=N * S * S, min_kept=min_kept, repeat=args.repeat, device=torch.cuda.get_device_name(0),
               map_MB=round(4 * N * S * S / 1e6, 1))
    for head, low in (('decode', S // 4), ('aux', S // 8)):
        logits = (torch.randn(N, C, low, low, generator=g) * 3).cuda()
        # thresh = 0.7 on random labels: far more than k + 1 probabilities lie below it -- the early-out; thresh = 1e-4: s[k] wins, three levels run
        cases = dict(thresh_early_out=0.7, thresh_full_select=1e-4, topk=None)
        for name, thresh in cases.items():
            w, info = ops.ohem_sample(logits, label, 255, thresh, min_kept * N, coef)
            ref = torch_sampler(logits, label, thresh, min_kept * N)
            torch.cuda.synchronize()
            i = info.cpu()
            r = dict(n_valid=int(i[1]), n_kept=int(i[2]), k=int(i[3]), cut=float(i[0:1].to(torch.int32).view(torch.float32)),
                     torch_n_kept=int(ref.sum()), differ_from_torch=int((ref != w).sum()))
            if thresh is not None:
                r['early_out'] = r['cut'] == float(torch.tensor(thresh, dtype=torch.float32))
            r['sampler'] = timed(lambda: ops.ohem_sample(logits, label, 255, thresh, min_kept * N, coef), args.repeat, args.warmup)
            r['torch'] = timed(lambda: torch_sampler(logits, label, thresh, min_kept * N), args.repeat, args.warmup)
            r['torch_over_sampler'] = round(r['torch']['median_ms'] / r['sampler']['median_ms'], 2)
            passes = 3 if r.get('early_out') else 6
            r['map_passes'] = passes
            r['map_TB_per_s'] = round(passes * 4 * N * S * S / (r['sampler']['median_ms'] * 1e-3) / 1e12, 3)
            res[f'{head}_{name}'] = r
    if not args.no_step:
        res['supervised_step'] = step_bench(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


def step_bench(args):
    """the supervised step at the workload's size without samplers, with threshold-mode samplers and with top-k samplers on both heads:
    blocks of steps alternate, a block starts and ends with a device synchronise"""
    import copy
    import torch
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import SGD_OPTIMIZER, workload_cfg
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    cfg, w = workload_cfg(NAME)
    batch = synth_batch(args.tiles, args.size, w['num_classes'], w['in_channels'], seed=1234, device='cuda')
    batch = {k: v for k, v in batch.items() if not k.startswith('target_')}
    kinds = {}
    for kind, sampler in (('plain', None), ('ohem_thresh', dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100000)),
                          ('ohem_topk', dict(type='OHEMPixelSampler', min_kept=100000))):
        mc = copy.deepcopy(cfg['model'])
        if sampler is not None:
            mc['decode_head']['sampler'] = dict(sampler)
            mc['auxiliary_head']['sampler'] = dict(sampler)
        torch.manual_seed(0)
        model = build_segmentor(mc)
        fill_state_dict(model.state_dict(), 0)
        model.cuda()
        kinds[kind] = (model, build_optimizer(model, dict(SGD_OPTIMIZER, lr=6e-5)))
    times = {k: [] for k in kinds}

    def run(kind, n, keep):
        model, opt = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            model.train_step(batch, opt)
        torch.cuda.synchronize()
        if keep:
            times[kind].append(1000.0 * (time.perf_counter() - t0) / n)

    for kind in kinds:
        run(kind, 2, False)
    blocks, per_block = 3, -(-args.steps // 3)
    for blk in range(blocks):
        for kind in (list(kinds) if blk % 2 == 0 else list(kinds)[::-1]):
            run(kind, per_block, True)
    out = dict(steps_per_block=per_block, blocks=blocks)
    for kind, v in times.items():
        out[kind] = dict(median_ms_per_step=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
    for kind in ('ohem_thresh', 'ohem_topk'):
        out[kind + '_minus_plain_ms'] = round(out[kind]['median_ms_per_step'] - out['plain']['median_ms_per_step'], 2)
    return out


if __name__ == '__main__':
    main()
