#!/usr/bin/env python3
"""Whole-scene prediction against the slide path it is built beside, in ONE process on one box: a synthetic random 6000 x 6000 uint8 scene
(Potsdam's size), a randomly initialised DeepLabV3+ R50-D8, window 1024 / stride 512 (121 windows), the default arithmetic.  Blocks of scenes
alternate between

  (a) slide      the existing path: pipeline.normalize of the scene on the host, upload of the fp32 image, EncoderDecoder.inference in
                 slide mode (one window per forward; resize, window_accumulate_, window_normalize_, softmax, arg-max as kernels of their own)
  (b) scene_b1   predict_scene, one window per batch: upload of the uint8 scene, scene_windows / forward / scene_accumulate_, scene_finalize
  (c) scene_bN   predict_scene, --windows-per-batch windows per batch (default 8)

Every scene is timed by the host clock from the host array to the labels on the host (a device synchronise is implied by that read); per
kind the median over all scenes, per block the median of its scenes, the spread of a kind = max - min of its block medians.  Printed as one
JSON line; `labels` compares the outputs: (b) must equal (a) bit for bit, (c) differs where the f16x3 scales over the batch move a tie.

    python tools/scene_predict_bench.py [--size 6000] [--window 1024] [--stride 512] [--windows-per-batch 8] [--scenes 2] [--blocks 3]

Under `rocprofv3 --kernel-trace --stats -- python tools/scene_predict_bench.py --only scene_bN --scenes 1 --blocks 1 --warmup 0` the trace
holds the per-kernel times of (c).

    python tools/scene_predict_bench.py --tta [--size 6000] [--classes 6] [--ratios 0.5 0.75 1.0 1.25 1.5 1.75] [--scenes 2] [--blocks 3]

The view step of test-time augmentation on scenes (predict_scene_tta) instead, without a model: for every ratio random window sums of the
view's size are folded into the scene-sized sum of probabilities, plain and mirrored, by

  (d) tta_fused  scene_tta_accumulate_: one pass
  (e) tta_chain  the kernels it replaces: a count plane, window_normalize_, resize_bilinear, softmax_nchw, flip_planes, axpy_

timed with device events per call, the two alternating in blocks as above (--scenes calls per block); `equal` compares the sums they leave."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--size', type=int, default=6000)
    ap.add_argument('--window', type=int, default=1024)
    ap.add_argument('--stride', type=int, default=512)
    ap.add_argument('--windows-per-batch', type=int, default=8)
    ap.add_argument('--scenes', type=int, default=2, help='scenes per block')
    ap.add_argument('--blocks', type=int, default=3, help='blocks per kind')
    ap.add_argument('--warmup', type=int, default=1, help='untimed scenes per kind')
    ap.add_argument('--only', default=None, help='run one kind only (slide / scene_b1 / scene_bN): for a kernel trace')
    ap.add_argument('--tta', action='store_true', help='time the view step of predict_scene_tta, fused against the chain of existing kernels')
    ap.add_argument('--classes', type=int, default=6, help='--tta: classes of the sums')
    ap.add_argument('--ratios', type=float, nargs='+', default=None, help='--tta: view ratios (default: the six of --aug-test)')
    args = ap.parse_args(argv)
    if args.tta:
        return tta_main(args)
    import numpy as np
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd import pipeline
    from pfst_amd.presets import model_cfg
    from pfst_amd.registry import build_segmentor
    from pfst_amd.scene import memory_needed, predict_scene, window_grid
    from pfst_amd.synthetic import fill_state_dict
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    crop, stride = (args.window,) * 2, (args.stride,) * 2
    cfg = model_cfg()
    cfg['test_cfg'] = dict(mode='slide', crop_size=crop, stride=stride)
    cfg['train_cfg'] = None
    torch.manual_seed(0)
    seg = build_segmentor(cfg)
    fill_state_dict(seg.state_dict(), 0)
    seg.cuda()
    scene = np.random.RandomState(0).randint(0, 256, (args.size, args.size, 3)).astype(np.uint8)
    wins, size = window_grid(args.size, args.size, crop, stride)

    def slide():
        img = torch.from_numpy(pipeline.normalize(scene, **NORM).transpose(2, 0, 1))[None].cuda().contiguous()
        lab, _ = seg.inference(img, None, False)
        return lab[0].cpu().numpy()

    def scene_run(per):
        def run():
            lab, _, _ = predict_scene(seg, torch.from_numpy(scene).cuda(), NORM, crop, stride, windows_per_batch=per)
            return lab.cpu().numpy()
        return run

    kinds = dict(slide=slide, scene_b1=scene_run(1), scene_bN=scene_run(args.windows_per_batch))
    if args.only:
        kinds = {args.only: kinds[args.only]}
    times = {k: [] for k in kinds}            # per kind: one list of scene times per block
    labels, peak = {}, {}
    with torch.no_grad():
        for kind, fn in kinds.items():
            for _ in range(args.warmup):
                fn()
        for blk in range(args.blocks):
            for kind in (list(kinds) if blk % 2 == 0 else list(kinds)[::-1]):          # alternate, rotating the order
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                block = []
                for _ in range(args.scenes):
                    t0 = time.perf_counter()
                    labels[kind] = kinds[kind]()
                    block.append(time.perf_counter() - t0)
                times[kind].append(block)
                peak[kind] = torch.cuda.max_memory_allocated()
    res = dict(size=args.size, window=list(size), stride=args.stride, windows=len(wins), windows_per_batch=args.windows_per_batch,
               scenes_per_block=args.scenes, blocks=args.blocks)
    for kind, blocks in times.items():
        meds = [statistics.median(b) for b in blocks]
        res[kind] = dict(median_s=round(statistics.median([t for b in blocks for t in b]), 4), block_medians_s=[round(m, 4) for m in meds],
                         spread_s=round(max(meds) - min(meds), 4), peak_MiB=round(peak[kind] / 2**20))
    if 'slide' in labels:
        res['labels'] = {k: dict(equal=bool(np.array_equal(v, labels['slide'])), differing_share=float((v != labels['slide']).mean()))
                         for k, v in labels.items() if k != 'slide'}
    fixed, act = memory_needed(seg.num_classes, args.size, args.size, size, args.windows_per_batch)
    res['memory_estimate_MiB'] = dict(sums_and_labels=round(fixed / 2**20), activations=round(act / 2**20))
    print(json.dumps(res))
    return res


def tta_main(args):
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd import hip_ops as ops
    from pfst_amd.evaluation import AUG_TEST_RATIOS
    from pfst_amd.scene import _count_tables, _view_add_chain, tta_views
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    H = W = args.size
    C = args.classes
    crop, stride = (args.window,) * 2, (args.stride,) * 2
    ratios = [float(r) for r in (args.ratios or AUG_TEST_RATIOS)]
    dev = torch.device('cuda')
    acc = torch.rand(C, H, W, device=dev)
    res = dict(tta=True, size=args.size, classes=C, window=args.window, stride=args.stride, calls_per_block=args.scenes, blocks=args.blocks,
               views=[])
    total = dict(tta_fused=0.0, tta_chain=0.0)
    for v in tta_views(H, W, ratios, True):
        hr, wr = v['size']
        rows_d, cols_d = _count_tables(hr, wr, crop, stride, dev)
        master = 3 * torch.randn(C, hr, wr, device=dev) * (rows_d[:, None] * cols_d[None, :])
        sums = master.clone()
        hflip = v['flip']

        def fused():
            ops.scene_tta_accumulate_(acc, sums, rows_d, cols_d, hflip, False, accumulate=True)

        def chain():
            _view_add_chain(acc, sums, rows_d, cols_d, (H, W), hflip, False)

        kinds = dict(tta_fused=fused, tta_chain=chain)
        left = {}
        for kind, fn in kinds.items():                                  # the sums each leaves from the same start, and the warm-up
            start = acc.clone()
            fn()
            left[kind], acc = acc, start
            sums.copy_(master)                                         # the chain normalises the view sums in place
        equal = bool(torch.equal(left['tta_fused'], left['tta_chain']))
        del left
        times = {k: [] for k in kinds}
        for blk in range(args.blocks):
            for kind in (list(kinds) if blk % 2 == 0 else list(kinds)[::-1]):
                block = []
                for _ in range(args.scenes):
                    sums.copy_(master)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    kinds[kind]()
                    t1.record()
                    t1.synchronize()
                    block.append(t0.elapsed_time(t1))
                times[kind].append(statistics.median(block))
        rec = dict(ratio=v['ratio'], flip=v['flip'], view=[hr, wr], equal=equal)
        for kind, meds in times.items():
            rec[kind] = dict(median_ms=round(statistics.median(meds), 3), spread_ms=round(max(meds) - min(meds), 3))
            total[kind] += statistics.median(meds)
        res['views'].append(rec)
        del master, sums
    res['sum_of_medians_ms'] = {k: round(t, 3) for k, t in total.items()}
    res['acc_traffic_GB_per_view'] = round(2 * 4 * C * H * W / 1e9, 3)        # the read-modify-write of the scene-sized sum, the floor of either
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
