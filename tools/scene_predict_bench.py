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
holds the per-kernel times of (c)."""
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
    args = ap.parse_args(argv)
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


if __name__ == '__main__':
    main()
