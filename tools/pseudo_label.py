#!/usr/bin/env python3
"""Offline pseudo-labels of a target split with class-wise entropy thresholds: what the reference's PseudoLabelingHookV4
(rsiseg/core/hook/pseudo_labeling_hookv4.py) and LoadAnnotationsPseudoLabelsV2 (rsiseg/datasets/pipelines/loading.py:392-520) compute
together, written as ordinary label maps.

  python tools/pseudo_label.py CONFIG CHECKPOINT --out-dir DIR [--split test|val] [--ratio R [R ...]] [--label-ratio R] [--teacher]
      [--revise-checkpoint-key] [--reduce-zero-label] [--entropy] [--max-images N] [--gpu-id 0] [--cfg-options ...]

Phase 1 runs the model over every tile of the split and keeps the low-resolution logits on the device.  Phase 2 finds, for every predicted
class and every --ratio r, the entropy below which the share r of that class's pixels lies (`thre@r`, over all pixels of all tiles, exact).
Phase 3 writes `<out-dir>/<stem>.png` per tile: the predicted class where the pixel's entropy lies below the class's `thre@<label-ratio>`,
255 elsewhere -- a mode-P PNG with the dataset's palette that `TileFolder(ann_dir=...)` reads, e.g. for a second self-training stage with
`tools/train.py --supervised`.  --label-ratio (default 0.5, the reference's pseudo_ratio) must be one of --ratio (default: the hook's
0.01 0.05 0.1 0.2 0.3 0.4 0.5).  --reduce-zero-label writes the files in annotation space (class + 1, 0 for ignored), which a dataset with
reduce_zero_label=True reads back as class / 255.  --entropy adds `<stem>_entropy.png`, 8-bit grey, 255 x entropy / ln(classes).
--teacher labels with the EMA teacher of a PFGST checkpoint (its `ema_model.*` keys) instead of the student.
`pseudo_labels.json` holds every `thre@r` table, the pixels predicted per class, the per-class predicted / kept counts of the written
maps, the settings and the seconds per phase.

`--synthetic N` needs neither a checkpoint nor data (nor a config: the Potsdam -> Vaihingen one is built in): a seeded random model on N seeded
synthetic tiles of --synthetic-size pixels."""
import argparse
import json
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):          # the tools folder (predict.py's PNG writer) and the package
    if _p not in sys.path:
        sys.path.insert(0, _p)

SYNTHETIC_WORKLOAD = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='pfst_amd: offline pseudo-labels with class-wise entropy thresholds')
    p.add_argument('config', nargs='?')
    p.add_argument('checkpoint', nargs='?')
    p.add_argument('--out-dir', required=True)
    p.add_argument('--split', default='test', choices=['test', 'val'])
    p.add_argument('--ratio', type=float, nargs='+', default=None, help='the shares r of the thre@r tables, each in [0, 1)')
    p.add_argument('--label-ratio', type=float, default=None, help='the table the label maps are cut with; one of --ratio')
    p.add_argument('--teacher', action='store_true', help="label with a PFGST checkpoint's EMA teacher")
    p.add_argument('--revise-checkpoint-key', action='store_true')
    p.add_argument('--reduce-zero-label', action='store_true', help='write class + 1 and 0 (annotation space) instead of class and 255')
    p.add_argument('--entropy', action='store_true', help='also write <stem>_entropy.png')
    p.add_argument('--max-images', type=int, default=None)
    p.add_argument('--synthetic', type=int, default=None, metavar='N', help='a seeded random model on N seeded synthetic tiles')
    p.add_argument('--synthetic-size', type=int, default=128)
    p.add_argument('--gpu-id', type=int, default=0)
    p.add_argument('--cfg-options', nargs='+')
    args = p.parse_args(argv)
    if args.synthetic is None and (args.config is None or args.checkpoint is None):
        p.error('CONFIG and CHECKPOINT are required without --synthetic')
    if args.synthetic is not None and args.synthetic < 1:
        p.error('--synthetic needs at least one tile')
    if args.max_images is not None and args.max_images < 1:
        p.error('--max-images must be at least 1')
    from pfst_amd.pseudo_labels import DEFAULT_LABEL_RATIO, DEFAULT_RATIOS, check_ratios
    if args.ratio is None:
        args.ratio = list(DEFAULT_RATIOS)
    if args.label_ratio is None:
        args.label_ratio = DEFAULT_LABEL_RATIO
    try:
        args.ratio = check_ratios(args.ratio, args.label_ratio)
    except ValueError as e:
        p.error(str(e))
    return args


def load_config(args):
    """the config file with --cfg-options merged; without a file (--synthetic) the built-in Potsdam -> Vaihingen workload"""
    from pfst_amd.config import Config, parse_cfg_options
    if args.config is not None:
        cfg = Config.fromfile(args.config)
    else:
        from pfst_amd.presets import workload_cfg
        uda, _ = workload_cfg(SYNTHETIC_WORKLOAD)
        cfg = Config(dict(model=uda.pop('model'), uda=uda))
    if args.cfg_options:
        cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    return cfg


def build_model_and_data(args, cfg, dev):
    from pfst_amd.apis import init_segmentor
    if args.synthetic is not None:
        import torch
        from pfst_amd.statistics import SyntheticTiles
        from pfst_amd.synthetic import fill_state_dict
        torch.manual_seed(0)
        model = init_segmentor(cfg, None, device='cpu')
        fill_state_dict(model.state_dict(), 0)
        model.to(dev)
        data = SyntheticTiles(args.synthetic, args.synthetic_size, cfg.model.decode_head.num_classes, cfg.model.backbone.get('in_channels', 3))
        return model, data
    from pfst_amd.data import TileFolder
    try:
        model = init_segmentor(cfg, args.checkpoint, device=dev, revise_checkpoint_key=args.revise_checkpoint_key, teacher=args.teacher)
    except RuntimeError as e:
        if 'keys are missing' in str(e):
            raise SystemExit(str(e))
        raise
    return model, TileFolder(cfg.data[args.split], test_mode=True)


def entropy_png(ent, num_classes):
    """entropy float [H, W] on the device -> uint8 [H, W] (NumPy): 255 x entropy / ln(classes), rounded"""
    import torch
    top = math.log(max(num_classes, 2))
    return torch.clamp(ent * (255.0 / top) + 0.5, 0, 255).to(torch.uint8).cpu().numpy()


def main(argv=None):
    args = parse_args(argv)
    import torch
    from PIL import Image
    import pfst_amd  # noqa: F401
    from pfst_amd import hip_ops as ops
    from pfst_amd.pseudo_labels import ClassEntropyThresholds, collect, label_maps
    from predict import write_label_png
    cfg = load_config(args)
    torch.cuda.set_device(args.gpu_id)
    dev = torch.device('cuda', args.gpu_id)
    model, data = build_model_and_data(args, cfg, dev)
    C = cfg.model.decode_head.num_classes
    acc = ClassEntropyThresholds(C, dev)
    seconds = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        stems = collect(model, data, acc, max_images=args.max_images)
    except MemoryError as e:
        raise SystemExit(str(e))
    torch.cuda.synchronize()
    seconds['forward'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    table, n_c = acc.thresholds(args.ratio)                                     # the reads end the queued work
    seconds['thresholds'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    os.makedirs(args.out_dir, exist_ok=True)
    thr = table[args.ratio.index(float(args.label_ratio))]
    thr_d = torch.from_numpy(thr).to(dev)
    counts = torch.zeros(C, 2, dtype=torch.int64, device=dev)
    palette = getattr(model, 'PALETTE', None) or getattr(data, 'PALETTE', [])
    for block, size, tags in acc.blocks():
        labels, _ = label_maps(block, size, thr_d, args.reduce_zero_label, counts)
        labels = labels.cpu().numpy()
        ent = ops.entropy_upsample(block, size, 1, want_pred=False)[0] if args.entropy else None
        for j, stem in enumerate(tags):
            # annotation space: value v shows class v - 1's colour, 0 (ignored) black
            pal = ([[0, 0, 0]] + list(palette)) if args.reduce_zero_label else palette
            write_label_png(os.path.join(args.out_dir, f'{stem}.png'), labels[j], pal)
            if ent is not None:
                Image.fromarray(entropy_png(ent[j], C)).save(os.path.join(args.out_dir, f'{stem}_entropy.png'))
    counts = counts.cpu().tolist()
    seconds['labels'] = time.perf_counter() - t0
    out = dict(config=args.config, checkpoint=args.checkpoint, split=None if args.synthetic is not None else args.split,
               synthetic=args.synthetic, teacher=args.teacher, reduce_zero_label=args.reduce_zero_label, images=len(stems), stems=stems,
               num_classes=C, ratios=args.ratio, label_ratio=args.label_ratio, radix_levels=[list(l) for l in acc.levels],
               histogram_passes=acc.passes, thresholds={f'thre@{r}': [float(v) for v in row] for r, row in zip(args.ratio, table)},
               n_c=[int(v) for v in n_c], predicted=[int(c[0]) for c in counts], kept=[int(c[1]) for c in counts],
               seconds={k: round(v, 4) for k, v in seconds.items()})
    path = os.path.join(args.out_dir, 'pseudo_labels.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=1)
    kept, total = sum(out['kept']), sum(out['predicted'])
    print(f"{len(stems)} tiles, kept {kept} of {total} pixels ({100.0 * kept / max(total, 1):.1f} %) at thre@{args.label_ratio}; "
          + ', '.join(f'{k} {v:.2f} s' for k, v in seconds.items()) + f' -> {path}')
    return out


if __name__ == '__main__':
    main()
