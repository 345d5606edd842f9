#!/usr/bin/env python3
"""Predict whole images -- complete ISPRS scenes at their native resolution, not pre-cut tiles -- and write label maps and pictures: the
surface of the reference's `tools/test.py --show-dir DIR --opacity X` and `rsiseg.apis.inference_segmentor`.

  python tools/predict.py CONFIG CHECKPOINT IMAGE_OR_DIR [...] --out-dir DIR [--opacity 0.5] [--confidence] [--window N] [--stride N]
      [--windows-per-batch 8] [--aug-test] [--ratios R [R ...]] [--no-flip] [--ann-dir DIR [--reduce-zero-label]] [--revise-checkpoint-key]
      [--gpu-id 0] [--cfg-options ...]

Per input `<stem>`: `<stem>.png`, a mode-P PNG whose pixel values are the class indices and whose palette is the dataset's (one file is the
machine-readable result and a colour picture); with --opacity `<stem>_overlay.png`, the colours blended over the image as show_result
blends them; with --confidence `<stem>_conf.png`, 8-bit grey, 255 x the probability of the predicted class.  `predict.json` lists size,
windows, batches and seconds per image.  The scene is covered with sliding windows forwarded --windows-per-batch at a time; --window /
--stride default to the config's test_cfg.crop_size / stride when it is a `slide` config, to 1024 / 512 otherwise.

--aug-test predicts with the reference's test-time augmentation (`tools/test.py --aug-test`): the scene at 0.5, 0.75, 1.0, 1.25, 1.5 and 1.75
times its size, each plain and mirrored, the class probabilities of the twelve views averaged at the scene's size.  --ratios sets the ratios
(with the mirrored views, unless --no-flip); one ratio with --no-flip predicts the scene at another resolution.  `predict.json` then lists
the ratios, `flip` and the views per image.  --ann-dir DIR scores every image that has a label map `DIR/<stem>.png` (class indices;
--reduce-zero-label as LoadAnnotations applies it) and adds aAcc / mIoU / mAcc / IoU per image and overall to `predict.json`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE_SUFFIXES = ('.png', '.tif', '.tiff', '.jpg', '.jpeg', '.bmp')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='pfst_amd: predict whole images with batched sliding windows')
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('inputs', nargs='+', help='image files and / or folders of images')
    p.add_argument('--out-dir', required=True)
    p.add_argument('--opacity', type=float, default=None, help='also write <stem>_overlay.png with this opacity of the colours, in [0, 1]')
    p.add_argument('--confidence', action='store_true', help='also write <stem>_conf.png')
    p.add_argument('--window', type=int, default=None)
    p.add_argument('--stride', type=int, default=None)
    p.add_argument('--windows-per-batch', type=int, default=8)
    p.add_argument('--aug-test', action='store_true', help='multi-scale + flip test-time augmentation with the ratios of the reference')
    p.add_argument('--ratios', type=float, nargs='+', default=None, help='ratios of the scene size to predict at (with mirrored views)')
    p.add_argument('--no-flip', action='store_true', help='no mirrored views with --aug-test / --ratios')
    p.add_argument('--ann-dir', default=None, help='folder of label maps <stem>.png to score the predictions against')
    p.add_argument('--reduce-zero-label', action='store_true', help='label 0 of the --ann-dir maps is ignored and the others shift down by one')
    p.add_argument('--revise-checkpoint-key', action='store_true')
    p.add_argument('--gpu-id', type=int, default=0)
    p.add_argument('--cfg-options', nargs='+')
    args = p.parse_args(argv)
    if args.opacity is not None and not 0.0 <= args.opacity <= 1.0:
        p.error('--opacity must lie in [0, 1]')
    if not 1 <= args.windows_per_batch <= 16:
        p.error('--windows-per-batch must lie in 1 .. 16')
    if args.ratios is not None and min(args.ratios) <= 0:
        p.error('--ratios must be positive')
    if args.reduce_zero_label and args.ann_dir is None:
        p.error('--reduce-zero-label needs --ann-dir')
    return args


def tta_options(args):
    """(ratios, flip) for predict_image: --ratios, else with --aug-test the six ratios of the reference's tools/test.py, else None (no
    augmentation); the mirrored views go with either unless --no-flip"""
    ratios = args.ratios
    if ratios is None and args.aug_test:
        from pfst_amd.evaluation import AUG_TEST_RATIOS
        ratios = list(AUG_TEST_RATIOS)
    return ratios, ratios is not None and not args.no_flip


def read_annotation(ann_dir, stem, reduce_zero_label=False):
    """the label map `<ann_dir>/<stem>.png` as uint8 class indices (LoadAnnotations with the pillow backend), or None when there is none"""
    path = os.path.join(ann_dir, stem + '.png')
    if not os.path.exists(path):
        return None
    from pfst_amd.data import _read_label
    from pfst_amd.pipeline import reduce_zero_label as reduce
    seg = _read_label(path)
    if seg.ndim != 2:
        raise SystemExit(f'{path}: a label map holds one class index per pixel, got shape {seg.shape}')
    return reduce(seg) if reduce_zero_label else seg


def metrics_record(areas):
    """(inter, union, pred, label) areas -> dict(aAcc, mIoU, mAcc, IoU) in percent as CustomDataset.evaluate reports them; classes absent
    from prediction and annotation (nan) are left out of the means and listed as null"""
    import numpy as np
    from pfst_amd.evaluation import total_area_to_metrics
    import warnings
    pct = lambda v: None if np.isnan(v) else round(100 * float(v), 4)
    with warnings.catch_warnings(), np.errstate(invalid='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)               # an annotation without a single labelled pixel: every mean is nan
        m = total_area_to_metrics(*areas)
        return dict(aAcc=pct(m['aAcc']), mIoU=pct(np.nanmean(m['IoU'])), mAcc=pct(np.nanmean(m['Acc'])), IoU=[pct(v) for v in m['IoU']])


def load_config(args):
    from pfst_amd.config import Config, parse_cfg_options
    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    return cfg


def window_and_stride(args, cfg):
    """((h, w), (h, w)): --window / --stride, else the config's slide window, else 1024 / 512"""
    from pfst_amd.apis import window_defaults
    return window_defaults(cfg.model.get('test_cfg'), args.window, args.stride)


def list_images(inputs):
    """files as given, folders expanded to their images in name order -> [(path, stem)]; stems must be distinct (they name the outputs)"""
    paths = []
    for item in inputs:
        if os.path.isdir(item):
            paths += [os.path.join(item, f) for f in sorted(os.listdir(item)) if f.lower().endswith(IMAGE_SUFFIXES)]
        else:
            paths.append(item)
    out = [(p, os.path.splitext(os.path.basename(p))[0]) for p in paths]
    stems = [s for _, s in out]
    if len(set(stems)) != len(stems):
        raise SystemExit('two inputs share a file stem: their outputs would overwrite each other')
    if not out:
        raise SystemExit('no images found')
    return out


def write_label_png(path, labels, palette):
    """labels uint8 [H, W] -> a mode-P PNG: pixel values = class indices, embedded palette = `palette` (RGB rows)"""
    import numpy as np
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(labels, dtype=np.uint8))          # mode L; putpalette makes it P
    flat = [int(v) for colour in palette for v in colour]
    im.putpalette(flat + [0] * (768 - len(flat)))
    im.save(path)


def main(argv=None):
    args = parse_args(argv)
    import numpy as np
    import torch
    from PIL import Image
    import pfst_amd  # noqa: F401
    from pfst_amd.apis import init_segmentor, paint_result, predict_image
    cfg = load_config(args)
    crop, stride = window_and_stride(args, cfg)
    images = list_images(args.inputs)
    torch.cuda.set_device(args.gpu_id)
    try:
        model = init_segmentor(cfg, args.checkpoint, f'cuda:{args.gpu_id}', args.revise_checkpoint_key)
    except RuntimeError as e:
        if 'keys are missing' in str(e):
            raise SystemExit(str(e))
        raise
    os.makedirs(args.out_dir, exist_ok=True)
    ratios, flip = tta_options(args)
    records, total = [], None
    for path, stem in images:
        t0 = time.perf_counter()
        out = predict_image(model, path, crop, stride, args.windows_per_batch, confidence=args.confidence, ratios=ratios, flip=flip)
        labels = out['labels'].cpu().numpy()           # the read that waits for the device
        seconds = time.perf_counter() - t0
        write_label_png(os.path.join(args.out_dir, stem + '.png'), labels, model.PALETTE)
        if args.opacity is not None:
            over = paint_result(model, out['labels'], out['scene'], args.opacity)
            Image.fromarray(over.cpu().numpy()).save(os.path.join(args.out_dir, stem + '_overlay.png'))
        if args.confidence:
            Image.fromarray(out['confidence'].cpu().numpy()).save(os.path.join(args.out_dir, stem + '_conf.png'))
        records.append(dict(image=path, height=int(labels.shape[0]), width=int(labels.shape[1]), window=out['window'], windows=out['windows'],
                            batches=out['batches'], seconds=round(seconds, 4), views=out.get('views', 1)))
        gt = read_annotation(args.ann_dir, stem, args.reduce_zero_label) if args.ann_dir else None
        if gt is not None:
            if gt.shape != labels.shape:
                raise SystemExit(f'{stem}: the label map is {gt.shape[0]} x {gt.shape[1]}, the image {labels.shape[0]} x {labels.shape[1]}')
            from pfst_amd.evaluation import AreaAccumulator
            gt_d = torch.from_numpy(np.array(gt, np.uint8)).to(out['labels'].device)
            one = AreaAccumulator(model.num_classes, device=gt_d.device)
            one.update(out['labels'], gt_d)
            total = total or AreaAccumulator(model.num_classes, device=gt_d.device)
            total.hist += one.hist
            records[-1]['metric'] = metrics_record(one.areas())
        print(json.dumps(records[-1]), flush=True)
    with open(os.path.join(args.out_dir, 'predict.json'), 'w') as f:
        json.dump(dict(config=args.config, checkpoint=args.checkpoint, window=list(crop), stride=list(stride),
                       windows_per_batch=args.windows_per_batch, ratios=ratios, flip=flip, images=records,
                       **(dict(ann_dir=args.ann_dir, reduce_zero_label=args.reduce_zero_label, scored=sum('metric' in r for r in records),
                               metric=metrics_record(total.areas()) if total is not None else None) if args.ann_dir else {})), f, indent=1)
    return records


if __name__ == '__main__':
    main()
