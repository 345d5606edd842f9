"""The inference API of the reference (rsiseg/apis/inference.py): `init_segmentor` builds a segmentor from a config and a checkpoint,
`inference_segmentor` predicts one image.  Here an image is a whole scene at its native resolution, predicted with batched sliding
windows (pfst_amd/scene.py); `predict_image` is the same call with everything left on the device, for tools/predict.py."""
import numpy as np
import torch

from . import hip_ops as ops
from .config import Config
from .scene import predict_scene, predict_scene_tta

DEFAULT_WINDOW, DEFAULT_STRIDE = 1024, 512


def find_normalize(pipeline):
    """dict(mean, std, to_rgb) of the `Normalize` step of a config pipeline, found by type, also inside a MultiScaleFlipAug's transforms;
    None when the pipeline has none"""
    for step in pipeline or []:
        if step.get('type') == 'Normalize':
            return dict(mean=list(step['mean']), std=list(step['std']), to_rgb=bool(step.get('to_rgb', True)))
        if step.get('type') == 'MultiScaleFlipAug':
            found = find_normalize(step.get('transforms'))
            if found is not None:
                return found
    return None


def scene_norm_cfg(pipeline):
    """the normalisation a scene gets: the pipeline's Normalize, or without one what the loader's metas carry (mean 0, std 1, no channel
    swap: LoadImageFromFile's default, as pfst_amd.pipeline.Pipeline.__call__ sets it)"""
    types = {s.get('type') for s in pipeline or []}
    if types & {'ClipNormalize', 'Uint82Float'}:
        raise NotImplementedError('scene prediction reads 8-bit three-band images; a pipeline with ClipNormalize / Uint82Float (season_net) is '
                                  'outside it')
    return find_normalize(pipeline) or dict(mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], to_rgb=False)


def window_defaults(test_cfg, window=None, stride=None):
    """((h, w) crop, (h, w) stride) of the sliding window: the arguments (a number or an (h, w) pair each) when given, else test_cfg's
    crop_size / stride when it is a `slide` config, else 1024 / 512"""
    slide = bool(test_cfg) and test_cfg.get('mode', 'whole') == 'slide'
    pair = lambda v: (int(v[0]), int(v[1])) if isinstance(v, (list, tuple)) else (int(v),) * 2
    crop = pair(window) if window else pair(test_cfg['crop_size']) if slide else (DEFAULT_WINDOW,) * 2
    step = pair(stride) if stride else pair(test_cfg['stride']) if slide else (DEFAULT_STRIDE,) * 2
    return crop, step


def init_segmentor(config, checkpoint=None, device='cuda:0', revise_checkpoint_key=False, teacher=False):
    """config: a file name or a Config.  The checkpoint's `state_dict` is loaded as tools/test.py loads it: with `revise_checkpoint_key` the
    DDP `module.` and the UDA wrapper's `model.` prefixes are stripped first (a PFGST checkpoint needs it), and segmentor keys the checkpoint
    does not have are an error.  `teacher`: the EMA teacher of a PFGST checkpoint instead of its student (evaluation.teacher_checkpoint_keys).
    The model carries `cfg`, `CLASSES` and `PALETTE` (the checkpoint's meta, else the ISPRS ones)."""
    from .data import ISPRS_CLASSES, ISPRS_PALETTE
    from .evaluation import revise_checkpoint_keys, teacher_checkpoint_keys
    from .registry import build_segmentor
    if isinstance(config, str):
        config = Config.fromfile(config)
    elif not isinstance(config, Config):
        raise TypeError(f'config must be a filename or Config object, but got {type(config)}')
    config.model['pretrained'] = None
    config.model['train_cfg'] = None
    model = build_segmentor(config.model)
    meta = {}
    if checkpoint is not None:
        ckpt = torch.load(checkpoint, map_location='cpu', weights_only=False)
        sd = ckpt.get('state_dict', ckpt)
        if teacher:
            sd = teacher_checkpoint_keys(sd)
        elif revise_checkpoint_key:
            sd = revise_checkpoint_keys(sd)
        missing = model.load_state_dict(sd, strict=False)
        own = [k for k in missing.missing_keys if not k.endswith('num_batches_tracked')]
        if own:
            raise RuntimeError(f'{len(own)} segmentor keys are missing from the checkpoint (first: {own[:3]}); a PFGST checkpoint needs '
                               'revise_checkpoint_key=True (--revise-checkpoint-key)')
        meta = ckpt.get('meta') or {} if isinstance(ckpt, dict) else {}
    model.CLASSES = tuple(meta.get('CLASSES') or ISPRS_CLASSES)
    model.PALETTE = [list(c) for c in (meta.get('PALETTE') or ISPRS_PALETTE)]
    model.cfg = config
    model.to(device)
    return model


def predict_image(model, img, window=None, stride=None, windows_per_batch=8, confidence=False, return_probs=False, ratios=None, flip=False,
                  flip_direction='horizontal'):
    """img: a path or an H x W x 3 BGR uint8 array -> dict(scene, labels, confidence, probs, windows, batches, window): device tensors
    (confidence / probs None unless asked for) and the window / batch counts.  The scene is predicted at its native resolution; with
    `ratios` (floats that multiply the scene's size) and / or `flip` it is predicted with test-time augmentation, the probabilities of
    every resized / mirrored view averaged at the scene's size (scene.predict_scene_tta; the dict then also holds views and view_windows)."""
    from .data import _read_image_bgr
    if isinstance(img, (str, bytes)) or hasattr(img, '__fspath__'):
        img = _read_image_bgr(img)
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f'an image is a path or an H x W x 3 uint8 array (BGR), got {img.dtype} {img.shape}')
    cfg = model.cfg
    data_test = (cfg.get('data') or {}).get('test') or {}
    norm = scene_norm_cfg(data_test.get('pipeline'))
    crop, step = window_defaults(model.test_cfg, window, stride)
    dev = next(model.parameters()).device
    scene = torch.from_numpy(np.ascontiguousarray(img)).to(dev)
    stats = {}
    with torch.no_grad():
        if ratios is None and not flip:
            labels, conf, probs = predict_scene(model, scene, norm, crop, step, windows_per_batch, confidence, return_probs, stats)
        else:
            labels, conf, probs = predict_scene_tta(model, scene, norm, crop, step, [1.0] if ratios is None else ratios, flip, flip_direction,
                                                    windows_per_batch, confidence, return_probs, stats)
    return dict(scene=scene, labels=labels, confidence=conf, probs=probs, **stats)


def inference_segmentor(model, img, **options):
    """-> [labels]: a list holding the H x W uint8 label array of the image, as the reference returns a list (with confidence=True /
    return_probs=True those arrays follow the labels).  options: window, stride, windows_per_batch, confidence, return_probs, and for
    test-time augmentation ratios, flip, flip_direction."""
    out = predict_image(model, img, **options)
    res = [out['labels'].cpu().numpy()]
    res += [out[k].cpu().numpy() for k in ('confidence', 'probs') if out[k] is not None]
    return res


def paint_result(model, result, scene=None, opacity=None, palette=None):
    """BaseSegmentor.show_result (segmentors/base.py:227-300) on the device: labels (device uint8 [H, W]) -> uint8 [H, W, 3] RGB painted
    with the model's palette, blended over `scene` (device uint8 [H, W, 3], BGR) when an opacity is given"""
    pal = np.asarray(model.PALETTE if palette is None else palette, np.uint8)
    assert pal.ndim == 2 and pal.shape[1] == 3
    pal_d = torch.from_numpy(pal).to(result.device)
    return ops.paint_labels(result, pal_d, scene if opacity is not None else None, opacity)
