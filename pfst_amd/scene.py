"""Whole-scene prediction: one complete image (an ISPRS scene, 6000 x 6000 for Potsdam) resident on the device as uint8 is covered with
the overlapping windows of `slide_inference` (encoder_decoder.py:220-263), the windows are forwarded in batches, and the sums of their
logits become a label map (+ confidence, + probabilities).  DESIGN.md §8f.

Per batch: scene_windows (cut + normalise, the arithmetic of pipeline.normalize) -> the eval-mode forward without its final resize ->
scene_accumulate_ (resize + add, gathered per scene pixel in window order); then scene_finalize (divide by the cover count, softmax,
arg-max).  Every kernel is bit-identical to the chain of the existing slide path it replaces; at one window per batch so is the whole
prediction, at more the f16x3 convolutions take their scales over the batch (the tolerance of DESIGN.md §8e)."""
import numpy as np
import torch

from . import hip_ops as ops
from .layers import bn_eval


def window_grid(H, W, crop, stride):
    """the windows of slide_inference (encoder_decoder.py:231-243) in its row-major order -> ([(y1, x1), ...], (h, w)): one every `stride`
    pixels, the last of a row / column shifted back inside the image; on an axis where the image is smaller than the crop the windows are
    clipped to it, so all windows of a scene have one size"""
    (h_crop, w_crop), (h_stride, w_stride) = crop, stride
    if min(H, W, h_crop, w_crop, h_stride, w_stride) < 1:
        raise ValueError(f'window_grid: sizes must be positive, got {(H, W)}, crop {crop}, stride {stride}')
    h_grids = max(H - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(W - w_crop + w_stride - 1, 0) // w_stride + 1
    wins = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y2, x2 = min(h_idx * h_stride + h_crop, H), min(w_idx * w_stride + w_crop, W)
            wins.append((max(y2 - h_crop, 0), max(x2 - w_crop, 0)))
    return wins, (min(h_crop, H), min(w_crop, W))


def cover_counts(H, W, crop, stride):
    """(rows int32 [H], cols int32 [W]): windows of the grid covering each row / each column.  The grid is a product of row and column
    offsets, so the cover count of pixel (y, x) -- the reference's count_mat -- is rows[y] * cols[x]"""
    wins, (h, w) = window_grid(H, W, crop, stride)
    rows, cols = np.zeros(H, np.int32), np.zeros(W, np.int32)
    for y1 in sorted({y for y, _ in wins}):
        rows[y1:y1 + h] += 1
    for x1 in sorted({x for _, x in wins}):
        cols[x1:x1 + w] += 1
    assert rows.min() >= 1 and cols.min() >= 1              # the reference's `assert (count_mat == 0).sum() == 0`
    return rows, cols


_tables = {}


def _count_tables(H, W, crop, stride, dev):
    """cover_counts on the device, uploaded once per scene geometry (a folder of equally sized scenes shares them)"""
    key = (H, W, crop, stride, str(dev))
    t = _tables.get(key)
    if t is None:
        if len(_tables) >= 8:
            _tables.clear()
        rows, cols = cover_counts(H, W, crop, stride)
        t = _tables[key] = (torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev))
    return t


# peak bytes of the eval-mode forward per input pixel of a batch (fp32): the 3-channel window (12), the widest live pair of layers of
# ResNetV1c-50 + the ASPP head without a tape -- layer1's 256 channels at 1/4 resolution in and out plus a 64-channel bottleneck
# ((256 + 256 + 64) / 16 floats = 144 bytes) -- and the stem at 1/2 resolution (64 + 64 channels / 4 floats = 128 bytes, not live at the same
# time), doubled for allocator slack and the f16x3 operand images
ACTIVATION_BYTES_PER_PIXEL = 2 * (12 + 144)


def memory_needed(C, H, W, size, windows_per_batch, confidence=False, return_probs=False):
    """-> (bytes of the sums and outputs, estimated bytes of one batch's activations)"""
    fixed = 4 * C * H * W * (2 if return_probs else 1) + H * W * (2 if confidence else 1)
    return fixed, ACTIVATION_BYTES_PER_PIXEL * windows_per_batch * size[0] * size[1]


def low_res_logits(seg, img):
    """the forward of `_eval_encode_decode` (BatchNorm on running statistics, dropout off) without its final resize: [B, C, hl, wl]"""
    with bn_eval():
        x = seg.extract_feat(img, None)
        logits = seg.decode_head(x, return_features=False, tape=None, training=False)
    return logits.data


def predict_scene(seg, scene_u8, norm_cfg, crop, stride, windows_per_batch=8, confidence=False, return_probs=False, stats=None):
    """Labels of a whole scene.  seg: an EncoderDecoder on the device; scene_u8: device uint8 [H, W, 3] as read from the file (BGR);
    norm_cfg: dict(mean, std, to_rgb) of the pipeline's Normalize; crop / stride: (h, w) pairs of the sliding window.
    -> (labels uint8 [H, W], confidence uint8 [H, W] or None, probabilities float32 [C, H, W] or None), device tensors: nothing here
    synchronises, the caller's read of the labels does.  `stats` (a dict) receives the window and batch counts."""
    if not (scene_u8.is_cuda and scene_u8.dtype == torch.uint8 and scene_u8.dim() == 3 and scene_u8.shape[2] == 3):
        raise ValueError('predict_scene needs a device uint8 [H, W, 3] scene')
    if not 1 <= windows_per_batch <= ops.SCENE_MAX_WINDOWS:
        raise ValueError(f'windows_per_batch must lie in 1 .. {ops.SCENE_MAX_WINDOWS}, got {windows_per_batch}')
    H, W = scene_u8.shape[:2]
    C = seg.num_classes
    dev = scene_u8.device
    wins, size = window_grid(H, W, crop, stride)
    B = min(windows_per_batch, len(wins))
    fixed, act = memory_needed(C, H, W, size, B, confidence, return_probs)
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if fixed + act > free:
        raise MemoryError(f'predict_scene: a {H} x {W} scene with {C} classes needs {fixed / 2**20:.0f} MiB for its sums and outputs plus about '
                          f'{act / 2**20:.0f} MiB for the activations of {B} windows of {size[0]} x {size[1]}; {free / 2**20:.0f} MiB of device '
                          'memory are free.  Lower windows_per_batch or the window size, or cut the scene: it is not tiled silently')
    scene_u8 = scene_u8.contiguous()
    rows_d, cols_d = _count_tables(H, W, tuple(crop), tuple(stride), dev)
    mean, std, to_rgb = norm_cfg['mean'], norm_cfg['std'], norm_cfg.get('to_rgb', True)
    seg.repack_weights(need_dgrad=False)
    sums = torch.zeros(C, H, W, device=dev)
    batches = 0
    for i in range(0, len(wins), B):
        batch = wins[i:i + B]
        img = ops.scene_windows(scene_u8, batch, size, mean, std, to_rgb)
        ops.scene_accumulate_(sums, low_res_logits(seg, img), batch, size)
        batches += 1
    if stats is not None:
        stats.update(windows=len(wins), batches=batches, window=list(size))
    return ops.scene_finalize(sums, rows_d, cols_d, confidence, return_probs)


# ---------------------------------------------------------------------------------------------------------------- test-time augmentation
def tta_views(H, W, ratios, flip, flip_direction='horizontal'):
    """The views of MultiScaleFlipAug(img_scale=None, img_ratios=ratios, flip=flip, flip_direction=...) for an H x W scene, in the order of
    Pipeline._views (test_time_aug.py:98-126): scale-major, then flip False / True.  -> [dict(ratio, scale_index, size=(Hr, Wr), flip,
    flip_direction)]; the size is what the pipeline's Resize(keep_ratio=True) makes of the scale (int(W * r), int(H * r))"""
    from .pipeline import rescale_size
    ratios = list(ratios) if isinstance(ratios, (list, tuple)) else [ratios]
    if not ratios or not all(isinstance(r, float) and r > 0 for r in ratios):
        raise ValueError(f'tta_views: ratios must be positive floats (MultiScaleFlipAug img_ratios), got {ratios}')
    if flip_direction not in ('horizontal', 'vertical'):
        raise ValueError(f"tta_views: flip_direction must be 'horizontal' or 'vertical', got {flip_direction}")
    if min(H, W) < 1:
        raise ValueError(f'tta_views: sizes must be positive, got {(H, W)}')
    views = []
    for si, r in enumerate(ratios):
        size = rescale_size((H, W), (int(W * r), int(H * r))) if min(int(W * r), int(H * r)) >= 1 else (0, 0)
        if min(size) < 1:
            raise ValueError(f'tta_views: ratio {r} leaves nothing of a {H} x {W} scene')
        for f in ([False, True] if flip else [False]):
            views.append(dict(ratio=r, scale_index=si, size=size, flip=f, flip_direction=flip_direction))
    return views


def tta_memory_needed(C, H, W, views, crop, stride, windows_per_batch, confidence=False, return_probs=False):
    """-> (bytes of the sum over views and the outputs, bytes of the largest view's window sums + its resized scene, estimated bytes of one
    batch's activations at the view where they are largest)"""
    fixed = 4 * C * H * W * (2 if return_probs else 1) + H * W * (2 if confidence else 1)
    view, act = 0, 0
    for v in views:
        hr, wr = v['size']
        wins, size = window_grid(hr, wr, crop, stride)
        resized = 0 if (hr, wr) == (H, W) and not v['flip'] else 3 * hr * wr
        view = max(view, 4 * C * hr * wr + resized)
        act = max(act, ACTIVATION_BYTES_PER_PIXEL * min(windows_per_batch, len(wins)) * size[0] * size[1])
    return fixed, view, act


def _view_add_chain(acc, sums, rows_d, cols_d, out_hw, hflip, vflip):
    """what pfst_scene_tta_accumulate fuses, from the existing ops (more than ops.TTA_MAX_C classes): the same values"""
    count = (rows_d[:, None] * cols_d[None, :]).to(torch.float32)[None, None].contiguous()
    p = ops.window_normalize_(sums[None], count)
    if tuple(p.shape[2:]) != tuple(out_hw):
        p = ops.resize_bilinear(p, out_hw)
    p = ops.softmax_nchw(p)
    if hflip or vflip:
        p = ops.flip_planes(p, horizontal=hflip, vertical=vflip)
    if acc is None:
        return p[0]
    return ops.axpy_(acc, p[0])


def predict_scene_tta(seg, scene_u8, norm_cfg, crop, stride, ratios, flip=True, flip_direction='horizontal', windows_per_batch=8,
                      confidence=False, return_probs=False, stats=None):
    """Labels of a whole scene with multi-scale + flip test-time augmentation: aug_test (encoder_decoder.py:355-372) over slide_inference, the
    views of tta_views.  Per view the scene is resized with the pipeline's bilinear arithmetic and mirrored on the device (ratio 1 unflipped:
    the scene itself), goes through predict_scene's window path unchanged, and its window sums become probabilities at the scene's size,
    un-flipped and added to the sum over views, in one pass; the sum / views -> first maximal class.  Arguments and result as predict_scene;
    ratios: positive floats that multiply the scene's own size (the config's img_scale is not used: the scene is its own scale).  Nothing here
    synchronises.  `stats` receives views, view_windows (per view), windows, batches and the window size of the first view."""
    if not (scene_u8.is_cuda and scene_u8.dtype == torch.uint8 and scene_u8.dim() == 3 and scene_u8.shape[2] == 3):
        raise ValueError('predict_scene_tta needs a device uint8 [H, W, 3] scene')
    if not 1 <= windows_per_batch <= ops.SCENE_MAX_WINDOWS:
        raise ValueError(f'windows_per_batch must lie in 1 .. {ops.SCENE_MAX_WINDOWS}, got {windows_per_batch}')
    H, W = scene_u8.shape[:2]
    C = seg.num_classes
    dev = scene_u8.device
    crop, stride = tuple(crop), tuple(stride)
    views = tta_views(H, W, ratios, flip, flip_direction)
    fixed, view, act = tta_memory_needed(C, H, W, views, crop, stride, windows_per_batch, confidence, return_probs)
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if fixed + view + act > free:
        big = max(views, key=lambda v: v['size'][0] * v['size'][1])['size']
        raise MemoryError(f'predict_scene_tta: a {H} x {W} scene with {C} classes and {len(views)} views needs {fixed / 2**20:.0f} MiB for the sum '
                          f'over views and the outputs, {view / 2**20:.0f} MiB for the window sums and the resized scene of its largest view '
                          f'({big[0]} x {big[1]}) and about {act / 2**20:.0f} MiB for the activations of a batch of windows; {free / 2**20:.0f} '
                          'MiB of device memory are free.  Lower windows_per_batch, the window size or the ratios, or cut the scene: it is not '
                          'tiled silently')
    scene_u8 = scene_u8.contiguous()
    mean, std, to_rgb = norm_cfg['mean'], norm_cfg['std'], norm_cfg.get('to_rgb', True)
    seg.repack_weights(need_dgrad=False)
    fused = C <= ops.TTA_MAX_C
    acc = torch.empty(C, H, W, device=dev) if fused else None
    view_windows, batches, first_size = [], 0, None
    for vi, v in enumerate(views):
        hr, wr = v['size']
        hflip, vflip = v['flip'] and v['flip_direction'] == 'horizontal', v['flip'] and v['flip_direction'] == 'vertical'
        plain = (hr, wr) == (H, W) and not (hflip or vflip)
        view_u8 = scene_u8 if plain else ops.scene_resize_u8(scene_u8, (hr, wr), hflip, vflip)
        wins, size = window_grid(hr, wr, crop, stride)
        rows_d, cols_d = _count_tables(hr, wr, crop, stride, dev)
        B = min(windows_per_batch, len(wins))
        sums = torch.zeros(C, hr, wr, device=dev)
        for i in range(0, len(wins), B):
            batch = wins[i:i + B]
            img = ops.scene_windows(view_u8, batch, size, mean, std, to_rgb)
            ops.scene_accumulate_(sums, low_res_logits(seg, img), batch, size)
            batches += 1
        if fused:
            ops.scene_tta_accumulate_(acc, sums, rows_d, cols_d, hflip, vflip, accumulate=vi > 0)
        else:
            acc = _view_add_chain(acc, sums, rows_d, cols_d, (H, W), hflip, vflip)
        view_windows.append(len(wins))
        first_size = first_size or list(size)
        del sums, view_u8
    if stats is not None:
        stats.update(views=len(views), view_windows=view_windows, windows=sum(view_windows), batches=batches, window=first_size)
    return ops.scene_tta_finalize(acc, len(views), confidence, return_probs)
