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
