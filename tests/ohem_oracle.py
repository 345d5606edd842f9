"""Plain-torch restatement of OHEMPixelSampler for the sampler tests, in float32 or float64: the formulas of
rsiseg/core/seg/sampler/ohem_pixel_sampler.py behind the decode head's bilinear resize, with the project's decisions (a label outside [0, C)
is not valid; ties at the cut of the top-k mode are kept in raster order).  tests/test_ohem_cpu.py pins the float32 form against the weight
maps the reference's own file returned (tests/golden/ohem_sampler.npz)."""
import numpy as np
import torch
import torch.nn.functional as F

P_REL = 2e-5          # relative error allowed on a key p (|logit| <= 32): 2 x (3 * 2^-24 * 32 + (C + 4) * 2^-24), C <= 19
NLL_ABS = 2e-5        # absolute error allowed on a key nll
BAND_SHARE = 0.0025   # condition on the inputs: at most this share of the valid pixels may lie in the band around the cut


def upsample(logits, size, dtype):
    z = logits.to(dtype)
    return z if tuple(z.shape[2:]) == tuple(size) else F.interpolate(z, size=tuple(size), mode='bilinear', align_corners=False)


def keys(logits, label, ignore_index=255, thresh_mode=True, coef=None, dtype=torch.float64):
    """logits [N, C, h, w] (CPU), label uint8 [N, H, W] -> (key [N, H, W] in dtype: p_label, or coef[y] * max(nll, 0); -1 where not valid,
    valid bool [N, H, W])"""
    C = logits.shape[1]
    lab = label.long()
    valid = (lab != ignore_index) & (lab < C)
    z = upsample(logits, label.shape[-2:], dtype)
    idx = torch.where(valid, lab, torch.zeros_like(lab)).unsqueeze(1)
    if thresh_mode:
        key = F.softmax(z, dim=1).gather(1, idx).squeeze(1)
    else:
        nll = F.cross_entropy(z, idx.squeeze(1), reduction='none').clamp_min(0)
        cf = torch.ones(C, dtype=dtype) if coef is None else torch.as_tensor(coef, dtype=torch.float32).to(dtype)
        key = cf[idx.squeeze(1)] * nll
    return torch.where(valid, key, torch.full_like(key, -1)), valid


def thresh32(thresh):
    return float(np.float32(thresh))


def select_thresh(key, valid, thresh, batch_kept):
    """-> (weight float32 [N, H, W], threshold as a Python float in key's precision, k)"""
    v = key[valid]
    if v.numel() == 0:
        return torch.zeros(key.shape), thresh32(thresh), 0
    k = min(int(batch_kept), v.numel() - 1)
    thr = max(float(v.sort()[0][k]), thresh32(thresh))
    return (valid & (key < thr)).float(), thr, k


def select_topk(key, valid, batch_kept):
    """-> (weight float32 [N, H, W], cut value (inf when nothing is kept), m): the m = min(batch_kept, n_valid) largest keys, a stable
    descending sort over the raster order -- pixels equal to the cut are taken in raster order"""
    flat, vf = key.reshape(-1), valid.reshape(-1)
    pos = vf.nonzero().flatten()
    m = min(int(batch_kept), pos.numel())
    w = torch.zeros(flat.numel())
    if m == 0:
        return w.view(key.shape), float('inf'), 0
    s, order = flat[pos].sort(descending=True, stable=True)
    w[pos[order[:m]]] = 1.0
    return w.view(key.shape), float(s[m - 1]), m


def band_thresh(key64, valid, thr64):
    """the pixels a key error of P_REL (relative; on the pixel's key and, through s[k], on the threshold) can move across the threshold"""
    return valid & ((key64 - thr64).abs() <= P_REL * (key64.abs() + abs(thr64)))


def band_topk(key64, valid, cut64, coef_max=1.0):
    return valid & ((key64 - cut64).abs() <= 2 * NLL_ABS * coef_max)


def ce_under_weights(logits, label, weight, ignore_index=255, class_weight=None, loss_weight=1.0):
    """fp64 CE of the head (mean over ALL pixels) under a fixed pixel-weight map, with autograd -> (loss, d logits)"""
    z = logits.double().clone().requires_grad_()
    up = upsample(z, label.shape[-2:], torch.float64)
    cw = None if class_weight is None else torch.tensor(class_weight, dtype=torch.float64)
    nll = F.cross_entropy(up, label.long(), weight=cw, ignore_index=ignore_index, reduction='none')
    loss = loss_weight * (nll * weight.double()).sum() / label.numel()
    loss.backward()
    return float(loss.detach()), z.grad
