"""fp64 restatement of the class-wise entropy thresholds and the pseudo-label cut for the pseudo-label tests: the formulas of
PseudoLabelingHookV4._cal_threshold and LoadAnnotationsPseudoLabelsV2.__call__ in float64 NumPy, pinned against numbers the reference's own
files returned (tests/golden/pseudo_labels.npz) by tests/test_pseudo_labels_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F


def upsample64(logits, size):
    """fp32 logits [N, C, h, w] (NumPy) -> float64 [N, C, H, W]: the bilinear resize (align_corners=False) in float64; identity sizes pass"""
    z = torch.from_numpy(np.asarray(logits, np.float32)).double()
    if tuple(z.shape[2:]) != tuple(size):
        z = F.interpolate(z, size=tuple(size), mode='bilinear', align_corners=False)
    return z.numpy()


def softmax64(z):
    """float64 [N, C, H, W] -> probabilities, exp(z - max) / sum"""
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def top2_gap(p):
    """the difference of the two largest probabilities per pixel"""
    s = np.sort(p, axis=1)
    return s[:, -1] - s[:, -2] if p.shape[1] > 1 else np.ones_like(s[:, -1])


def hook_entropy(p):
    """-sum p log p, a term with p == 0 taken as 0 -> (entropy, arg-max of p)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    return -t.sum(axis=1), p.argmax(axis=1)


def loader_entropy(z, p):
    """-sum p log(p + 1e-8) -> (entropy, arg-max of the logits)"""
    return -(p * np.log(p + 1e-8)).sum(axis=1), z.argmax(axis=1)


def thresholds(ent, pred, ratios, num_classes, drop=None):
    """thr[r][c] = sorted(ent | pred == c)[int(n_c r)], 0 for an empty class; `drop`: flat indices (over N, H, W) left out, as the
    reference's permutation leaves one out -> (table [R][C] in ent's dtype, n_c)"""
    e, q = ent.reshape(-1), pred.reshape(-1)
    if drop is not None:
        keep = np.ones(e.size, bool)
        keep[np.asarray(drop).reshape(-1)] = False
        e, q = e[keep], q[keep]
    table = np.zeros((len(ratios), num_classes), ent.dtype)
    n_c = np.zeros(num_classes, np.int64)
    for c in range(num_classes):
        s = np.sort(e[q == c])
        n_c[c] = s.size
        for i, r in enumerate(ratios):
            table[i, c] = s[int(s.size * r)] if s.size else 0
    return table, n_c


def labels(ent, pred, thr, annotation_space=False):
    """pred where ent < thr[pred], else 255 (annotation space: pred + 1, else 0) -> (uint8 labels, counts [C][2] (predicted, kept))"""
    thr = np.asarray(thr)
    keep = ent < thr[pred]
    out = np.where(keep, pred + 1, 0) if annotation_space else np.where(keep, pred, 255)
    C = thr.size
    counts = np.stack([np.bincount(pred.reshape(-1), minlength=C), np.bincount(pred[keep].reshape(-1), minlength=C)], 1).astype(np.int64)
    return out.astype(np.uint8), counts


def midpoint_thresholds(ent, pred, ratio, num_classes, min_gap):
    """Per class a threshold in the MIDDLE of a gap >= min_gap between consecutive order statistics of `ent`, the gap nearest to rank
    int(n_c ratio) -> (thr float32 [C], ok): ok is False when some non-empty class has no such gap.  An empty class gets 0."""
    thr = np.zeros(num_classes, np.float32)
    ok = True
    for c in range(num_classes):
        s = np.sort(ent[pred == c].reshape(-1))
        if s.size < 2:
            thr[c] = 0.0 if s.size == 0 else np.float32(s[0] + 1.0)
            continue
        gaps = np.diff(s)
        cand = np.nonzero(gaps >= min_gap)[0]
        if cand.size == 0:
            ok = False
            continue
        k = cand[np.argmin(np.abs(cand - int(s.size * ratio)))]
        thr[c] = np.float32(0.5 * (s[k] + s[k + 1]))
        # the float32 rounding of the midpoint must leave it strictly inside the gap, with room on both sides
        ok = ok and (float(thr[c]) - s[k] >= 0.4 * min_gap) and (s[k + 1] - float(thr[c]) >= 0.4 * min_gap)
    return thr, ok
