"""fp64 NumPy restatement of the reference's EntropyLoss (rsiseg/models/losses/entropy_loss.py:27-42), the 1e-30 included, and its gradient
with respect to the logits as autograd forms it: the seed g = dL/dp through the softmax's Jacobian.

    p = softmax_c(z)
    entropy:     L = w * mean_px( -sum_c p_c log2(p_c + 1e-30) / log2 C )     g_c = -(log2(p_c + eps) + p_c / ((p_c + eps) ln 2)) / log2 C * w / (N h w)
    max_square:  L = -w * mean(p^2) / 2                                        g_c = -p_c * w / (N C h w)
    dL/dz_j = p_j (g_j - sum_c p_c g_c)
"""
import numpy as np

EPS = 1e-30
WEIGHT_KEYS = {'entropy': 'loss_ent', 'max_square': 'loss_max_square'}


def softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def entropy_loss(logits, loss_type, weight):
    """-> (loss float64, d loss / d logits float64 [N, C, h, w])"""
    p = softmax64(logits)
    n, c, h, w = p.shape
    weight = float(weight)
    if loss_type == 'entropy':
        loss = weight * (-(p * np.log2(p + EPS)) / np.log2(c)).sum(axis=1).mean()
        g = -(np.log2(p + EPS) + p / ((p + EPS) * np.log(2.0))) / np.log2(c) * weight / (n * h * w)
    elif loss_type == 'max_square':
        loss = -weight * (p ** 2).mean() / 2
        g = -p * weight / (n * c * h * w)
    else:
        raise ValueError(loss_type)
    grad = p * (g - (p * g).sum(axis=1, keepdims=True))
    return float(loss), grad


def per_link_excess(got, ref):
    """max over elements of |got - ref| - (1e-4 max|ref| + 1e-3 |ref|): <= 0 within the project's per-link bound"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) - (1e-4 * np.abs(ref).max() + 1e-3 * np.abs(ref))).max())
