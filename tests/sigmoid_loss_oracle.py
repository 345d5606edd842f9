"""fp64 oracle of the sigmoid decode-head losses (FocalLoss, CrossEntropyLoss(use_sigmoid=True)) behind the head's bilinear resize: the closed
form of DESIGN.md section 8k in plain torch, and the literal formulas of the reference (focal_loss.py:45-67, cross_entropy_loss.py:68-156)
for fp64 autograd to compare it with.

    y = t ? -x : x,  q = sigmoid(y),  b = softplus(y),  k = coef[c][t ? 0 : 1]
    l = k q^gamma b,  dl/dx = (t ? -1 : 1) k q^gamma (q + gamma (1 - q) b)

1 - q is sigmoid(-y), q^gamma is exp(-gamma softplus(-y)) (1 at gamma = 0): no negative power, finite everywhere."""
import numpy as np
import torch
import torch.nn.functional as F


def focal_coef(C, alpha=0.5, class_weight=None):
    alpha = list(alpha) if isinstance(alpha, (list, tuple)) else [alpha] * C
    cw = class_weight if class_weight is not None else [1.0] * C
    return [[w * a, w * (1.0 - a)] for w, a in zip(cw, alpha)]


def bce_coef(C, class_weight=None):
    cw = class_weight if class_weight is not None else [1.0] * C
    return [[float(w), 1.0] for w in cw]


def divisor(reduction, n, c, H, W):
    return 1.0 if reduction == 'sum' else float(n * c * H * W)


def upsample(z, size):
    return F.interpolate(z, size=tuple(size), mode='bilinear', align_corners=False)


def _masks(label, C, weight, ign):
    lab = label.reshape(label.shape[0], *label.shape[-2:]).long()
    valid = (lab != ign) & (lab < C)
    t = torch.zeros(lab.shape[0], C, *lab.shape[1:], dtype=torch.bool)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    t.scatter_(1, safe.unsqueeze(1), valid.unsqueeze(1))
    w = valid.double() if weight is None else weight.double().reshape(lab.shape) * valid.double()
    return lab, valid, t, w


def elementwise(x, t, coef, gamma):
    """x fp64 [N,C,H,W], t bool one-hot -> (l, dl/dx) by the closed form"""
    k = torch.tensor(coef, dtype=torch.float64)
    kk = torch.where(t, k[:, 0].view(1, -1, 1, 1), k[:, 1].view(1, -1, 1, 1))
    y = torch.where(t, -x, x)
    L = torch.log1p(torch.exp(-y.abs()))
    b = y.clamp(min=0) + L
    e = torch.exp(-y.abs())
    r = 1.0 / (1.0 + e)
    q = torch.where(y >= 0, r, e * r)
    p = torch.where(y >= 0, e * r, r)
    qg = torch.ones_like(q) if gamma == 0 else torch.exp(-gamma * ((-y).clamp(min=0) + L))
    sign = torch.where(t, -torch.ones_like(x), torch.ones_like(x))
    return kk * qg * b, sign * kk * qg * (q + gamma * p * b)


def sigmoid_loss(z, label, size, coef, gamma=0.0, weight=None, ign=255, reduction='mean', loss_weight=1.0, grad_scale=1.0):
    """z [N,C,h,w] (any float dtype; computed in fp64), label uint8 [N,(1,)H,W], weight [N,H,W] or None.
    -> dict(loss, sums [N, C] = sum_px w valid l_c, grad = d(grad_scale * loss) / dz, counts = (#correct, #valid, #bad), map = weighted l)"""
    z64 = z.detach().double().requires_grad_()
    n, C = z64.shape[:2]
    x = upsample(z64, size)
    lab, valid, t, w = _masks(label, C, weight, ign)
    l, g = elementwise(x.detach(), t, coef, gamma)
    wl = l * w.unsqueeze(1)
    D = divisor(reduction, n, C, *size)
    (dz,) = torch.autograd.grad(x, z64, grad_outputs=g * w.unsqueeze(1) * (loss_weight * grad_scale / D))
    arg = x.detach().argmax(1)
    correct = int(((arg == lab) & valid).sum())
    bad = int(((lab != ign) & (lab >= C)).sum())
    sums = wl.sum(dim=(2, 3))
    return dict(loss=float(loss_weight * sums.sum() / D), sums=sums.numpy(), grad=dz.numpy(), counts=(correct, int(valid.sum()), bad), map=wl)


def literal_loss(z, label, size, kind, gamma=2.0, alpha=0.5, class_weight=None, weight=None, ign=255, reduction='mean', loss_weight=1.0,
                 dtype=torch.float64):
    """the reference's formulas as written, differentiated by autograd in `dtype` -> (loss, dz).  kind: 'focal' | 'bce'"""
    zz = z.detach().to(dtype).requires_grad_()
    n, C = zz.shape[:2]
    x = upsample(zz, size)
    lab, valid, t, w = _masks(label, C, weight, ign)
    tf, w = t.to(dtype), w.to(dtype).unsqueeze(1)
    if kind == 'focal':
        a = torch.tensor(list(alpha) if isinstance(alpha, (list, tuple)) else [alpha] * C, dtype=dtype).view(1, C, 1, 1)
        ps = x.sigmoid()
        one_minus_pt = (1 - ps) * tf + ps * (1 - tf)
        fw = (a * tf + (1 - a) * (1 - tf)) * one_minus_pt.pow(gamma)
        l = F.binary_cross_entropy_with_logits(x, tf, reduction='none') * fw
        if class_weight is not None:
            l = l * torch.tensor(class_weight, dtype=dtype).view(1, C, 1, 1)
    else:
        pos = None if class_weight is None else torch.tensor(class_weight, dtype=dtype).view(1, C, 1, 1)
        l = F.binary_cross_entropy_with_logits(x, tf, pos_weight=pos, reduction='none')
    loss = loss_weight * (l * w).sum() / divisor(reduction, n, C, *size)
    (dz,) = torch.autograd.grad(loss, zz)
    return float(loss.detach()), dz.double().numpy()


def link_bound(ref):
    """the per-link gradient bound of DESIGN.md section 7, per element: 1e-4 max|ref| + 1e-3 |ref|"""
    ref = np.asarray(ref, dtype=np.float64)
    return 1e-4 * np.abs(ref).max() + 1e-3 * np.abs(ref)


def worst_ratio(got, ref):
    """max over elements of |got - ref| / bound; <= 1 passes.  A zero reference with a zero result counts as 0."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = link_bound(ref)
    err = np.abs(got - ref)
    if not np.isfinite(got).all():
        return float('inf')
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))))


# ---- the shared cases of the CPU and GPU tests (tests/golden/make_golden_focal.py documents the stored ones)
def expand_blocks(blocks, size):
    H, W = size
    return blocks.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()


def load_fixture(path):
    gold = np.load(path)
    return {k: gold[k] for k in gold.files}
