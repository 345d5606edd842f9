"""Seeded inputs and float64 references of the kernel-level tests of csrc/loss.hip (tests/test_ce_edges_cpu.py, tests/test_ce_edges_gpu.py):
the decode heads' fused bilinear resize + cross-entropy + accuracy, its gradient, and the pseudo-label rule.  Plain torch on the CPU:
F.interpolate(z.double(), size, 'bilinear', align_corners=False), F.cross_entropy(reduction='none') times the pixel weight, autograd for the
gradient, softmax -> max for the pseudo-labels, and the per-pixel bound maps the GPU test holds the kernels to (derived in its docstring).

A label outside [0, C) that is not ignore_index is no term of the loss and is counted (acc[3]); the weight of a pixel is the float32 product
pix_weight * class_weight[label] the kernels form, so the reference sums the same weights."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
LOSS_WEIGHT = 0.4
SHARE = 0.01          # condition on the inputs: at most this share of a case's pixels may fall under any one exclusion
MIN_VALID = 0.25      # and every image keeps at least this share of valid pixels

#        C   (h, w)     (H, W)    N
CASES = {
    'g_up':    (6, (13, 9), (50, 37), 3),        # non-integer ratios that differ per axis
    'g_c9':    (9, (13, 9), (50, 37), 3),        # two-pass forward, per-class backward
    'g_c33':   (33, (7, 11), (30, 41), 3),       # many classes
    'g_down':  (6, (20, 24), (11, 15), 3),       # down-sampling: the gather window of the backward kernels
    'g_same':  (3, (10, 12), (10, 12), 3),       # ratio 1: one tap of weight exactly 1
    'g_x2':    (6, (12, 10), (24, 20), 3),       # exact ratio 2
    'g_one':   (5, (1, 1), (5, 7), 3),           # every tap clamped
    'g_mixed': (6, (8, 6), (32, 48), 3),         # H == 4 h but W == 8 w
    'x4':      (6, (17, 16), (68, 64), 1),       # block kernels: crosses the 15-cell ownership edge and the 16-block tile edge
    'x8':      (8, (5, 17), (40, 136), 3),       # block kernels at the class limit
    'x4_c1':   (1, (4, 5), (16, 20), 3),         # one class
}
IGNORE_CASES = [(name, ign) for name in ('g_up', 'x4', 'x8') for ign in (2, 0)]
# pseudo-labels: the CE cases' logits, and two classes at g_up's shape
PSEUDO = {name: CASES[name] for name in ('g_up', 'g_down', 'g_x2', 'g_one', 'x4', 'g_c33', 'x4_c1')}
PSEUDO['p_c2'] = (2, (13, 9), (50, 37), 3)
THRESHOLDS = (0.9, 0.0, 1.5)
_SEED = {name: 100 + 10 * i for i, name in enumerate(list(CASES) + ['p_c2'])}


def g(seed):
    return torch.Generator().manual_seed(seed)


def shape_of(name):
    return CASES[name] if name in CASES else PSEUDO[name]


def is_pow2_ratio(lo, hi):
    """h / H and w / W both powers of two: source coordinates and weights are exact in float32"""
    def p2(a, b):
        big, small = max(a, b), min(a, b)
        return big % small == 0 and (big // small) & (big // small - 1) == 0
    return p2(lo[0], hi[0]) and p2(lo[1], hi[1])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(logits f32 [N,C,h,w], label u8 [N,H,W], pw f32 [N,H,W], cw f32 [C], old f32 [N,C,h,w])"""
    C, (h, w), (H, W), N = shape_of(name)
    s = _SEED[name]
    logits = torch.randn(N, C, h, w, generator=g(s)) * 3
    label = torch.randint(0, C, (N, H, W), generator=g(s + 1))
    label[:, H // 3:H // 3 + max(1, H // 5), W // 4:W // 4 + max(1, W // 3)] = 255          # a 255 region
    label[:, H - 1, :] = 255                                                                 # a run of 255 along one full border row
    if C < 255:                                                           # a handful of labels in [C, 255), none in [C, C + 8): the padded twins
        for n in range(N):
            pos = torch.randperm((H - 1) * W, generator=g(s + 2 + n))[:3]
            label[n].view(-1)[pos] = torch.tensor([C + 8, C + (254 - C) // 2, 254])
    return dict(logits=logits, label=label.to(torch.uint8), pw=torch.rand(N, H, W, generator=g(s + 6)) + 0.25,
                cw=torch.rand(C, generator=g(s + 7)) + 0.5, old=torch.randn(N, C, h, w, generator=g(s + 8)))


def scale_of(name):
    """the backward's scale as the float32 the C ABI receives"""
    C, lo, (H, W), N = shape_of(name)
    return float(np.float32(LOSS_WEIGHT / (N * H * W)))


def tol_z(name):
    """[N, 1, 1]: the bound on an interpolated logit, 2^-24 A (12 max(h, w) d + 4) (the resize bound of tests/test_plane_views_gpu.py)"""
    C, lo, hi, N = shape_of(name)
    A = inputs(name)['logits'].double().abs().amax((1, 2, 3)).view(N, 1, 1)
    d = 0 if is_pow2_ratio(lo, hi) else 1
    return U * A * (12 * max(lo) * d + 4)


def upsampled(logits, size, dtype=torch.float64):
    return F.interpolate(logits.to(dtype), size=tuple(size), mode='bilinear', align_corners=False)


def top2_gap(x):
    """[N, C, H, W] -> the gap between the two largest entries along dim 1 (inf with one class), the two classes"""
    if x.shape[1] == 1:
        z = torch.zeros(x.shape[0], *x.shape[2:], dtype=torch.long)
        return torch.full_like(x[:, 0], float('inf')), z, z
    v, i = x.topk(2, dim=1)
    return v[:, 0] - v[:, 1], i[:, 0], i[:, 1]


def _ce(name, weighted, ignore_index, dtype):
    C, lo, (H, W), N = shape_of(name)
    d = inputs(name)
    z = d['logits'].to(dtype).clone().requires_grad_()
    up = upsampled(z, (H, W), dtype)
    lab = d['label'].long()
    valid = (lab != ignore_index) & (lab < C)
    bad = (lab != ignore_index) & (lab >= C)
    idx = torch.where(valid, lab, torch.zeros_like(lab))
    nll = F.cross_entropy(up, idx, reduction='none')
    wp = (d['pw'] * d['cw'][idx]) if weighted else torch.ones(N, H, W)                      # float32 product, as the kernels form it
    wp = torch.where(valid, wp, torch.zeros_like(wp)).to(dtype)
    loss = (nll * wp).sum()
    (loss * scale_of(name)).backward()
    return dict(up=up.detach(), lse=torch.logsumexp(up.detach(), 1), nll=nll.detach(), wp=wp, loss=float(loss.detach()), grad=z.grad, valid=valid, bad=bad,
                lab=lab)


@functools.lru_cache(maxsize=None)
def reference(name, weighted, ignore_index=255):
    """the float64 reference of one CE launch and its bounds"""
    C, lo, (H, W), N = shape_of(name)
    r = _ce(name, weighted, ignore_index, torch.float64)
    tz = tol_z(name)
    gap, first, _ = top2_gap(r['up'])
    r['tol_z'] = tz
    r['tol_lse'] = tz + U * (2 * C + 8) + U * r['lse'].abs()
    r['tol_loss'] = float((r['wp'] * (r['tol_lse'] + tz + 2 * U * r['nll'].abs())).sum()) + U * abs(r['loss'])
    r['correct'] = int(((first == r['lab']) & r['valid']).sum())
    r['near_tie'] = r['valid'] & (gap < 2 * tz)                       # pixels whose arg-max an error of tol_z on two logits can turn
    r['n_valid'], r['n_bad'] = int(r['valid'].sum()), int(r['bad'].sum())
    r['prob'] = torch.softmax(r['up'], 1)
    return r


@functools.lru_cache(maxsize=None)
def torch32(name, weighted, ignore_index=255):
    """torch's own float32 CPU autograd on the same inputs: printed beside the kernels' ratios, for scale"""
    r = _ce(name, weighted, ignore_index, torch.float32)
    return dict(lse=r['lse'], loss=r['loss'], grad=r['grad'])


def grad_bound(ref_grad):
    """the per-link bound of DESIGN section 7, per element"""
    return 1e-4 * ref_grad.abs().max() + 1e-3 * ref_grad.abs()


def grad_bound_same(name, r):
    """ratio 1 (g_same): a cell receives one term of weight 1 -- |scale g| (p_c (tol_lse + 4u) + 2u |p_c - 1{l = c}|)"""
    C = shape_of(name)[0]
    onehot = F.one_hot(torch.where(r['valid'], r['lab'], torch.zeros_like(r['lab'])), C).permute(0, 3, 1, 2).double()
    sg = (scale_of(name) * r['wp']).abs().unsqueeze(1)
    return sg * (r['prob'] * (r['tol_lse'].unsqueeze(1) + 4 * U) + 2 * U * (r['prob'] - onehot).abs())


@functools.lru_cache(maxsize=None)
def pseudo_reference(name):
    """float64 softmax -> max of the resized logits, the top-2 probability gap and the two classes that may win inside it"""
    C, lo, hi, N = shape_of(name)
    p = torch.softmax(upsampled(inputs(name)['logits'], hi), 1)
    gap, first, second = top2_gap(p)
    tz = tol_z(name)
    return dict(pmax=p.amax(1), first=first, second=second, gap=gap, tol_p=tz + 4 * U, sure=gap > 2 * tz + 8 * U)


def padded_twin(name, extra):
    """the case's logits plus `extra` classes of constant logit -1e30 that are never labelled"""
    x = inputs(name)['logits']
    N, C, h, w = x.shape
    return torch.cat([x, torch.full((N, extra, h, w), -1e30)], 1).contiguous()
