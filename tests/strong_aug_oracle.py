"""Float64 references, seeded inputs and bounds of the strong-augmentation tests (tests/test_strong_aug_cpu.py, test_strong_aug_edges_gpu.py,
test_strong_aug_step_gpu.py).  Plain torch / NumPy on the CPU, restated from the comments of csrc/strong_aug.hip and from
rsiseg/models/utils/dacs_transforms.py:44-107:

  jitter   per image: (x std + mean) / 255, the four ops in the image's order -- brightness x + b - 1, contrast x c (both clamped to [0, 1]),
           saturation s <- clamp(s f) and hue h <- (h + dh) mod 2 pi in HSV (rgb_to_hsv with s = d / (max + 1e-8) and torch.max's first-max
           rule, hsv_to_rgb by sector table; no clamp of the RGB result) -- then (x 255 - mean) / std.  2 pi is math.pi's, not the kernel's
           fp32 constant: the difference (2.8e-8 relative) is part of the error the bound counts.
  blur     a separable filter, x pass then y pass, over ALL taps; reflect-without-edge-repeat indices from a table (any K / 2, also >= n).
  draws    the host draws of pfst_amd.strong_aug.apply_strong_aug, replayed from a snapshot of the generator states.

`wrong=` selects a deliberately wrong variant: the CPU test shows that each one moves the GPU tests' inputs by more than ten times their bound.
The same jitter code runs in float32 (dtype=torch.float32): the CPU statement of what fp32 rounding alone does to these formulas."""
import functools
import itertools
import math

import numpy as np
import torch

U = 2.0 ** -24
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)
TWO_PI = 2.0 * math.pi

# ------------------------------------------------------------------------------------------------------------------------------ colour jitter
# K_JITTER: the fp32 roundings of the longest chain (an order with both HSV steps), one 2^-24 of a quantity <= 1 each:
#   de-normalise 3 (x std, + mean, / 255), brightness 2, contrast 1, re-normalise 3 (x 255, - mean, / std: values up to 255, so 2^-24 255 / std)
#   rgb_to_hsv 10 (d; max + 1e-8; s; max - c; hh; + 2 d or 4 d; / d; / 6; - floor; x 2 pi)      hsv_to_rgb 6 (/ 2 pi; x 6; 1 - f; f s; 1 - f s; x v)
#   saturation step 10 + 1 (s f) + 6 = 17, hue step 10 + 2 (h + dh; + 2 pi after fmod) + 6 = 18                   -> 3 + 2 + 1 + 17 + 18 + 3 = 44
# The eight roundings of an angle (x 2 pi, + dh, + 2 pi, / 2 pi, x 6: three in the saturation step, five in the hue step) are of quantities up
# to 2 pi resp. 6 and reach the result through f with slope 6 v s / (2 pi) per radian: each weighs up to 6 at h -> 2 pi, 3 in the mean over
# the hue circle; they are independent, so the mean weight is counted: + 8 (3 - 1) = 16.  The oracle's exact 2 pi against the kernel's fp32
# constant moves dh / (2 pi) by 2.8e-8 x 0.5 turns, x 6 in f: 1.4 units, counted as 2.  K_JITTER = 44 + 16 + 2 + 2 spare = 64.
# A contrast factor c > 1 multiplies a value AND the absolute error it carries (the errors of 1 - f s and max - c do not shrink with the
# value), a saturation factor likewise the chroma's: the bound of an image is K_JITTER 2^-24 max(1, c) max(1, f), from its parameter row.
# The count is checked, not fitted: test_strong_aug_cpu.py holds this module's own float32 evaluation to HALF the bound.
K_JITTER = 64
# a black pixel de-normalises to a residue, not to 0: |c| <= RHO in either arithmetic (the rounding of (0 - mean) / std, and without FMA
# contraction the rounding of the product); there s = d / (max + 1e-8) is of order 1 or more and differs between arithmetics
RHO = 2 * U * max(MEAN) / 255.0
BLACK = 1e-6          # an HSV step whose fp64 |max + 1e-8| is below this gets the absolute term
BLACK_S_MAX = 16.0    # condition on the inputs: |s| of the reference at such pixels (the residues must not sit ON the singularity)

ORDERS = [list(p) for p in itertools.permutations(range(4))]
#              brightness contrast saturation hue
PARAM_SETS = {
    'hi':    (1.2, 1.2, 1.2, 0.2 * TWO_PI),        # the shipped extremes (color_jitter_strength 0.2)
    'lo':    (0.8, 0.8, 0.8, -0.2 * TWO_PI),
    'sat0':  (1.1, 0.9, 0.0, -math.pi),            # factors 0 and 2 and hue +-pi: a dict-valued jitter_s of 1.0 (hue 0.5)
    'sat2':  (0.9, 1.1, 2.0, math.pi),
    'con2':  (0.7, 2.0, 1.0, 1.0),
    'con0':  (1.3, 0.0, 1.5, -2.0),
    'bri0':  (0.0, 1.5, 0.5, 0.5),
    'bri2':  (2.0, 0.5, 1.5, -0.5),
    'ident': (1.0, 1.0, 1.0, 0.0),
}
#            (h, w)
JITTER_PLANES = [(1, 1), (3, 5), (31, 33), (25, 41)]      # HW = 1, 15, 1023 (one short of four blocks' worth), 1025
JITTER_BIG = (1450, 1450)                                 # cdiv(HW, 1024) = 2054 > 2048: the capped grid's stride loop runs

_GREYS = [(v, v, v) for v in range(0, 256, 17)]
PLANTED = ([(0, 0, 0)] * 2 + [(255, 255, 255)] * 2 + _GREYS
           + [(200, 200, 50), (1, 1, 0), (255, 255, 0), (30, 180, 180), (0, 255, 255), (0, 7, 7)]            # r == g > b, g == b > r
           + [(90, 200, 90), (200, 90, 200), (0, 255, 0), (255, 0, 255), (128, 0, 128)]                      # r == b, below and above g
           + [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]            # primaries and secondaries
           + [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (255, 254, 255), (254, 255, 254), (255, 0, 1)])    # value 1 next to 0, 255 next to 254


def params_for(name, n=24):
    """[n, 8] float32: parameter set `name` with the 24 op orders as the rows (image i: order i mod 24)"""
    b, c, s, h = PARAM_SETS[name]
    return torch.tensor([[b, c, s, h] + [float(o) for o in ORDERS[i % 24]] for i in range(n)], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def jitter_pixels(n, h, w, seed=0):
    """uint8 pixel values [n, 3, h, w]: random, with the PLANTED pixels written from the front of each plane (image i starts the list at
    7 i, so that planes too small for the list cover it across the batch)"""
    g = torch.Generator().manual_seed(1000 + seed)
    p = torch.randint(0, 256, (n, 3, h * w), generator=g)
    pl = torch.tensor(PLANTED).t()                                   # [3, P]
    for i in range(n):
        m = min(h * w, pl.shape[1])
        p[i, :, :m] = pl.roll(-7 * i, 1)[:, :m]
    return p.view(n, 3, h, w)


def normalise(p):
    """as the loader: (p - mean) / std in float32"""
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    return (p.float() - mean) / std


def jitter_input(n, h, w, denorm, seed=0):
    """float32 [n, 3, h, w]: the normalised image (denorm) or the image in [0, 1]"""
    p = jitter_pixels(n, h, w, seed)
    return normalise(p) if denorm else p.float() / 255.0


@functools.lru_cache(maxsize=None)
def out_of_gamut_input(n=8, h=9, w=11):
    """normalised float32 [n, 3, h, w] whose de-normalised channels lie in [-0.5, 1.5] with each pixel's largest channel >= 0.05"""
    g = torch.Generator().manual_seed(77)
    x = torch.rand(n, 3, h, w, generator=g, dtype=torch.float64) * 2.0 - 0.5
    top = x.amax(1, keepdim=True)
    x = torch.where((top < 0.06) & (x == top), torch.full_like(x, 0.06) + 0.5 * x.abs(), x)
    mean, std = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return ((x * 255.0 - mean) / std).float()


def out_of_gamut_params(n=8):
    """orders that begin with op 2 and with op 3 (the first op sees the raw de-normalised image), shipped-range parameters"""
    first = [o for o in ORDERS if o[0] in (2, 3)]
    sets = [PARAM_SETS['hi'], PARAM_SETS['lo']]
    return torch.tensor([list(sets[i % 2]) + [float(v) for v in first[(5 * i) % len(first)]] for i in range(n)], dtype=torch.float32)


SECTORS = ('vtp', 'qvp', 'pvt', 'pqv', 'tpv', 'vpq')


def rgb_to_hsv(r, g, b):
    mx, mn = torch.maximum(r, torch.maximum(g, b)), torch.minimum(r, torch.minimum(g, b))
    d = mx - mn
    s = d / (mx + 1e-8)
    d = torch.where(d == 0, torch.ones_like(d), d)
    rc, gc, bc = mx - r, mx - g, mx - b
    hh = torch.where((r >= g) & (r >= b), bc - gc, torch.where(g >= b, (rc - bc) + 2 * d, (gc - rc) + 4 * d))       # the first maximum wins
    hh = hh / d / 6
    hh = hh - torch.floor(hh)
    return TWO_PI * hh, s, mx


def hsv_to_rgb(h, s, v, sectors=SECTORS):
    h6 = h / TWO_PI * 6
    fl = torch.floor(h6)
    hi = torch.remainder(fl, 6).long()
    f = h6 - fl
    val = dict(v=v, p=v * (1 - s), q=v * (1 - f * s), t=v * (1 - (1 - f) * s))
    table = torch.stack([torch.stack([val[ch] for ch in row]) for row in sectors])          # [6, 3, ...]
    return table.gather(0, hi.expand(1, 3, *hi.shape))[0]


def jitter_ex(img, params, mean=MEAN, std=STD, denorm=True, dtype=torch.float64, wrong=None):
    """-> (result [n, 3, h, w] in `dtype`, allow [n, h, w]: the absolute term of the bound in unit scale (0 off the black pixels),
    smax [n, h, w]: the largest |s| any HSV step of the pixel saw).  params: the float32 [n, 8] rows the kernel receives."""
    n = img.shape[0]
    mean_t, std_t = torch.tensor(mean, dtype=dtype).view(3, 1, 1), torch.tensor(std, dtype=dtype).view(3, 1, 1)
    if wrong == 'std_swap':
        std_t = std_t[[0, 2, 1]]
    if wrong == 'next_params':
        params = params.roll(-1, 0)
    sectors = SECTORS[:4] + (SECTORS[5], SECTORS[4]) if wrong == 'sector_swap' else SECTORS
    out, allow, smax = [], [], []
    for i in range(n):
        x = img[i].to(dtype)
        if denorm:
            x = (x * std_t + mean_t) / 255.0
        bf, cf, sf, hf = [float(v) for v in params[i, :4]]
        order = [int(v) for v in params[i, 4:]]
        if wrong == 'order_shift':
            order = order[1:] + order[:1]
        al, sm = torch.zeros(x.shape[1:], dtype=torch.float64), torch.zeros(x.shape[1:], dtype=torch.float64)
        for op in order:
            if op == 0:
                x = (x + bf - 1).clamp(0, 1)
            elif op == 1:
                x = (x * cf).clamp(0, 1)
            else:
                h, s, v = rgb_to_hsv(x[0], x[1], x[2])
                black = ((v + 1e-8).abs() < BLACK).double()
                al = torch.maximum(al, black * 4.0 * (1.5 * RHO + v.abs().clamp(max=RHO).double() * (1 + s.abs().double())))
                sm = torch.maximum(sm, s.abs().double())
                if op == 2:
                    s = s * sf
                    if wrong != 'no_sat_clamp':
                        s = s.clamp(0, 1)
                else:
                    h = torch.remainder(h + (-hf if wrong == 'hue_sign' else hf), TWO_PI)
                x = hsv_to_rgb(h, s, v, sectors)
        if denorm:
            x = (x * 255.0 - mean_t) / std_t
        out.append(x), allow.append(al), smax.append(sm)
    return torch.stack(out), torch.stack(allow), torch.stack(smax)


def jitter(img, params, mean=MEAN, std=STD, denorm=True):
    return jitter_ex(img, params, mean, std, denorm)[0]


def jitter_bound(allow, params, std=STD, denorm=True, smax=None):
    """[n, 3, h, w]: K_JITTER 2^-24 255 / std_c (unit scale without denorm) times the image's max(1, contrast) max(1, saturation factor),
    times max(1, |s|) where `smax` is given (out of gamut), plus the
    black pixels' absolute term.  The absolute term, in unit scale: at a pixel whose channels are residues |c| <= RHO an HSV step returns
    v (1 - s phi), phi in [0, 1], so |result| <= |v| (1 + |s|) in either arithmetic.  The reference's own value of that, plus what fp32
    without FMA can return -- there the residues are multiples of q = 2^-17 / 255 = 0.52 RHO inside +-RHO, i.e. -q, 0 or q, so max = q at
    most, s <= 2 q / (q + 1e-8) = 1.5 and |result| <= 2.5 q < 1.5 RHO -- bounds the difference; x 4 for a later contrast and saturation
    factor of 2 each.  With |v| ~ 4e-9 and |s| ~ 2..5 on these inputs: 4 (8.7e-8 + 2.4e-8) = 4.4e-7."""
    scale = (255.0 / torch.tensor(std, dtype=torch.float64) if denorm else torch.ones(3, dtype=torch.float64)).view(1, 3, 1, 1)
    gain = (params[:, 1].double().clamp(min=1.0) * params[:, 2].double().clamp(min=1.0)).view(-1, 1, 1)
    rel = K_JITTER * U * gain * (torch.ones_like(allow) if smax is None else smax.clamp(min=1.0))
    return (rel + allow).unsqueeze(1) * scale


def jitter_ratio(got, img, params, denorm=True, out_of_gamut=False):
    """-> (the largest |got - reference| / bound over EVERY element, the reference, the bound)"""
    ref, allow, smax = jitter_ex(img, params, MEAN, STD, denorm)
    bound = jitter_bound(allow, params, STD, denorm, smax if out_of_gamut else None)
    return float(((got.double().cpu() - ref).abs() / bound).max()), ref, bound


JITTER_WRONG = ('hue_sign', 'no_sat_clamp', 'order_shift', 'std_swap', 'next_params', 'sector_swap')


# ------------------------------------------------------------------------------------------------------------------------------ gaussian blur
def reflect_table(n, K, wrong=None):
    """int64 [n, K]: the source index of tap t at position i, torch's 'reflect' (no edge repeat), any number of periods"""
    i = np.arange(n)[:, None] + np.arange(K)[None, :] - K // 2 + (1 if wrong == 'shift' else 0)
    if wrong == 'edge_repeat':                       # 'symmetric': ... 1 0 | 0 1 2 ...
        period = 2 * n
        i = np.mod(i, period)
        return torch.from_numpy(np.where(i < n, i, period - 1 - i))
    if n == 1:
        return torch.zeros(1, K, dtype=torch.int64)
    period = 2 * (n - 1)
    i = np.mod(i, period)
    return torch.from_numpy(np.where(i < n, i, period - i))


def _blur_pass(x, taps, axis, reach=None, wrong=None):
    n, K = taps.shape
    idx = reflect_table(x.shape[axis], K, wrong)
    lo, hi = (0, K - 1) if reach is None else (max(0, K // 2 - reach), min(K - 1, K // 2 + reach))
    out = torch.zeros_like(x)
    for t in range(lo, hi + 1):
        out += taps[:, t].view(n, 1, 1, 1) * x.index_select(axis, idx[:, t])
    return out


def blur(img, taps_y, taps_x, wrong=None, reach=None):
    """img [n, C, H, W]; taps_y [n, Ky], taps_x [n, Kx]: the float32 taps the kernel receives -> float64 [n, C, H, W]"""
    x, ty, tx = img.double(), taps_y.double(), taps_x.double()
    if wrong == 'next_taps':
        ty, tx = ty.roll(-1, 0), tx.roll(-1, 0)
    if wrong == 'swap_xy':
        ty, tx = tx, ty
    w = wrong if wrong in ('shift', 'edge_repeat') else None
    return _blur_pass(_blur_pass(x, tx, 3, reach, w), ty, 2, reach, w)


def looped(K, reach):
    return min(K - 1, K // 2 + reach) - max(0, K // 2 - reach) + 1


def blur_bound(img, Ky, Kx, reach):
    """[n, C, 1, 1]: 2^-24 A (nx + ny + 2), A = max |x| of the plane, nx and ny the taps looped: each fmaf rounds a partial sum <= A (the
    weights are positive and sum to 1), the second pass carries the first pass's error through unit-sum weights; + 2 for the weights' sum
    being 1 only to 2^-22 and the dropped taps (< 2^-60 A)"""
    A = img.double().abs().amax((2, 3), keepdim=True)
    return U * A * (looped(Kx, reach) + looped(Ky, reach) + 2)


def gauss_taps64(k, sigma):
    x = np.arange(k, dtype=np.float64) - k // 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def taps_for(k, sigmas):
    from pfst_amd.strong_aug import _gauss_taps
    return torch.stack([_gauss_taps(k, s) for s in sigmas])


def host_reach(sigmas):
    return int(math.ceil(max(sigmas) * 10.0)) + 1


def _explicit_taps(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, K, generator=g) + 0.1
    return t / t.sum(1, keepdim=True)


#                 (H, W)       sigmas or None          reach
BLUR_CASES = {
    'truncated':  ((90, 130), (0.15, 0.15), 3),                  # K = 9, 13: 7 of 9 and 7 of 13 taps looped, as production truncates
    'shared':     ((290, 310), (0.15, 1.15), 13),                # K = 29, 31: K / 2 = 14, 15 > 13, the reach the larger sigma sets
    'full':       ((96, 128), (0.4, 1.1), 13),                   # K = 9, 13 untruncated (the case of test_strong_aug_gpu.py)
    'centre':     ((20, 30), (0.6, 1.0), 0),                     # K = 1, 3 -- reach 0: the centre tap only
    'k1':         ((7, 9), None, 13),                            # K = 1 both ways
    'k1_row':     ((1, 5), None, 13),
    'tail_1023':  ((33, 31), (1.0, 0.7), 13),                    # K = 3, 3
    'tail_1025':  ((41, 25), (1.0, 0.7), 13),                    # K = 5, 3
    'periods':    ((3, 4), 'explicit9', 13),                     # K = 9 >= 2 n: the reflection wraps more than once
    'one_row':    ((1, 6), 'explicit5', 13),                     # n = 1 along y with K = 5
    'per_image':  ((50, 70), (0.2, 0.6, 1.15), 13),              # K = 5, 7, three images
}


@functools.lru_cache(maxsize=None)
def blur_case(name):
    """-> (img float32 [n, 3, H, W], taps_y, taps_x, reach)"""
    from pfst_amd.strong_aug import _blur_kernel_size
    (H, W), sig, reach = BLUR_CASES[name]
    n = len(sig) if isinstance(sig, tuple) else 2
    g = torch.Generator().manual_seed(500 + list(BLUR_CASES).index(name))
    img = torch.randn(n, 3, H, W, generator=g)
    if sig is None:
        ty = tx = torch.ones(n, 1)
    elif sig == 'explicit9':
        ty, tx = _explicit_taps(n, 9, 1), _explicit_taps(n, 9, 2)
    elif sig == 'explicit5':
        ty, tx = _explicit_taps(n, 5, 3), _explicit_taps(n, 5, 4)
    else:
        ky, kx = _blur_kernel_size(H), _blur_kernel_size(W)
        if name in ('k1', 'k1_row'):
            assert (ky, kx) == (1, 1)
        ty, tx = taps_for(ky, sig), taps_for(kx, sig)
    return img, ty, tx, reach


BLUR_WRONG = ('edge_repeat', 'shift', 'short_reach', 'next_taps', 'swap_xy')


# ------------------------------------------------------------------------------------------------------------------------------ host draws
def draw_params(n, s, torch_state, end_state=False):
    """the [n, 8] float32 parameter rows apply_strong_aug draws from torch's CPU generator in state `torch_state`: per image four uniform_
    draws (brightness, contrast, saturation around 1 and floored at 0, hue in +-s turns) and one randperm(4); end_state: also the state the
    generator is left in"""
    g = torch.Generator()
    g.set_state(torch_state)
    s = s if isinstance(s, dict) else dict(brightness=s, contrast=s, saturation=s, hue=s)
    rows = []
    for _ in range(n):
        vals = [torch.empty(1).uniform_(max(0.0, 1 - s[k]), 1 + s[k], generator=g) for k in ('brightness', 'contrast', 'saturation')]
        vals.append(torch.empty(1).uniform_(-s['hue'], s['hue'], generator=g) * 2 * math.pi)
        rows.append(torch.cat(vals + [torch.randperm(4, generator=g).float()]))
    return (torch.stack(rows), g.get_state()) if end_state else torch.stack(rows)


def draw_sigmas(n, numpy_state, end_state=False):
    """-> (the n sigmas np.random.uniform(0.15, 1.15) gives from `numpy_state`, the reach the largest one sets[, the state left behind])"""
    rs = np.random.RandomState()
    rs.set_state(numpy_state)
    sig = [rs.uniform(0.15, 1.15) for _ in range(n)]
    return (sig, host_reach(sig), rs.get_state()) if end_state else (sig, host_reach(sig))


def strong_aug(img, metas, jitter_s, torch_state, numpy_state, denorm=True):
    """apply_strong_aug with both transforms drawn, in float64 -> (result, per-element bound [n, 3, 1, 1]): the jitter bound's largest value
    per channel passes the blur unchanged (unit-sum weights), the blur adds its own"""
    from pfst_amd.strong_aug import _blur_kernel_size
    n, _, h, w = img.shape
    cfg = metas[0]['img_norm_cfg']
    out = img
    bound = torch.zeros(n, 3, 1, 1, dtype=torch.float64)
    if torch_state is not None:
        prm = draw_params(n, jitter_s, torch_state)
        out, allow, _ = jitter_ex(img, prm, cfg['mean'], cfg['std'], denorm)
        bound = jitter_bound(allow, prm, cfg['std'], denorm).amax((2, 3), keepdim=True)
    if numpy_state is not None:
        sig, reach = draw_sigmas(n, numpy_state)
        ky, kx = _blur_kernel_size(h), _blur_kernel_size(w)
        ty, tx = taps_for(ky, sig), taps_for(kx, sig)
        bound = bound + blur_bound(out, ky, kx, reach)
        out = blur(out, ty, tx)
    return out.double(), bound
