"""Seeded inputs, case tables and float64 references of the kernel-level tests of csrc/spatial.hip (tests/test_spatial_edges_cpu.py,
tests/test_spatial_edges_gpu.py): the 3 x 3 / stride 2 / pad 1 max-pool and its adjoint, normalise-on-load, nearest up-sampling, channel_scale,
the element-wise kernels and the inference plane kernels (softmax, arg-max, flips, sliding-window sums).  Plain torch on the CPU, written from
the definitions; nothing here calls the project's kernels.

Max-pool: over the valid taps of a window the winner is the LAST NaN tap in row-major order if there is one (torch's `val > max || isnan(val)`
keeps replacing), else the FIRST maximal tap (found with an equality mask and a cumulative sum: argmax promises no tie order).
Arg-max over classes: the FIRST NaN class if there is one (torch.argmax), else the first maximal class."""
import functools

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126          # the smallest normal float32: below it a result has no relative accuracy (and may be flushed to zero)


def g(seed):
    return torch.Generator().manual_seed(seed)


def bits(t):
    """float32 values as int32 bit patterns, every NaN replaced by one pattern: +0 and -0 differ, NaNs are equal"""
    t = t.detach().float().cpu()
    return torch.where(torch.isnan(t), torch.full_like(t, 12345.0), t).contiguous().view(torch.int32)


def dyadic(shape, seed, step, bound):
    """multiples of `step` (a power of two) in [-bound, bound], float32"""
    k = int(round(bound / step))
    return torch.randint(-k, k + 1, shape, generator=g(seed)).float() * step


# ---------------------------------------------------------------------------------------------------------------------------- max-pool
POOL_SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (2, 4), (4, 4), (2, 8), (5, 8), (8, 6), (6, 12), (17, 22), (72, 72)]
PN, PC = 2, 3
# operand views of a launch: (name, floats x starts past a 16-byte boundary, floats y does, bytes idx does)
POOL_VIEWS = [('plain', 0, 0, 0), ('x + 4 B', 1, 0, 0), ('y + 4 B', 0, 1, 0), ('idx + 1 B', 0, 0, 1)]
BWD_VIEWS = [('plain', 0), ('dx + 4 B', 1)]
POOL_ROUTES = {'fwd pair', 'fwd generic', 'bwd 2x2', 'bwd generic'}
AXPY_ROUTES = {'axpy float4', 'axpy scalar'}


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def route_maxpool(H, W, x_ptr, y_ptr, idx_ptr):
    """pfst_maxpool3x3s2: two outputs per thread (16-byte loads of x, float2 / uchar2 stores) or one"""
    if W % 4 == 0 and H % 2 == 0 and x_ptr % 16 == 0 and y_ptr % 8 == 0 and idx_ptr % 2 == 0:
        return 'fwd pair'
    return 'fwd generic'


def route_maxpool_bwd(H, W, dx_ptr):
    """pfst_maxpool3x3s2_bwd: one thread per 2 x 2 input block (float2 stores) or one per input pixel"""
    return 'bwd 2x2' if H % 2 == 0 and W % 2 == 0 and dx_ptr % 8 == 0 else 'bwd generic'


def route_axpy(y_ptr, x_ptr):
    """axpy_kernel: float4 loop + scalar tail when both pointers are 16-byte aligned, else scalar"""
    return 'axpy float4' if (y_ptr | x_ptr) % 16 == 0 else 'axpy scalar'


def pool_eligible(H, W):
    """sizes at which the alignment of the operands decides the forward route"""
    return W % 4 == 0 and H % 2 == 0


def _taps(x):
    """-> (values [9, N, C, Ho, Wo], valid [9, 1, 1, Ho, Wo]) of the nine taps ty * 3 + tx of every window"""
    N, C, H, W = x.shape
    Ho, Wo = out_hw(H, W)
    xp = torch.zeros(N, C, H + 2, W + 2, dtype=x.dtype)
    ok = torch.zeros(1, 1, H + 2, W + 2, dtype=torch.bool)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    ok[:, :, 1:H + 1, 1:W + 1] = True
    vals, valid = [], []
    for ty in range(3):
        for tx in range(3):
            sl = (slice(None), slice(None), slice(ty, ty + 2 * Ho - 1, 2), slice(tx, tx + 2 * Wo - 1, 2))
            vals.append(xp[sl]), valid.append(ok[sl])
    return torch.stack(vals), torch.stack(valid)


def maxpool_ref(x):
    """-> (values float64 [N, C, Ho, Wo], taps int64): see the module docstring"""
    T, V = _taps(x.double())
    k = torch.arange(9).view(9, 1, 1, 1, 1)
    nan = torch.isnan(T) & V
    last_nan = torch.where(nan, k, torch.full_like(k, -1)).amax(0)
    Tm = torch.where(V & ~nan, T, torch.full_like(T, float('-inf')))
    eq = (Tm == Tm.amax(0, keepdim=True)) & V & ~nan
    first = eq & (eq.long().cumsum(0) == 1)
    first_max = (first.long() * k).sum(0)
    tap = torch.where(last_nan >= 0, last_nan, first_max)
    return T.gather(0, tap[None])[0], tap


def maxpool_bwd_ref(dy, idx, hw):
    """scatter-add in float64: dx[2 oy - 1 + ty][2 ox - 1 + tx] += dy[oy][ox] for the saved tap ty * 3 + tx of every window"""
    H, W = hw
    N, C, Ho, Wo = dy.shape
    dy, idx = dy.double(), idx.long()
    dxp = torch.zeros(N, C, H + 2, W + 2, dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):      # the windows of one tap land on distinct pixels: a slice add is a scatter-add
            dxp[:, :, ty:ty + 2 * Ho - 1:2, tx:tx + 2 * Wo - 1:2] += torch.where(idx == ty * 3 + tx, dy, torch.zeros_like(dy))
    assert float(dxp[:, :, 0].abs().sum() + dxp[:, :, H + 1].abs().sum() + dxp[:, :, :, 0].abs().sum() + dxp[:, :, :, W + 1].abs().sum()) == 0.0
    return dxp[:, :, 1:H + 1, 1:W + 1]


def bn_on_load_ref(x, coef):
    """max(fma(v, sc, sh), 0) per tap, coef [C, 4] = (mean, invstd, sc, sh): the product of two float32 values is exact in float64, so the
    float64 expression rounds once, as a fused multiply-add does"""
    sc, sh = coef[:, 2].double().view(1, -1, 1, 1), coef[:, 3].double().view(1, -1, 1, 1)
    return (x.double() * sc + sh).clamp_min(0.0)


NAN = float('nan')
INF = float('inf')


def has_interior(H, W):
    """window (1, 1) has nine valid taps: rows and columns 1 .. 3"""
    return H >= 4 and W >= 4


@functools.lru_cache(maxsize=None)
def pool_inputs(H, W):
    """-> {name: x [PN, PC, H, W]}, the input families of the forward test at one size"""
    shape = (PN, PC, H, W)
    rnd = torch.randn(shape, generator=g(7 + H * 100 + W))
    d = {'random': rnd.clone()}
    d['constant planes'] = torch.tensor([1.5, -2.0, 0.0, -0.0, 3.25, -1e-3]).view(PN, PC, 1, 1).expand(shape).clone()
    d['columns constant'] = torch.randn(PN, PC, 1, W, generator=g(8)).expand(shape).clone()          # ties between taps of different rows
    d['rows constant'] = torch.randn(PN, PC, H, 1, generator=g(9)).expand(shape).clone()
    d['three values'] = torch.randint(0, 3, shape, generator=g(10)).float()
    d['all -inf'] = torch.full(shape, -INF)
    x = rnd.clone()
    x[:, :, H // 2, W // 2] = INF
    x[:, 1, H - 1, W - 1] = INF
    d['+inf'] = x
    x = rnd.clone()
    x[:, :, 0, 0] = NAN
    x[:, 2, H - 1, W - 1] = NAN
    d['NaN in border windows'] = x
    x = rnd.clone()
    x[:, :, 0, 0] = NAN
    x[:, :, min(1, H - 1), min(1, W - 1)] = NAN
    if has_interior(H, W):
        x[:, :, 2, 1] = NAN
        x[:, :, 3, 3] = NAN
    d['two NaNs in a window'] = x
    if has_interior(H, W):
        for t in range(9):
            x = rnd.clone()
            x[:, :, 1 + t // 3, 1 + t % 3] = NAN
            d[f'NaN at tap {t} of window (1, 1)'] = x
    return d


@functools.lru_cache(maxsize=None)
def pool_case(H, W):
    """all families stacked along the batch axis -> dict(x, y, tap, names): one launch per size and view"""
    fam = pool_inputs(H, W)
    x = torch.cat(list(fam.values()))
    y, tap = maxpool_ref(x)
    return dict(x=x, y=y, tap=tap, names=list(fam))


BNL_COEFS = [[0.0, 0.25, -0.5], [1.0, -2.0, 2.0], [-0.25, 0.5, -1.0], [-0.0, -0.25, 0.5]]           # sc per channel; 0: every tap equal


@functools.lru_cache(maxsize=None)
def bnl_case(H, W):
    """x and sh multiples of 1/8 in [-4, 4], sc in +-{0, 1/4, 1/2, 1, 2}: v sc is a multiple of 1/32 below 8 and v sc + sh exact in float32
    and float64 alike -> dict(x [len(BNL_COEFS) PN, PC, H, W], coefs [(coef [PC, 4], y, tap)])"""
    x = dyadic((PN, PC, H, W), 21 + H * 100 + W, 0.125, 4.0)
    out = []
    for i, sc in enumerate(BNL_COEFS):
        coef = torch.zeros(PC, 4)
        coef[:, 0], coef[:, 1] = 77.0, -3.0          # mean and invstd are not read by the pool
        coef[:, 2] = torch.tensor(sc)
        coef[:, 3] = dyadic((PC,), 31 + i, 0.125, 4.0)
        out.append((coef,) + maxpool_ref(bn_on_load_ref(x, coef)))
    return dict(x=x, coefs=out)


# ------------------------------------------------------------------------------------------------------------------ nearest up-sampling
UPS_CASES = [((h, w), u) for (h, w) in ((1, 1), (3, 5), (7, 9)) for u in (1, 2, 3, 4, 8)] + [((33, 17), 4)]


def upsample_ref(x, u):
    return x.repeat_interleave(u, 2).repeat_interleave(u, 3)


def upsample_bwd_ref(dy, u):
    N, C, H, W = dy.shape
    return dy.double().view(N, C, H // u, u, W // u, u).sum((3, 5))


# ------------------------------------------------------------------------------------------------------------------ element-wise kernels
GRID_CAP = 2048 * 256            # threads of the largest element-wise grid (ew_grid): one pass
FILL_N = [1, 255, 257, GRID_CAP + 3]
AXPY_N = [1000, 1001, 1002, 1003, 4 * GRID_CAP + 7]
AXPY_VIEWS = [(0, 0), (0, 1), (1, 0), (1, 1)]          # floats past a 16-byte boundary: (y, x)
DIVISORS = [3.0, 7.0, 12.0, 0.1]
FLIP_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 9), (33, 47), (72, 72)]


def flip_ref(x, horizontal, vertical):
    dims = [d for d, on in ((3, horizontal), (2, vertical)) if on]
    return x.flip(dims) if dims else x.clone()


# ----------------------------------------------------------------------------------------------------------------------------- softmax
SM_C = [1, 2, 6, 19, 150]
SM_HW = [1, 3, 255, 1025]
SM_N = 2
SM_FAMILIES = ['randn', 'randn * 30', 'randn + 1e4', 'one class 120 below', '-inf classes']
# expf's own error in units of 2^-24 relative (2 units = 1 ulp).  Measured first: the worst excess of torch's float32 CPU softmax over
# (|z|max + C) 2^-24 on the inputs below (probabilities of at least 2^-100) is NEGATIVE, -0.14 units (C = 2, HW = 1025, randn): the |z| and C terms
# already cover all that this softmax shows, and twice a negative excess is no margin.  The value is therefore reasoned instead: expf enters a
# probability twice, in its numerator and through the sum in its denominator, and the HIP math API documents expf as within 1 ulp = 2 units: 4.
# With it torch's float32 softmax reaches 0.90 of the bound (C = 2, randn * 30, where |z| is about 64 and the rounded difference dominates).
U_EXP = 4.0
SM_VIEWS = {'slice': dict(), 'odd stride': dict(odd=1), 'lead': dict(lead=1)}


@functools.lru_cache(maxsize=None)
def softmax_inputs(C, HW, family):
    x = torch.randn(SM_N, C, HW, 1, generator=g(1000 + 10 * C + HW))
    if family == 'randn * 30':
        x = x * 30
    elif family == 'randn + 1e4':
        x = x + 1e4
    elif family == 'one class 120 below':
        x[:, C // 2] -= 120.0
    elif family == '-inf classes':          # every second class from 1 on, and never all of them
        x[:, 1::2] = -INF
    else:
        assert family == 'randn'
    return x


def softmax_reference(x):
    """-> dict(p float64, zmax [N, 1, HW, 1] the largest finite |x - max| of the pixel, bound: the relative bound per pixel)"""
    xd = x.double()
    z = xd - xd.amax(1, keepdim=True)
    zmax = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z)).amax(1, keepdim=True)
    return dict(p=torch.softmax(xd, 1), zmax=zmax, bound=(zmax + x.shape[1] + U_EXP) * U)


def softmax_ratio(got, ref):
    """the worst |got - p| / (bound p + TINY): a probability below the smallest normal float32 carries no relative accuracy"""
    err = (got.double() - ref['p']).abs()
    return float((err / (ref['bound'] * ref['p'] + TINY)).max())


@functools.lru_cache(maxsize=None)
def softmax_special(C, HW):
    """constructed rows: image 0, pixel 0 holds +inf in its last class; image 1, the last pixel is all -inf -> (x, rows [N, 1, HW, 1] bool)"""
    x = softmax_inputs(C, HW, 'randn').clone()
    rows = torch.zeros(SM_N, 1, HW, 1, dtype=torch.bool)
    x[0, C - 1, 0] = INF
    x[1, :, HW - 1] = -INF
    rows[0, 0, 0] = rows[1, 0, HW - 1] = True
    return x, rows


# ----------------------------------------------------------------------------------------------------------------------------- arg-max
AM_C = [1, 2, 19, 255]
AM_HW = [1, 3, 1025, 1028]          # 1028: the one size at which tta_finalize takes its 16-byte path
AM_N = 2
AM_FAMILIES = ['three values', 'all -inf', 'NaN classes', 'NaN after +inf']


def argmax_ref(x):
    """over dim 1: the first NaN class if any, else the first maximal class"""
    k = torch.arange(x.shape[1]).view(1, -1, *([1] * (x.dim() - 2)))
    nan = torch.isnan(x)
    first_nan = (nan & (nan.long().cumsum(1) == 1)).long().mul(k).sum(1)
    xm = torch.where(nan, torch.full_like(x, -INF), x)
    eq = xm == xm.amax(1, keepdim=True)
    first_max = (eq & (eq.long().cumsum(1) == 1)).long().mul(k).sum(1)
    return torch.where(nan.any(1), first_nan, first_max)


@functools.lru_cache(maxsize=None)
def argmax_inputs(C, HW, family):
    shape = (AM_N, C, HW, 1)
    gen = g(2000 + 10 * C + HW)
    if family == 'three values':
        return torch.randint(0, 3, shape, generator=gen).float() / 3
    if family == 'all -inf':
        return torch.full(shape, -INF)
    x = torch.randn(shape, generator=gen)
    p = torch.arange(HW)
    if family == 'NaN classes':          # two NaNs per pixel, the first anywhere from class 0 to C - 1: the lower index wins
        x[0, p % C, p, 0] = NAN
        x[0, (p * 7 + 3) % C, p, 0] = NAN
        x[1, (C - 1 - p) % C, p, 0] = NAN
        return x
    assert family == 'NaN after +inf'
    x[:, 0] = INF
    x[:, C - 1] = NAN
    if C > 2:
        x[:, C // 2] = NAN
    return x


@functools.lru_cache(maxsize=None)
def pair_ties(C):
    """one pixel per pair of classes i < j, both at the maximum over distinct descending values (the last pair repeated up to a multiple
    of four pixels) -> (x [1, C, P, 1], winner [P])"""
    pairs = [(i, j) for i in range(C) for j in range(i + 1, C)] or [(0, 0)]
    pairs += [pairs[-1]] * (-len(pairs) % 4)
    i, j = torch.tensor(pairs).t()
    P = len(pairs)
    x = (-1.0 - torch.arange(C, dtype=torch.float32)).view(1, C, 1, 1).repeat(1, 1, P, 1)
    x[0, i, torch.arange(P), 0] = 6.0
    x[0, j, torch.arange(P), 0] = 6.0
    return x, i


# ------------------------------------------------------------------------------------------------------------------- sliding windows
WIN_N = 2
WIN_C = [1, 19]
CANVASES = [(37, 41), (72, 72)]


def windows(H, W):
    """(y1, x1, hc, wc) in call order; the LAST is the full image, the ones before it leave pixels uncovered"""
    hc, wc = 16, 20
    return [(0, 0, hc, wc), (0, W - wc, hc, wc), (H - hc, 0, hc, wc), (H - hc, W - wc, hc, wc),          # the four corners
            (H - 1, W - 1, 1, 1),                                                                    # one pixel, bottom right
            (2, 3, 33, 32),                                                                          # more than 1024 pixels
            (5, 7, hc, wc), (5, 7, hc, wc), (9, 12, hc, wc), (5, 7, hc, wc),                            # repeated, overlapping
            (0, 0, H, W)]


def refused_windows(H, W):
    return [(-1, 0, 4, 4), (0, -1, 4, 4), (H - 3, 0, 4, 4), (0, W - 3, 4, 4), (0, 0, H + 1, 4), (0, 0, 4, W + 1)]


@functools.lru_cache(maxsize=None)
def window_case(H, W, C):
    """-> dict(crops, preds / count after every call (float32 slice adds on the CPU in call order), uncovered: a pixel no window but the last covers)"""
    preds, count = torch.zeros(WIN_N, C, H, W), torch.zeros(WIN_N, 1, H, W)
    crops, steps = [], []
    for i, (y1, x1, hc, wc) in enumerate(windows(H, W)):
        crop = torch.randn(WIN_N, C, hc, wc, generator=g(3000 + i)) * 3
        preds[:, :, y1:y1 + hc, x1:x1 + wc] += crop
        count[:, :, y1:y1 + hc, x1:x1 + wc] += 1
        crops.append(crop), steps.append((preds.clone(), count.clone()))
    return dict(crops=crops, steps=steps)
