"""The kernels of csrc/spatial.hip that the inference tests are anchored on, and the pooling / nearest-resize / element-wise kernels beside them,
against the float64 references of tests/spatial_oracle.py: maxpool (both forward kernels, normalise-on-load, the published maximum) and
maxpool_bwd (both kernels), upsample_nearest / _bwd, channel_scale, fill_, axpy_, to_u8 / to_i64, div_scalar_, flip_planes, softmax_nchw,
argmax_nchw / tta_finalize (and scene_tta_finalize's NaN rule), window_accumulate_ / window_normalize_.

Every output is written into a canary buffer (helpers.Guard for float planes, Pad below for bytes and int64), inputs must come back unchanged.
The host's choices (pfst_maxpool3x3s2, pfst_maxpool3x3s2_bwd, axpy_kernel's branch) are restated in spatial_oracle.route_*; every launch asserts
the route its operands meet and test_every_route_is_reached asserts that the operands of this file reach all of them.

What is compared how (u = 2^-24):
  selections and copies (max-pool values and taps, up-sampling, flips, conversions, fill, arg-max) bit for bit: int32 patterns, NaNs as one.
  sums on dyadic grids (max-pool backward, nearest backward, axpy_) bit for bit: every partial sum is exact, so the order cannot matter.
  max-pool backward, random dy   3 u sum |terms| per pixel: three roundings of a sum of at most four terms.
  nearest backward, random dy    (f^2 - 1) u sum |terms| per pixel for the factor f.
  axpy_, random                  u |ref|: one rounding of the fused multiply-add.
  channel_scale, div_scalar_, window sums and window_normalize_: bit-equal to the same float32 operation on the CPU (one IEEE rounding each).
  softmax_nchw  |p - ref| <= (|z|max + C + 4) u ref + 2^-126 (spatial_oracle.U_EXP = 4 says where the 4 comes from; the last term: a value
                below the smallest normal float32 has no relative accuracy), rows sum to 1 within C u, classes at -inf or 120 below the rest are
                exactly 0, rows holding +inf or only -inf are NaN exactly where torch's float32 softmax is.

Worst measured ratio to each bound, MI355X (pytest -s prints them):
  maxpool_bwd            0.595 (2 x 2 blocks), 0.600 (one pixel per thread)
  upsample_nearest_bwd   0 (x1, exact), 0.683 (x2), 0.229 (x3), 0.232 (x4), 0.028 (x8)
  axpy_                  0.999 on both branches, 0.998 with x is y: the bound is the rounding of the result itself
  softmax_nchw           randn 0.48, randn * 30 0.911, randn + 1e4 0.301, one class 120 below 0.058, -inf classes 0.342, the rows beside the
                         constructed NaN rows 0.48; row sums 0.719 of C u.  torch's float32 CPU softmax on the same inputs: 0.904 at the worst
                         (randn * 30, C = 2: |z| is about 64 there and the rounding of x - max, multiplied by |z| inside exp, is the whole error).
Mutations each caught (on scratch builds of the library): `>=` in maxpool_kernel (test_maxpool_forward at every size above 1 x 1, normalise-on-load,
backward) or in maxpool_pair_kernel (the five pair-eligible sizes of the same tests); the pair kernel without its `k == 0` column guard (the same
five sizes: column 0 wins as tap 0 instead of tap 1); axpy_kernel's tail starting one element late (test_axpy at n = 1001, 1002, 1003 and
2097159); softmax_nchw_kernel without the max subtraction or with x_bs as the output's batch stride (all twenty test_softmax cases); the arg-max
walks without the NaN clause (test_argmax_and_tta_finalize at every C > 1; the 16-byte path of tta_finalize alone: the three HW = 1028 cases).
"""
import numpy as np
import pytest
import torch

import spatial_oracle as O
from helpers import Guard, note, report
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = O.U
FILL = {torch.uint8: 0xA5, torch.int64: -7777}


class Pad:
    """`numel` dense elements of `dtype` (uint8, int64), `lead` elements past a 16-byte boundary, between two runs of 64 canary elements"""

    def __init__(self, numel, dtype, lead=0):
        self.lo, self.n = 64 + lead, numel
        self.flat = torch.full((64 + lead + numel + 64,), FILL[dtype], dtype=dtype, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[self.lo:self.lo + numel]

    def ptr(self):
        return self.view.data_ptr()

    def intact(self, what=''):
        out = torch.cat([self.flat[:self.lo], self.flat[self.lo + self.n:]])
        assert bool((out == FILL[self.flat.dtype]).all()), f'{what}: elements outside the {self.flat.dtype} buffer were written'


def planes(nc, h, w, lead=0, src=None):
    """nc dense float planes inside canaries (one plane in front, three behind), `lead` floats past a 16-byte boundary"""
    gd = Guard((1, nc, h, w), lead=lead)
    if src is not None:
        gd.put(src.reshape(1, nc, h, w).to(DEV))
    return gd


def flat(n, lead=0, src=None):
    """n floats inside canaries; lead = 0: 16-byte aligned"""
    gd = Guard((1, 1, 1, n), front=4, back=1, lead=lead)
    assert gd.view.data_ptr() % 16 == 4 * lead
    if src is not None:
        gd.put(src.reshape(1, 1, 1, n).to(DEV))
    return gd


def dbits(t):
    """a device float tensor as int32 patterns (NaN payloads and the sign of zero count)"""
    return t.contiguous().view(torch.int32)


def same_bits(got, ref, what, names=None, per=1):
    """got (device) and ref (CPU, float64 or float32 holding float32 values) agree bit for bit, NaNs as one; names: the family of a batch index"""
    a, b = O.bits(got), O.bits(ref)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = (a != b).nonzero()
        k = int(bad[0, 0])
        where = f' (family {names[k // per]!r})' if names else ''
        at = tuple(bad[0].tolist())
        raise AssertionError(f'{what}: {bad.shape[0]} of {a.numel()} values differ, the first at {list(at)}{where}: '
                             f'{float(got.detach().cpu()[at])!r} against {float(ref[at])!r}')


def worst(err, bound):
    """the largest ratio of an error to its bound (a bound of 0 admits an error of 0 only)"""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(ratio.max())


def refused(ops):
    from pfst_amd._lib import PfstHipError
    return pytest.raises(PfstHipError)


# ------------------------------------------------------------------------------------------------------------------------ max-pool forward
def pool_operands(shape, view):
    """canary buffers of one forward launch and the kernel the host will choose for them"""
    _, dx, dy, di = view
    n, c, H, W = shape
    Ho, Wo = O.out_hw(H, W)
    xg, yg, ig = planes(n * c, H, W, lead=dx), planes(n * c, Ho, Wo, lead=dy), Pad(n * c * Ho * Wo, torch.uint8, lead=di)
    if O.pool_eligible(H, W):          # the views misalign by what they say, and nothing else does
        assert (xg.view.data_ptr() % 16, yg.view.data_ptr() % 8, ig.ptr() % 2) == (4 * dx, 4 * dy, di)
    return xg, yg, ig, O.route_maxpool(H, W, xg.view.data_ptr(), yg.view.data_ptr(), ig.ptr())


def run_pool(ops, x, view, coef=None, amax=None):
    n, c, H, W = x.shape
    Ho, Wo = O.out_hw(H, W)
    xg, yg, ig, route = pool_operands(x.shape, view)
    assert route == ('fwd pair' if O.pool_eligible(H, W) and view[0] == 'plain' else 'fwd generic')
    xd = x.to(DEV)
    xg.put(xd.reshape(1, n * c, H, W))
    ops.call('pfst_maxpool3x3s2', xg.view.data_ptr(), yg.view.data_ptr(), ig.ptr(), n * c, H, W, Ho, Wo, 0 if coef is None else coef.data_ptr(), c,
             0 if amax is None else amax.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    what = f'maxpool {H} x {W}, {view[0]} ({route})'
    xg.intact(what), yg.intact(what), ig.intact(what)
    assert torch.equal(dbits(xg.view), dbits(xd).view(1, n * c, H, W)), f'{what}: the input was changed'
    return yg.view.reshape(n, c, Ho, Wo).clone(), ig.view.reshape(n, c, Ho, Wo).clone(), what


def test_every_route_is_reached(ops):
    fwd = {pool_operands((O.PN, O.PC, H, W), v)[3] for H, W in O.POOL_SHAPES for v in O.POOL_VIEWS}
    bwd = {O.route_maxpool_bwd(H, W, planes(O.PN * O.PC, H, W, lead=d).view.data_ptr()) for H, W in O.POOL_SHAPES for _, d in O.BWD_VIEWS}
    assert fwd | bwd == O.POOL_ROUTES, O.POOL_ROUTES - (fwd | bwd)
    ax = {O.route_axpy(flat(n, a).view.data_ptr(), flat(n, b).view.data_ptr()) for n in O.AXPY_N[:4] for a, b in O.AXPY_VIEWS}
    assert ax == O.AXPY_ROUTES, O.AXPY_ROUTES - ax


@pytest.mark.parametrize('H,W', O.POOL_SHAPES)
def test_maxpool_forward(ops, H, W):
    c = O.pool_case(H, W)
    first = None
    for view in O.POOL_VIEWS:
        y, idx, what = run_pool(ops, c['x'], view)
        same_bits(y, c['y'], what + ' values', c['names'], O.PN)
        bad = (idx.cpu().long() != c['tap']).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} taps differ, the first at {bad[0].tolist()} (family {c['names'][int(bad[0, 0]) // O.PN]!r})"
        if first is None:
            first = (y, idx)
        assert torch.equal(dbits(y), dbits(first[0])) and torch.equal(idx, first[1]), f'{what}: differs from the plain launch'


@pytest.mark.parametrize('H,W', O.POOL_SHAPES)
def test_maxpool_normalise_on_load(ops, H, W):
    c = O.bnl_case(H, W)
    for coef, y_ref, tap_ref in c['coefs']:
        for view in O.POOL_VIEWS[:2]:
            y, idx, what = run_pool(ops, c['x'], view, coef=coef.to(DEV))
            same_bits(y, y_ref, what + f' bnl sc = {coef[:, 2].tolist()}')
            assert torch.equal(idx.cpu().long(), tap_ref), what + f' bnl sc = {coef[:, 2].tolist()}: taps'


@pytest.mark.parametrize('H,W', O.POOL_SHAPES)
def test_maxpool_publishes_max_abs(ops, H, W):
    rnd = O.pool_inputs(H, W)['random']
    b = O.bnl_case(H, W)
    cases = [('random', rnd, None), ('all negative', -rnd.abs() - 1, None), ('all zero', torch.zeros_like(rnd), None)]
    cases += [(f'bnl {i}', b['x'], coef) for i, (coef, _, _) in enumerate(b['coefs'])]
    for name, x, coef in cases:
        ref = O.maxpool_ref(x if coef is None else O.bn_on_load_ref(x, coef))[0]
        for view in O.POOL_VIEWS[:2]:
            slots = ops.amax_slots(torch.device(DEV, torch.cuda.current_device()))
            assert float(slots.abs().max()) == 0.0
            y, _, what = run_pool(ops, x, view, coef=None if coef is None else coef.to(DEV), amax=slots)
            assert float(slots.max()) == float(ref.abs().max()) == float(y.abs().max()), f'{what}, {name}: published {float(slots.max())}'


# ----------------------------------------------------------------------------------------------------------------------- max-pool backward
def run_pool_bwd(ops, dy, idx, hw, view):
    n, c, Ho, Wo = dy.shape
    H, W = hw
    dg = planes(n * c, H, W, lead=view[1])
    route = O.route_maxpool_bwd(H, W, dg.view.data_ptr())
    assert route == ('bwd 2x2' if H % 2 == 0 and W % 2 == 0 and view[1] == 0 else 'bwd generic')
    dyd, before = dy.to(DEV), idx.clone()
    ops.call('pfst_maxpool3x3s2_bwd', dyd.data_ptr(), idx.data_ptr(), dg.view.data_ptr(), n * c, H, W, Ho, Wo, ops._stream())
    torch.cuda.synchronize()
    what = f'maxpool_bwd {H} x {W}, {view[0]} ({route})'
    dg.intact(what)
    assert torch.equal(idx, before) and torch.equal(dyd.cpu(), dy)
    return dg.view.reshape(n, c, H, W).clone(), route, what


@pytest.mark.parametrize('H,W', O.POOL_SHAPES)
def test_maxpool_backward(ops, H, W):
    c = O.pool_case(H, W)
    _, idx, _ = run_pool(ops, c['x'], O.POOL_VIEWS[0])          # the taps of the forward pass, NaN winners included
    assert torch.equal(idx.cpu().long(), c['tap'])
    exact = O.dyadic(tuple(c['tap'].shape), 41, 2.0 ** -6, 8.0)
    rnd = torch.randn(tuple(c['tap'].shape), generator=g(42))
    ref_exact = O.maxpool_bwd_ref(exact, c['tap'], (H, W))
    ref_rnd, ref_abs = O.maxpool_bwd_ref(rnd, c['tap'], (H, W)), O.maxpool_bwd_ref(rnd.abs(), c['tap'], (H, W))
    for view in O.BWD_VIEWS:
        dx, route, what = run_pool_bwd(ops, exact, idx, (H, W), view)
        same_bits(dx, ref_exact, what + ', dyadic dy', c['names'], O.PN)
        dx, route, what = run_pool_bwd(ops, rnd, idx, (H, W), view)
        ratio = worst((dx.double().cpu() - ref_rnd).abs(), 3 * U * ref_abs)
        note('maxpool_bwd', route, ratio)
        assert ratio <= 1.0, f'{what}: {ratio:.3g} x the bound'
    report('maxpool_bwd')


# --------------------------------------------------------------------------------------------------------------------- nearest up-sampling
@pytest.mark.parametrize('hw,u', O.UPS_CASES)
def test_upsample_nearest(ops, hw, u):
    h, w = hw
    nc = O.PN * O.PC
    x = torch.randn(O.PN, O.PC, h, w, generator=g(51))
    x[0, 0, 0, 0], x[1, 2, h - 1, w - 1] = O.NAN, -0.0

    def up(x):
        xd, yg = x.to(DEV), planes(nc, h * u, w * u)
        ops.call('pfst_upsample_nearest', xd.data_ptr(), yg.view.data_ptr(), nc, h, w, u, ops._stream())
        torch.cuda.synchronize()
        yg.intact(f'upsample_nearest {hw} x{u}')
        assert torch.equal(dbits(xd), dbits(x.to(DEV)))
        return yg.view.reshape(O.PN, O.PC, h * u, w * u).clone()

    def up_bwd(dy):
        dyd, dg = dy.to(DEV), planes(nc, h, w, lead=1)
        ops.call('pfst_upsample_nearest_bwd', dyd.data_ptr(), dg.view.data_ptr(), nc, h, w, u, ops._stream())
        torch.cuda.synchronize()
        dg.intact(f'upsample_nearest_bwd {hw} x{u}')
        assert torch.equal(dyd.cpu(), dy)
        return dg.view.reshape(O.PN, O.PC, h, w).clone()

    same_bits(up(x), O.upsample_ref(x, u), f'upsample_nearest {hw} x{u}')
    exact = O.dyadic((O.PN, O.PC, h * u, w * u), 52, 2.0 ** -6, 8.0)
    dx_exact = up_bwd(exact)
    same_bits(dx_exact, O.upsample_bwd_ref(exact, u), f'upsample_nearest_bwd {hw} x{u}, dyadic dy')
    rnd = torch.randn(O.PN, O.PC, h * u, w * u, generator=g(53))
    ratio = worst((up_bwd(rnd).double().cpu() - O.upsample_bwd_ref(rnd, u)).abs(), (u * u - 1) * U * O.upsample_bwd_ref(rnd.abs(), u))
    note('upsample_nearest_bwd', f'x{u}', ratio)
    assert ratio <= 1.0, f'upsample_nearest_bwd {hw} x{u}: {ratio:.3g} x the bound'
    # <up(x), g> = <x, up_bwd(g)>: both kernels' outputs are exact here (a copy; a dyadic sum), so the two float64 dot products differ by
    # their own summation error alone, at most (terms) 2^-52 sum |terms|
    xf = torch.randn(O.PN, O.PC, h, w, generator=g(54))
    terms = up(xf).double().cpu() * exact.double()
    lhs, rhs = float(terms.sum()), float((xf.double() * dx_exact.double().cpu()).sum())
    assert abs(lhs - rhs) <= terms.numel() * 2.0 ** -52 * float(terms.abs().sum()), (lhs, rhs)
    report('upsample_nearest_bwd')


@pytest.mark.parametrize('C', [1, 7])
@pytest.mark.parametrize('HW', [1, 99, 1025])
def test_channel_scale(ops, HW, C):
    N = 2
    x = torch.randn(N, C, HW, 1, generator=g(61)) * 3
    x[0, 0] = O.INF
    x[1, C - 1, HW // 2] = -O.INF
    m = (torch.rand(N, C, generator=g(62)) > 0.3).float() / 0.7
    m[0, 0] = m[1, C - 1] = 0.0          # inf * 0: NaN, as x * 0 in torch
    xd, md, yg = x.to(DEV), m.to(DEV), planes(N * C, HW, 1, lead=1)
    ops.call('pfst_channel_scale', xd.data_ptr(), md.data_ptr(), yg.view.data_ptr(), N, C, HW, ops._stream())
    torch.cuda.synchronize()
    yg.intact('channel_scale')
    ref = x * m.view(N, C, 1, 1)
    assert bool(torch.isnan(ref[0, 0]).all()) and bool(torch.isnan(ref[1, C - 1, HW // 2]).all())
    same_bits(yg.view.reshape(N, C, HW, 1), ref, f'channel_scale C = {C}, HW = {HW}')
    assert torch.equal(dbits(xd), dbits(x.to(DEV))) and torch.equal(md.cpu(), m)


# -------------------------------------------------------------------------------------------------------------------- element-wise kernels
@pytest.mark.parametrize('n', O.FILL_N)
def test_fill(ops, n):
    for lead, value in ((0, 3.25), (1, -0.0), (3, O.INF)):
        gd = flat(n, lead)
        ops.fill_(gd.view.view(-1), value)
        torch.cuda.synchronize()
        gd.intact(f'fill_ n = {n}')
        same_bits(gd.view.view(-1), torch.full((n,), value), f'fill_ n = {n}, {value}')


def run_axpy(ops, y, x, alpha, a, b, alias=False):
    n = y.numel()
    yg = flat(n, a, y)
    xg = yg if alias else flat(n, b, x)
    route = O.route_axpy(yg.view.data_ptr(), xg.view.data_ptr())
    assert route == ('axpy float4' if (a == 0 and (alias or b == 0)) else 'axpy scalar')
    ops.axpy_(yg.view.view(-1), xg.view.view(-1), alpha)
    torch.cuda.synchronize()
    what = f'axpy_ n = {n}, y + {4 * a} B, ' + ('x is y' if alias else f'x + {4 * b} B') + f' ({route})'
    yg.intact(what)
    if not alias:
        xg.intact(what)
        assert torch.equal(dbits(xg.view.view(-1)), dbits(x.to(DEV))), what + ': x was changed'
    return yg.view.view(-1).clone(), route, what


@pytest.mark.parametrize('n', O.AXPY_N)
def test_axpy(ops, n):
    xe, ye = O.dyadic((n,), 71, 0.125, 4.0), O.dyadic((n,), 72, 0.125, 4.0)
    xr, yr = torch.randn(n, generator=g(73)), torch.randn(n, generator=g(74)) * 2
    ar = float(np.float32(0.37))
    for a, b in O.AXPY_VIEWS:
        got, route, what = run_axpy(ops, ye, xe, -1.5, a, b)          # -1.5 x: multiples of 1/16 up to 6, + y: exact
        same_bits(got, ye.double() - 1.5 * xe.double(), what + ', dyadic')
        got, route, what = run_axpy(ops, yr, xr, ar, a, b)
        ref = ar * xr.double() + yr.double()
        ratio = worst((got.double().cpu() - ref).abs(), U * ref.abs())
        note('axpy_', route, ratio)
        assert ratio <= 1.0, f'{what}: {ratio:.3g} x the bound'
    for a in (0, 1):          # x is y: y <- fma(alpha, y, y)
        got, route, what = run_axpy(ops, ye, None, -1.5, a, a, alias=True)
        same_bits(got, ye.double() - 1.5 * ye.double(), what + ', dyadic')
        got, route, what = run_axpy(ops, yr, None, ar, a, a, alias=True)
        ref = ar * yr.double() + yr.double()
        ratio = worst((got.double().cpu() - ref).abs(), U * ref.abs())
        note('axpy_', route + ', x is y', ratio)
        assert ratio <= 1.0, f'{what}: {ratio:.3g} x the bound'
    report('axpy_')


@pytest.mark.parametrize('n', [1, 255, 769, 1000, O.GRID_CAP + 3])
def test_label_conversions(ops, n):
    src = (torch.arange(n) * 37 + 5) % 256          # every value 0 .. 255 once n >= 256
    assert n < 256 or src.unique().numel() == 256
    s64 = src.to(DEV)
    for lead in (0, 1, 3):
        d8 = Pad(n, torch.uint8, lead)
        ops.call('pfst_i64_to_u8', s64.data_ptr(), d8.ptr(), n, ops._stream())
        torch.cuda.synchronize()
        d8.intact(f'to_u8 n = {n}')
        assert torch.equal(d8.view.cpu().long(), src) and torch.equal(s64.cpu(), src)
        d64 = Pad(n, torch.int64, lead % 2)
        ops.call('pfst_u8_to_i64', d8.ptr(), d64.ptr(), n, ops._stream())
        torch.cuda.synchronize()
        d64.intact(f'to_i64 n = {n}'), d8.intact(f'to_i64 n = {n}')
        assert torch.equal(d64.view.cpu(), src) and torch.equal(d8.view.cpu().long(), src)
    assert torch.equal(ops.to_i64(ops.to_u8(s64)), s64)


@pytest.mark.parametrize('n', [1, 257, O.GRID_CAP + 3])
def test_div_scalar(ops, n):
    x = torch.randn(n, generator=g(81)) * 5
    x[0] = 1.0
    for i, d in enumerate(O.DIVISORS):
        gd = flat(n, i % 2, x)
        ops.div_scalar_(gd.view.view(-1), d)
        torch.cuda.synchronize()
        gd.intact(f'div_scalar_ n = {n}')
        same_bits(gd.view.view(-1), x / torch.full_like(x, d), f'div_scalar_ n = {n}, / {d}')          # element by element: IEEE float32 division
    gd = flat(n, 0, x)
    with refused(ops):
        ops.div_scalar_(gd.view.view(-1), 0.0)
    torch.cuda.synchronize()
    gd.intact('div_scalar_ / 0')
    same_bits(gd.view.view(-1), x, 'div_scalar_ / 0 left x as it was')


@pytest.mark.parametrize('H,W', O.FLIP_SHAPES)
def test_flip_planes(ops, H, W):
    nc = 6
    x = torch.randint(-2 ** 31, 2 ** 31, (1, nc, H, W), generator=g(91), dtype=torch.int64).to(torch.int32)          # every bit pattern: NaN payloads too
    xd = x.to(DEV).view(torch.float32)
    for hf in (False, True):
        for vf in (False, True):
            yg = planes(nc, H, W, lead=1)
            ops.call('pfst_flip_planes', xd.data_ptr(), yg.view.data_ptr(), nc, H, W, int(hf), int(vf), ops._stream())
            torch.cuda.synchronize()
            yg.intact(f'flip_planes {H} x {W}')
            assert torch.equal(dbits(yg.view).cpu(), O.flip_ref(x, hf, vf)), f'flip_planes {H} x {W}, horizontal={hf}, vertical={vf}'
            assert torch.equal(dbits(xd).cpu(), x)
            assert torch.equal(dbits(ops.flip_planes(xd, hf, vf)), dbits(yg.view))
    with refused(ops):
        ops.call('pfst_flip_planes', xd.data_ptr(), xd.data_ptr(), nc, H, W, 1, 0, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dbits(xd).cpu(), x)


# ---------------------------------------------------------------------------------------------------------------------------------- softmax
def softmax_views(ops, x, what):
    """softmax_nchw on the three kinds of channel-slice views (x and out alike): canaries, x unchanged, the same bits from each"""
    N, C, HW, _ = x.shape
    outs = []
    for kind, kw in O.SM_VIEWS.items():
        kx, ko = dict(kw), dict(kw, back=5)          # out: two more channels behind the view, so the two batch strides differ
        if 'odd' in kw:
            kx['odd'], ko['odd'] = 1 - ((C + 4) * HW) % 2, 1 - ((C + 6) * HW) % 2
        xg, og = Guard(tuple(x.shape), **kx), Guard(tuple(x.shape), **ko)
        xv = xg.put(x.to(DEV))
        assert ops._bs(og.view) > ops._bs(xv) > C * HW and (kind != 'lead' or xg.off == HW + 1)
        assert kind != 'odd stride' or ops._bs(xv) % 2 == 1 == ops._bs(og.view) % 2
        ops.softmax_nchw(xv, out=og.view)
        torch.cuda.synchronize()
        xg.intact(f'{what}, {kind}: x'), og.intact(f'{what}, {kind}: out')
        assert torch.equal(dbits(xv), dbits(x.to(DEV))), f'{what}, {kind}: x was changed'
        outs.append(og.view.clone())
        assert torch.equal(dbits(outs[-1]), dbits(outs[0])), f'{what}: the {kind} view differs from the first'
    return outs[0].cpu()


@pytest.mark.parametrize('HW', O.SM_HW)
@pytest.mark.parametrize('C', O.SM_C)
def test_softmax(ops, C, HW):
    for fam in O.SM_FAMILIES:
        x = O.softmax_inputs(C, HW, fam)
        ref = O.softmax_reference(x)
        p = softmax_views(ops, x, f'softmax C = {C}, HW = {HW}, {fam}')
        assert not bool(torch.isnan(p).any())
        ratio = O.softmax_ratio(p, ref)
        note('softmax', fam, ratio)
        assert ratio < 1.0, f'softmax C = {C}, HW = {HW}, {fam}: {ratio:.3g} x the bound'
        rows = float((p.double().sum(1) - 1).abs().max()) / (C * U)
        note('softmax', 'row sums', rows)
        assert rows <= 1.0, f'softmax C = {C}, HW = {HW}, {fam}: rows sum to 1 within {rows:.3g} x C u'
        if fam == 'one class 120 below' and C > 1:
            assert bool((p[:, C // 2] == 0).all())
        if fam == '-inf classes':
            assert bool((p[:, 1::2] == 0).all())
    # the constructed rows: the NaN mask of torch's float32 softmax; every other row as above
    x, rows = O.softmax_special(C, HW)
    p = softmax_views(ops, x, f'softmax C = {C}, HW = {HW}, +inf and all -inf rows')
    assert torch.equal(torch.isnan(p), torch.isnan(torch.softmax(x, 1)))
    ref = O.softmax_reference(torch.where(rows, torch.zeros_like(x), x))          # the other rows are unchanged by this
    keep = ~rows.expand_as(p)
    err = (p.double() - ref['p']).abs() / (ref['bound'] * ref['p'] + O.TINY)
    ratio = float(err[keep].max()) if bool(keep.any()) else 0.0
    note('softmax', 'beside NaN rows', ratio)
    assert ratio < 1.0
    report('softmax')


# ---------------------------------------------------------------------------------------------------------------------------------- arg-max
def run_argmax(ops, x, lead, what):
    """argmax_nchw on a channel-slice view, labels into byte canaries"""
    N, C, HW, _ = x.shape
    xg, lab = Guard(tuple(x.shape), odd=1), Pad(N * HW, torch.uint8, lead)
    xv = xg.put(x.to(DEV))
    ops.call('pfst_argmax_nchw', xv.data_ptr(), ops._bs(xv), lab.ptr(), N, C, HW, ops._stream())
    torch.cuda.synchronize()
    xg.intact(what), lab.intact(what)
    assert torch.equal(dbits(xv), dbits(x.to(DEV)))
    assert torch.equal(ops.argmax_nchw(xv).flatten(), lab.view)
    return lab.view.cpu().long().view(N, HW, 1)


def run_finalize(ops, acc, views, lead, what):
    """tta_finalize on a dense sum, labels into byte canaries; lead = 0 and HW % 4 == 0: the 16-byte path"""
    N, C, HW, _ = acc.shape
    ad, lab = acc.to(DEV), Pad(N * HW, torch.uint8, lead)
    ops.call('pfst_tta_finalize', ad.data_ptr(), N, C, HW, views, lab.ptr(), ops._stream())
    torch.cuda.synchronize()
    lab.intact(what)
    assert torch.equal(dbits(ad), dbits(acc.to(DEV)))
    return lab.view.cpu().long().view(N, HW, 1)


def first_bad(got, ref, x):
    bad = (got != ref).nonzero()
    if bad.numel() == 0:
        return ''
    n, p, _ = bad[0].tolist()
    return f'{bad.shape[0]} labels differ, the first at image {n}, pixel {p}: {int(got[n, p, 0])} against {int(ref[n, p, 0])}, classes {x[n, :, p, 0].tolist()[:20]}'


@pytest.mark.parametrize('HW', O.AM_HW)
@pytest.mark.parametrize('C', O.AM_C)
def test_argmax_and_tta_finalize(ops, C, HW):
    for fam in O.AM_FAMILIES:
        x = O.argmax_inputs(C, HW, fam)
        ref = O.argmax_ref(x)
        q = x / torch.full_like(x, 3.0)          # tta_finalize divides first (IEEE float32, as div_scalar_)
        ref3 = O.argmax_ref(q)
        for lead in (0, 1):
            what = f'C = {C}, HW = {HW}, {fam}, labels + {lead} B'
            got = run_argmax(ops, x, lead, 'argmax_nchw ' + what)
            assert torch.equal(got, ref), 'argmax_nchw ' + what + ': ' + first_bad(got, ref, x)
            got = run_finalize(ops, x, 3, lead, 'tta_finalize ' + what)
            assert torch.equal(got, ref3), 'tta_finalize ' + what + ': ' + first_bad(got, ref3, q)
            assert torch.equal(ops.tta_finalize(x.to(DEV), 3).cpu().long().view(O.AM_N, HW, 1), ref3)


@pytest.mark.parametrize('C', O.AM_C)
def test_argmax_ties_between_every_pair_of_classes(ops, C):
    x, win = O.pair_ties(C)
    for lead in (0, 1):
        assert torch.equal(run_argmax(ops, x, lead, f'argmax_nchw, pair ties, C = {C}')[0, :, 0], win)
        assert torch.equal(run_finalize(ops, x, 1, lead, f'tta_finalize, pair ties, C = {C}')[0, :, 0], win)          # lead 0: 16-byte path
        assert torch.equal(run_finalize(ops, x[:, :, :-1].contiguous(), 1, lead, f'tta_finalize, pair ties, C = {C}')[0, :, 0], win[:-1])


def test_argmax_refuses_256_classes(ops):
    x = torch.zeros(1, 256, 8, 1, device=DEV)
    lab = Pad(8, torch.uint8)
    with refused(ops):
        ops.call('pfst_argmax_nchw', x.data_ptr(), 256 * 8, lab.ptr(), 1, 256, 8, ops._stream())
    with refused(ops):
        ops.call('pfst_tta_finalize', x.data_ptr(), 1, 256, 8, 1, lab.ptr(), ops._stream())
    torch.cuda.synchronize()
    lab.intact('256 classes')
    assert bool((lab.view == FILL[torch.uint8]).all())


@pytest.mark.parametrize('HW', [1025, 1028])
def test_scene_tta_finalize_lets_the_first_nan_win(ops, HW):
    """scene_tta_finalize documents div_scalar_ + argmax_nchw and is tied to them on NaN-free sums in test_scene_tta_gpu.py: the same rule here"""
    for fam in ('NaN classes', 'NaN after +inf', 'three values'):
        x = O.argmax_inputs(19, HW, fam)[0]          # [C, HW, 1]
        ref = O.argmax_ref((x / torch.full_like(x, 3.0))[None])[0]
        lab, _, _ = ops.scene_tta_finalize(x.to(DEV), 3)
        assert torch.equal(lab.cpu().long(), ref), fam
        assert torch.equal(lab, ops.argmax_nchw(ops.div_scalar_(x.to(DEV)[None].clone(), 3))[0])


# ---------------------------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize('C', O.WIN_C)
@pytest.mark.parametrize('H,W', O.CANVASES)
def test_window_sums(ops, H, W, C):
    N = O.WIN_N
    c = O.window_case(H, W, C)
    pg, cg = planes(N * C, H, W, lead=1), planes(N, H, W, lead=1)
    preds, count = pg.view.view(N, C, H, W).zero_(), cg.view.view(N, 1, H, W).zero_()
    assert pg.off == cg.off == H * W + 1          # one canary plane and a 4-byte lead in front of each

    def normalized(step):
        ng = planes(N * C, H, W, lead=1, src=preds)
        out = ops.window_normalize_(ng.view.view(N, C, H, W), count)
        torch.cuda.synchronize()
        ng.intact('window_normalize_'), cg.intact('window_normalize_')
        ref = c['steps'][step][0] / c['steps'][step][1]          # float32 division; 0 / 0: NaN
        same_bits(out, ref, f'window_normalize_ after call {step}')
        same_bits(count, c['steps'][step][1], 'window_normalize_ left the counts')
        return ref

    wins = O.windows(H, W)
    for i, ((y1, x1, hc, wc), crop) in enumerate(zip(wins, c['crops'])):
        cd = crop.to(DEV)
        ops.window_accumulate_(preds, count, cd, y1, x1)
        torch.cuda.synchronize()
        what = f'window_accumulate_ call {i}: {hc} x {wc} at ({y1}, {x1}) of {H} x {W}'
        pg.intact(what), cg.intact(what)
        same_bits(preds, c['steps'][i][0], what + ', preds')
        same_bits(count, c['steps'][i][1], what + ', count')
        assert torch.equal(cd.cpu(), crop)
        if i == len(wins) - 2:
            assert bool(torch.isnan(normalized(i)).any()), 'a pixel that no window covered: 0 / 0'
    assert not bool(torch.isnan(normalized(len(wins) - 1)).any())
    for y1, x1, hc, wc in O.refused_windows(H, W):
        with refused(ops):
            ops.window_accumulate_(preds, count, torch.ones(N, C, hc, wc, device=DEV), y1, x1)
    torch.cuda.synchronize()
    pg.intact('refused windows'), cg.intact('refused windows')
    same_bits(preds, c['steps'][-1][0], 'refused windows left preds')
    same_bits(count, c['steps'][-1][1], 'refused windows left count')
