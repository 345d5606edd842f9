"""The depthwise 3x3 family (csrc/dwconv.hip: pfst_dwconv3x3, _bwd, _wgrad, _multi_fwd, _multi_bwd) where tests/test_hip_ops.py and
tests/test_deterministic_kernels_gpu.py hold everything but (dil, H, W) fixed: channel counts that are no multiple of the plane kernels'
four channels per workgroup, one image, operands that are channel slices of larger buffers, planes that are misaligned although W % 4 == 0,
odd batch strides, the one-row clamp of strip_rows, and dilations at least as large as the plane.

References: fp64 on the CPU (F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight, mean and biased variance), seeded generators.
Bounds, INHERITED from test_hip_ops.test_depthwise: 1e-5 forward / dx / accumulate, 1e-4 weight gradients, 2e-5 mean and invstd out of
bn_finalize_partials.  Unlike there, every bound but the last is applied PER CHANNEL (max |got - ref| over a channel against that channel's
max |ref|), so that a wrong tail channel cannot hide behind a larger one; mean and invstd against the vector's maximum.  The inputs carry
offsets (x = randn + 1, w = randn + 0.25) so that at C == 1 the "vector's maximum" of the mean is not a sum that cancels to nothing; each
case asserts max |mean| > 0.1 before it uses the bound.  The partial sums themselves are held to the kernel's own output in fp64 within
64 * 2^-24 * sum |y| (resp. sum y^2): a thread adds at most 36 values in fp32 (35 rounding steps) before the block reduction in fp64 and the final rounding.
Fused options keep the bit-identity the suite already proves them by (torch.equal): bnl against the tensor bn_apply writes, bnb against
bn_backward writing dL/dpre first, the fused backward's dx against the data-gradient kernel, multi-branch outputs / partials against
per-branch launches.

Canaries: every output (y, dx, dw, the multi-branch dws) is a view into a buffer filled with SENT; afterwards everything outside the view is
still SENT -- the channels in front of and behind a slice, the gap between images, the 9 floats either side of dw.  The stats scratch is
filled with SENT too: nothing behind the [C][slots][2] sums (and the min/max block) may change.

Routes: dw_route() restates the host's choice (plane1/2/3, strip0/1/2/3, strips per image); every case names the route it is meant to hit
and asserts the helper agrees.  Covered here: plane1, plane2, plane3, strip0 (W % 4 != 0; misaligned plane; odd batch stride; one strip and
several), strip1 (several strips; bnl / bnb on a plane shape; the one-row clamp), strip2 and strip3 (bnl / bnb on plane shapes; strip3 with
two strips), each forward and with the weight gradient (WG), the stand-alone weight-gradient kernel in its four forms, the multi-branch
kernels with 1, 2, 3 branches; with ragged channel groups (C = 1, 6, 7 against cpb = 4) and N == 1 throughout group A.

One reference is zero by construction: a multi-branch branch with dil >= H, W under BatchNorm backward (multi_checks says why); its weight
gradient is held to the same 1e-4, of sum |x| |dL/dpre| instead of max |ref|.

MEASURED on an MI355X, worst ratio to its bound per group (1.0 would fail; the bounds themselves are the inherited ones above):
  group   forward   dx       dw       mean     invstd   partial sums
  A       0.016     0.019    0.037    0.0037   0.019    0.036          (dw of the cancelling sum: 1.7e-4)
  B       0.015     0.020    0.0053   0.0025   0.0060   0.012
  C       0.014     0.017    0.0038   0.0023   0.0049   0.013
  D       exact     exact    0.015
so the per-channel norm costs these kernels nothing: the worst channel sits at 4 % of the weight-gradient bound and 2 % of the others.
In deterministic mode the scalar route's weight gradients differ bitwise from the vector route's in every group B case (printed by
test_b_misaligned_operands_take_the_scalar_route), which is what lets that test tell the two routes apart.

Mutations of csrc/dwconv.hip tried against this file (none committed):
  1. `c1 = c0 + cpb` without the min (plane and multi-branch kernels) -- by reading: with C = 1, 6, 7 the last workgroup goes on to channels
     C .. c0 + 3, which are the canary channels behind the view (Guard keeps three), and writes stats slots behind [C][slots]: Guard.intact and
     the SENT check of check_partials fail in test_a_forward, test_a_gradients, test_a_multi_branch (every plane1/2/3 row) and in group B's
     plane rows with C = 6; the existing depthwise tests (C % 4 == 0) cannot see it.
  2. `(uintptr_t)x` dropped from pfst_dwconv3x3_bwd's `vec` -- by reading: a misaligned x then runs the vector kernel; the hardware tolerates
     the 4-byte-aligned 16-byte loads, so the VALUES stay right and only the order of the weight-gradient sums changes:
     test_b_misaligned_operands_take_the_scalar_route fails on `dw with a misaligned x differs from that with a misaligned dy` (calls bwd
     and bnb, all six cases); nothing else notices.
  3. `rows < 1` clamped to 2 -- run on the MI355X: test_c_strips_at_the_clamp fails for (16, 40, 512), (16, 40, 510) and (36, 20, 1024)
     on the slot count (20 / 10 strips instead of 40 / 20); the other 143 depthwise tests of the suite, old and new, pass.
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import SENT, Guard, chan_close, note, out_view, report
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD, WGRAD, STAT = 1e-5, 1e-4, 2e-5            # inherited from test_hip_ops.test_depthwise
SUMS = 64 * 2.0 ** -24                         # partial sums against the kernel's own output (docstring)
LDS = 64 * 1024                                # dwconv.hip DW_LDS_BYTES


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------- the host's choice, restated
def strip_rows(H, W, dil):
    """dwconv.hip strip_rows: the whole plane when it fits 64 KiB, else the rows that fit with their halo, at least one"""
    if H * W * 4 <= LDS:
        return H
    return min(max(LDS // (W * 4) - 2 * dil, 1), H)


def strip_lds(H, W, dil):
    """dwconv.hip strip_lds: bytes of a staged strip; its halo is clipped to the plane"""
    return min(strip_rows(H, W, dil) + 2 * dil, H) * W * 4


def dw_route(ops, H, W, dil, operands, bnl=False, bnb=False, wgrad=False):
    """-> (route, strips per image) of pfst_dwconv3x3 / _bwd (wgrad: pfst_dwconv3x3_wgrad, which has strip kernels only) for these tensors"""
    vec = W % 4 == 0 and all(t.data_ptr() % 16 == 0 and ops._bs(t) % 4 == 0 for t in operands)
    mode = 0 if not vec else 1 if dil % 4 == 0 else 3 if dil == 1 else 2
    plane = mode != 0 and H * W * 4 <= LDS and not bnl and not bnb and not wgrad
    return ('plane' if plane else 'strip') + str(mode), cdiv(H, strip_rows(H, W, dil))


def folded(route):
    """the route of the same shape with bnl or bnb (or of the weight-gradient kernel): those have no whole-plane variant"""
    return route.replace('plane', 'strip')


# ------------------------------------------------------------------------------------------------------------------------------ the checks
def vec_close(got, ref, bound, group, kind):
    got, ref = got.detach().double().cpu(), ref.double()
    ratio = float((got - ref).abs().max() / (bound * ref.abs().max()))
    note(group, kind, ratio)
    assert ratio < 1.0, f'{kind}: {ratio:.3g} x the bound {bound}'


@contextlib.contextmanager
def det_mode(ops, on=True):
    """deterministic mode on / off inside the block, the previous setting restored behind it"""
    before = ops.is_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(before)


class DwGuard:
    """a zeroed [C, 1, 3, 3] weight gradient with 9 SENT floats either side"""

    def __init__(self, C, fill=0.0):
        self.buf = torch.full((9 * C + 18,), SENT, device=DEV)
        self.dw = self.buf[9:9 + 9 * C]
        self.dw.fill_(fill)
        self.dw = self.dw.view(C, 1, 3, 3)

    def intact(self, what=''):
        assert bool((self.buf[:9] == SENT).all()) and bool((self.buf[-9:] == SENT).all()), f'{what}: floats beside dw were written'


def sent_scratch(ops, dev, tag, need, floor):
    st = ops._scratch(dev, tag, need, floor)
    st.fill_(SENT)
    return st


def check_partials(ops, y, st, slots, count, y_ref, group, minmax=True):
    """the [C][slots][2] sums against the kernel's own output in fp64, the min/max block exactly, nothing behind them written, and
    bn_finalize_partials against the fp64 reference's mean / biased variance"""
    C = y.shape[1]
    used = (4 if minmax else 2) * C * slots
    assert bool((st[used:] == SENT).all()), 'the stats scratch was written behind its partials'
    part = st[:2 * C * slots].view(C, slots, 2).double().cpu().sum(1)
    yd = y.double().cpu()
    for k, (tot, mag) in enumerate([(yd.sum((0, 2, 3)), yd.abs().sum((0, 2, 3))), ((yd * yd).sum((0, 2, 3)), (yd * yd).sum((0, 2, 3)))]):
        ratio = float(((part[:, k] - tot).abs() / (SUMS * mag)).max())
        note(group, 'partial sums', ratio)
        assert ratio < 1.0, f'partial sums [{k}]: {ratio:.3g} x the bound'
    if minmax:
        mm = st[2 * C * slots:4 * C * slots].view(C, slots, 2)
        assert torch.equal(mm[:, :, 0].min(dim=1)[0], y.amin(dim=(0, 2, 3))) and torch.equal(mm[:, :, 1].max(dim=1)[0], y.amax(dim=(0, 2, 3)))
    mean, invstd = ops.bn_finalize_partials(st, slots, C, count)
    yr = y_ref.double()
    mean_ref = yr.mean((0, 2, 3))
    assert float(mean_ref.abs().max()) > 0.1          # the bound is relative to this (docstring)
    vec_close(mean, mean_ref, STAT, group, 'mean')
    vec_close(invstd, 1.0 / torch.sqrt(yr.var((0, 2, 3), unbiased=False) + 1e-5), STAT, group, 'invstd')


# ---------------------------------------------------------------------------------------------------------------- inputs and fp64 references
@functools.lru_cache(maxsize=None)
def case_data(N, C, dil, H, W):
    """CPU inputs and the fp64 references of one (N, C, dil, H, W), computed once and never modified"""
    x = torch.randn(N, C, H, W, generator=g(1)) + 1.0
    w = torch.randn(C, 1, 3, 3, generator=g(2)) + 0.25
    dy = torch.randn(N, C, H, W, generator=g(3))
    d = dict(x=x, w=w, dy=dy)
    d['y'] = F.conv2d(x.double(), w.double(), None, 1, dil, dil, C)
    d['dx'] = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), 1, dil, dil, C)
    d['dw'] = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), 1, dil, dil, C)
    d['pre'] = torch.randn(N, C, H, W, generator=g(11)) * 2
    d['gamma'] = (torch.rand(C, generator=g(12)) + 0.5) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
    d['beta'] = torch.randn(C, generator=g(13))
    d['g2'], d['b2'] = torch.rand(C, generator=g(14)) + 0.5, torch.randn(C, generator=g(15)) * 0.3
    d['dyo'] = torch.randn(N, C, H, W, generator=g(16))
    return d


def ref_dx(d, dy, dil):
    C = d['w'].shape[0]
    return torch.nn.grad.conv2d_input(d['x'].shape, d['w'].double(), dy.double().cpu(), 1, dil, dil, C)


def ref_dw(x, d, dy, dil):
    C = d['w'].shape[0]
    return torch.nn.grad.conv2d_weight(x.double().cpu(), d['w'].shape, dy.double().cpu(), 1, dil, dil, C)


def bnb_setup(ops, d, xd, wd, dil):
    """this layer's own BatchNorm backward: pre = its convolution output, dyo the gradient of its BN + ReLU output -> (pre, dyo, rec, dL/dpre)"""
    C = wd.shape[0]
    pre = ops.dwconv(xd, wd, dil)
    g2, b2 = d['g2'].to(DEV), d['b2'].to(DEV)
    m2, i2, _ = ops.bn_stats(pre, gamma=g2, beta=b2)
    dyo = d['dyo'].to(DEV)
    dpre = ops.bn_backward(dyo, None, pre, m2, i2, g2, torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), True, beta=b2)
    rec = ops.bn_backward_sums(dyo, pre, m2, i2, g2, b2, torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
    return pre, dyo, rec, dpre


# =========================================================================================================== A: channel tails, batch sizes
NC = [(1, 1), (1, 7), (3, 6)]                  # one short group; 4 + 3 with N == 1; 4 + 2
A_ROWS = [('plane3', 1, 1, 16, 20), ('plane1', 1, 12, 32, 32), ('plane2', 1, 3, 24, 32), ('plane1', 1, 4, 128, 128),     # the last: n4 == 8 * 512
          ('strip1', 2, 4, 130, 132), ('strip0', 1, 2, 7, 9), ('strip0', 2, 3, 131, 130)]
a_cases = pytest.mark.parametrize('route,strips,dil,H,W', A_ROWS)
a_nc = pytest.mark.parametrize('N,C', NC)


def dev_inputs(d):
    return d['x'].to(DEV), d['w'].to(DEV), d['dy'].to(DEV)


@a_nc
@a_cases
def test_a_forward(ops, N, C, route, strips, dil, H, W):
    """dwconv, with fused statistics and min/max partials, and with the normalisation of the layer in front applied on load"""
    d = case_data(N, C, dil, H, W)
    xd, wd, _ = dev_inputs(d)
    shape = (N, C, H, W)
    gd, out = out_view(shape)
    assert dw_route(ops, H, W, dil, [xd, out]) == (route, strips)
    ops.dwconv(xd, wd, dil, out=out)
    chan_close(out, d['y'], FWD, 'A', 'forward')
    gd.intact('forward')
    slots = N * ops.lib().pfst_dwconv_stats_slots(H, W, dil)
    assert slots == N * strips
    gd2, out2 = out_view(shape)
    sent_scratch(ops, xd.device, 'stats', 4 * C * slots, ops._STATS_FLOOR)
    y2, st, sl = ops.dwconv(xd, wd, dil, out=out2, want_stats=True, want_minmax=True)
    assert sl == slots and torch.equal(y2, out)
    gd2.intact('forward with statistics')
    check_partials(ops, y2, st, sl, N * H * W, d['y'], 'A')
    # normalise-on-load: the strip kernel of the same mode, bit-identical to the kernel on the tensor bn_apply would have written
    pre, gamma, beta = d['pre'].to(DEV), d['gamma'].to(DEV), d['beta'].to(DEV)
    mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
    ymat = ops.bn_apply(pre, mean, invstd, gamma, beta, True)
    gd3, out3 = out_view(shape)
    assert dw_route(ops, H, W, dil, [pre, out3], bnl=True) == (folded(route), strips)
    ops.dwconv(pre, wd, dil, out=out3, bnl=coef)
    assert torch.equal(out3, ops.dwconv(ymat, wd, dil))
    chan_close(out3, F.conv2d(ymat.double().cpu(), d['w'].double(), None, 1, dil, dil, C), FWD, 'A', 'forward')
    gd3.intact('forward, normalise-on-load')
    report('A')


def backward_calls(ops, d, dil, group, route, strips, det):
    """the data gradient, the weight gradient and the fused backward in all its forms for one case, outputs in canary buffers"""
    N, C, H, W = d['x'].shape
    shape = (N, C, H, W)
    xd, wd, dyd = dev_inputs(d)
    with det_mode(ops, det):
        if not det:
            gd, dx = out_view(shape)
            assert dw_route(ops, H, W, dil, [dyd, dx]) == (route, strips)
            ops.dwconv(dyd, wd, dil, flip=True, out=dx)
            chan_close(dx, d['dx'], FWD, group, 'dx')
            gd.intact('data gradient')
            gd, acc = out_view(shape)
            ops.dwconv(dyd, wd, dil, flip=True, out=gd.put(xd), accumulate=True)
            chan_close(acc, d['dx'] + d['x'].double(), FWD, group, 'dx')
            gd.intact('data gradient, accumulate')
        dgrad = ops.dwconv(dyd, wd, dil, flip=True)
        # the stand-alone weight-gradient kernel
        dwg = DwGuard(C)
        assert dw_route(ops, H, W, dil, [xd, dyd], wgrad=True) == (folded(route), strips)
        ops.dwconv_wgrad_(dwg.dw, xd, dyd, dil)
        chan_close(dwg.dw, d['dw'], WGRAD, group, 'dw', cdim=0)
        dwg.intact('wgrad')
        # both gradients in one pass, then accumulating into both outputs
        gd, dx = out_view(shape)
        dwg = DwGuard(C)
        assert dw_route(ops, H, W, dil, [dyd, dx, xd]) == (route, strips)
        ops.dwconv_bwd_(dwg.dw, xd, dyd, wd, dil, dx)
        assert torch.equal(dx, dgrad), 'fused backward: dx against the data-gradient kernel'
        chan_close(dx, d['dx'], FWD, group, 'dx')
        chan_close(dwg.dw, d['dw'], WGRAD, group, 'dw', cdim=0)
        gd.put(xd)
        ops.dwconv_bwd_(dwg.dw, xd, dyd, wd, dil, dx, accumulate=True)
        chan_close(dx, d['dx'] + d['x'].double(), FWD, group, 'dx')
        chan_close(dwg.dw, 2 * d['dw'], WGRAD, group, 'dw', cdim=0)
        gd.intact('fused backward')
        dwg.intact('fused backward')
        # normalise-on-load of the forward input
        if not det:
            pre, gamma, beta = d['pre'].to(DEV), d['gamma'].to(DEV), d['beta'].to(DEV)
            mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
            ymat = ops.bn_apply(pre, mean, invstd, gamma, beta, True)
            gd, dx = out_view(shape)
            dwg = DwGuard(C)
            assert dw_route(ops, H, W, dil, [dyd, dx, pre], bnl=True) == (folded(route), strips)
            ops.dwconv_bwd_(dwg.dw, pre, dyd, wd, dil, dx, bnl=coef)
            assert torch.equal(dx, dgrad), 'normalise-on-load: dx'
            chan_close(dwg.dw, ref_dw(ymat, d, dyd, dil), WGRAD, group, 'dw', cdim=0)
            gd.intact('fused backward, bnl')
            dwg.intact('fused backward, bnl')
        # BatchNorm backward's second pass applied while staging
        with det_mode(ops, False):
            pre2, dyo, rec, dpre = bnb_setup(ops, d, xd, wd, dil)
        dxb = torch.empty_like(xd)
        ops.dwconv_bwd_(torch.zeros_like(wd), xd, dpre, wd, dil, dxb)
        gd, dx = out_view(shape)
        dwg = DwGuard(C)
        assert dw_route(ops, H, W, dil, [dyo, dx, xd, pre2], bnb=True) == (folded(route), strips)
        ops.dwconv_bwd_(dwg.dw, xd, dyo, wd, dil, dx, bnb=(pre2, rec))
        assert torch.equal(dx, dxb), 'BatchNorm backward on the fly: dx'
        chan_close(dx, ref_dx(d, dpre, dil), FWD, group, 'dx')
        chan_close(dwg.dw, ref_dw(d['x'], d, dpre, dil), WGRAD, group, 'dw', cdim=0)
        gd.intact('fused backward, bnb')
        dwg.intact('fused backward, bnb')


@pytest.mark.parametrize('det', [False, True])
@a_nc
@a_cases
def test_a_gradients(ops, N, C, route, strips, dil, H, W, det):
    """dwconv(flip), dwconv_wgrad_, dwconv_bwd_ plain / accumulate / bnl / bnb; det: the weight gradients through the [C][det_T][9] scratch and
    dw_det_reduce_kernel on dim3(C)"""
    backward_calls(ops, case_data(N, C, dil, H, W), dil, 'A', route, strips, det)
    report('A')


MULTI = [(32, 32, (12, 24, 36)), (24, 40, (4, 8)), (16, 16, (36,))]


@functools.lru_cache(maxsize=None)
def multi_data(N, C, H, W, dils):
    x = torch.randn(N, C, H, W, generator=g(1)) + 1.0
    ws = [torch.randn(C, 1, 3, 3, generator=g(2 + i)) + 0.25 for i in range(len(dils))]
    dys = [torch.randn(N, C, H, W, generator=g(7 + i)) for i in range(len(dils))]
    ys = [F.conv2d(x.double(), ws[i].double(), None, 1, dl, dl, C) for i, dl in enumerate(dils)]
    dx = sum(torch.nn.grad.conv2d_input(x.shape, ws[i].double(), dys[i].double(), 1, dl, dl, C) for i, dl in enumerate(dils))
    dws = [torch.nn.grad.conv2d_weight(x.double(), ws[i].shape, dys[i].double(), 1, dl, dl, C) for i, dl in enumerate(dils)]
    return dict(x=x, ws=ws, dys=dys, ys=ys, dx=dx, dws=dws, mg=torch.randn(N, C, generator=g(20)))


def multi_checks(ops, d, dils, xd, dyd, group, make_dx):
    """dwconv_multi with statistics, min/max and plane means, and dwconv_multi_bwd_ plain / accumulate / mean_grad / bnb for the operands
    xd, dyd (possibly views); make_dx() -> (guard, view)"""
    N, C, H, W = d['x'].shape
    k, dl = len(dils), list(dils)
    wd = [w.to(DEV) for w in d['ws']]
    assert ops.dwconv_multi_ok(xd, dl)
    for i in range(k):
        sent_scratch(ops, xd.device, ('multi', i), 4 * C * N, 1 << 16)
    res, mean = ops.dwconv_multi(xd, wd, dl, want_stats=True, want_minmax=True, want_mean=True)
    keep = [(y, st.clone(), sl) for y, st, sl in res]
    for i, dil in enumerate(dils):
        y, st, sl = keep[i]
        assert sl == N
        chan_close(y, d['ys'][i], FWD, group, 'forward')
        check_partials(ops, y, st, sl, N * H * W, d['ys'][i], group)
        assert dw_route(ops, H, W, dil, [xd, y]) == ('plane1', 1)
        y1, st1, sl1 = ops.dwconv(xd, wd[i], dil, want_stats=True, want_minmax=True)          # the branch's own launch: bit for bit
        assert torch.equal(y, y1) and sl == sl1 and torch.equal(st[:4 * C * sl], st1[:4 * C * sl1]), (i, dil)
    mref = d['x'].double().mean((2, 3))
    assert tuple(mean.shape) == (N, C, 1, 1)
    # fp64 sum, one rounding of 1 / (H W) to fp32, one of the result
    assert bool(((mean.double().cpu().view(N, C) - mref).abs() <= 2.0 ** -23 * mref.abs() + 1e-10).all())
    gap = ops.global_avgpool(xd)
    assert float((mean - gap).abs().max()) <= 1e-7 * float(gap.abs().max())

    def bwd(dys_, what, ref_dx_, ref_dws, cancels=None, **kw):
        gd, dx = make_dx()
        pref = kw.get('accumulate', False)
        if pref:
            gd.put(d['x'].to(DEV))
        dwgs = [DwGuard(C) for _ in range(k)]
        ops.dwconv_multi_bwd_([q.dw for q in dwgs], xd, dys_, wd, dl, dx, **kw)
        chan_close(dx, ref_dx_ + (d['x'].double() if pref else 0.0), FWD, group, 'dx', what=what + ': dx')
        for i in range(k):
            if cancels is not None and cancels[i] is not None:
                chan_close(dwgs[i].dw, ref_dws[i], WGRAD, group, 'dw, cancelling sum', cdim=0, what=f'{what}: dw[{i}]', scale=cancels[i])
            else:
                chan_close(dwgs[i].dw, ref_dws[i], WGRAD, group, 'dw', cdim=0, what=f'{what}: dw[{i}]')
            dwgs[i].intact(what)
        gd.intact(what)
        return dx

    bwd(dyd, 'multi backward', d['dx'], d['dws'])
    bwd(dyd, 'multi backward, accumulate', d['dx'], d['dws'], accumulate=True)
    bwd(dyd, 'multi backward, mean_grad', d['dx'] + (d['mg'].double() / (H * W)).view(N, C, 1, 1), d['dws'], mean_grad=d['mg'].to(DEV))
    # every branch's BatchNorm backward applied on the fly: as writing the dL/dpre tensors first, bit for bit
    gam = [(torch.rand(C, generator=g(30 + i)) + 0.5).to(DEV) for i in range(k)]
    bet = [(torch.randn(C, generator=g(40 + i)) * 0.3).to(DEV) for i in range(k)]
    pres = [q[0] for q in keep]
    dyc = [t.contiguous() for t in dyd]
    stats = [ops.bn_stats(pres[i], gamma=gam[i], beta=bet[i]) for i in range(k)]
    dpres = [ops.bn_backward(dyc[i], None, pres[i], stats[i][0], stats[i][1], gam[i], None, None, True, beta=bet[i]) for i in range(k)]
    recs = [ops.bn_backward_sums(dyc[i], pres[i], stats[i][0], stats[i][1], gam[i], bet[i], None, None) for i in range(k)]
    rdx = sum(torch.nn.grad.conv2d_input(d['x'].shape, d['ws'][i].double(), dpres[i].double().cpu(), 1, dil, dil, C) for i, dil in enumerate(dils))
    rdw = [torch.nn.grad.conv2d_weight(d['x'].double(), d['ws'][i].shape, dpres[i].double().cpu(), 1, dil, dil, C) for i, dil in enumerate(dils)]
    # A branch whose dilation is at least H and W has the centre tap only: its output is w[c, 1, 1] x, BatchNorm backward makes dL/dpre
    # orthogonal to that output over the batch, and the one weight gradient that is not identically zero, sum x dL/dpre, is ZERO in exact
    # arithmetic.  There is no max |ref| to be relative to; such a branch is held to the bound times the magnitude of what is summed,
    # sum |x| |dL/dpre| per channel (the other entries must be exactly zero either way)
    cancels = [(d['x'].double().abs() * dpres[i].double().cpu().abs()).sum((0, 2, 3)) if dil >= H and dil >= W else None
               for i, dil in enumerate(dils)]
    dxb = bwd(dpres, 'multi backward on dL/dpre', rdx, rdw, cancels)
    dxa = bwd(dyc, 'multi backward, bnb', rdx, rdw, cancels, bnb=[(pres[i], recs[i]) for i in range(k)])
    assert torch.equal(dxa, dxb), 'multi-branch backward with BatchNorm backward on the fly: dx'


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('H,W,dils', MULTI)
@a_nc
def test_a_multi_branch(ops, N, C, H, W, dils, det):
    d = multi_data(N, C, H, W, dils)
    xd, dyd = d['x'].to(DEV), [t.to(DEV) for t in d['dys']]
    with det_mode(ops, det):
        multi_checks(ops, d, dils, xd, dyd, 'A', lambda: out_view((N, C, H, W)))
    report('A')


# ================================================================================================================== B: views and alignment
B_N, B_C = 2, 6
B_PLANES = [('plane3', 1, 1, 16, 20), ('plane1', 1, 4, 32, 32), ('strip1', 2, 4, 130, 132)]
b_planes = pytest.mark.parametrize('route,strips,dil,H,W', B_PLANES)
ROLES = ('x', 'out', 'dy', 'dx', 'pre')


def b_calls(ops, d, dil, t, det, group, routes):
    """forward, data gradient, fused backward (plain and bnb) and weight gradient on the operands t[role] (each a view, its guard in
    t[role + '_g'] where it is an output); routes = (conv route, folded route, strips) asserted for every call -> dict of results"""
    N, C, H, W = d['x'].shape
    wd = d['w'].to(DEV)
    route, fold, strips = routes
    r = {}
    with det_mode(ops, det):
        assert dw_route(ops, H, W, dil, [t['x'], t['out']]) == (route, strips)
        ops.dwconv(t['x'], wd, dil, out=t['out'])
        r['y'] = t['out'].clone()
        assert dw_route(ops, H, W, dil, [t['dy'], t['dx']]) == (route, strips)
        ops.dwconv(t['dy'], wd, dil, flip=True, out=t['dx'])
        r['dgrad'] = t['dx'].clone()
        t['dx'].fill_(3.0)
        dwg = DwGuard(C)
        assert dw_route(ops, H, W, dil, [t['dy'], t['dx'], t['x']]) == (route, strips)
        ops.dwconv_bwd_(dwg.dw, t['x'], t['dy'], wd, dil, t['dx'])
        dwg.intact('fused backward')
        r['dx'], r['dw'] = t['dx'].clone(), dwg.dw.clone()
        t['dx'].fill_(3.0)
        dwg = DwGuard(C)
        assert dw_route(ops, H, W, dil, [t['dyo'], t['dx'], t['x'], t['pre']], bnb=True) == (fold, strips)
        ops.dwconv_bwd_(dwg.dw, t['x'], t['dyo'], wd, dil, t['dx'], bnb=(t['pre'], t['rec']))
        dwg.intact('fused backward, bnb')
        r['dx_bnb'], r['dw_bnb'] = t['dx'].clone(), dwg.dw.clone()
        dwg = DwGuard(C)
        assert dw_route(ops, H, W, dil, [t['x'], t['dy']], wgrad=True) == (fold, strips)
        ops.dwconv_wgrad_(dwg.dw, t['x'], t['dy'], dil)
        dwg.intact('wgrad')
        r['wgrad'] = dwg.dw.clone()
    for key in ('out_g', 'dx_g'):
        t[key].intact(key)
    chan_close(r['y'], d['y'], FWD, group, 'forward')
    chan_close(r['dgrad'], d['dx'], FWD, group, 'dx')
    chan_close(r['dx'], d['dx'], FWD, group, 'dx')
    chan_close(r['dx_bnb'], t['ref_dx_bnb'], FWD, group, 'dx')
    chan_close(r['dw'], d['dw'], WGRAD, group, 'dw', cdim=0)
    chan_close(r['wgrad'], d['dw'], WGRAD, group, 'dw', cdim=0)
    chan_close(r['dw_bnb'], t['ref_dw_bnb'], WGRAD, group, 'dw', cdim=0)
    return r


_B_BASE = {}


def b_base(ops, dil, H, W):
    """the contiguous operands of one plane of group B, the bnb record and references, and the contiguous calls' results in both modes"""
    key = (dil, H, W)
    if key not in _B_BASE:
        d = case_data(B_N, B_C, dil, H, W)
        xd, wd, dyd = dev_inputs(d)
        pre, dyo, rec, dpre = bnb_setup(ops, d, xd, wd, dil)
        t = dict(x=xd, dy=dyd, dyo=dyo, pre=pre, rec=rec, ref_dx_bnb=ref_dx(d, dpre, dil), ref_dw_bnb=ref_dw(d['x'], d, dpre, dil))
        route, strips = dw_route(ops, H, W, dil, [xd])
        res = {}
        for det in (False, True):
            t['out_g'], t['out'] = out_view(xd.shape, front=0, back=0)
            t['dx_g'], t['dx'] = out_view(xd.shape, front=0, back=0)
            res[det] = b_calls(ops, d, dil, t, det, 'B', (route, folded(route), strips))
        _B_BASE[key] = (d, t, res)
    return _B_BASE[key]


@pytest.mark.parametrize('which', ROLES + ('all',))
@b_planes
def test_b_channel_slices(ops, route, strips, dil, H, W, which):
    """each operand in turn, then all, as channels [2, 2 + C) of a (C + 5)-channel buffer: batch stride (C + 5) H W, planes still aligned, so
    the vector routes stay; results bit-identical to the contiguous calls (weight gradients: in deterministic mode, where their order is fixed)"""
    d, base, res = b_base(ops, dil, H, W)
    shape = (B_N, B_C, H, W)
    t = dict(base)
    for role in ROLES:
        sliced = which in (role, 'all')
        gd = Guard(shape, front=2, back=3) if sliced else Guard(shape, front=0, back=0)
        assert gd.bs == ((B_C + 5) if sliced else B_C) * H * W
        if role in ('out', 'dx'):
            t[role], t[role + '_g'] = gd.view, gd
        else:
            t[role] = gd.put(base[role])
            if role == 'dy':
                t['dyo'] = Guard(shape, front=2, back=3).put(base['dyo']) if sliced else base['dyo']
    for det in (False, True):
        r = b_calls(ops, d, dil, t, det, 'B', (route, folded(route), strips))
        for key in ('y', 'dgrad', 'dx', 'dx_bnb') + (('dw', 'dw_bnb', 'wgrad') if det else ()):
            assert torch.equal(r[key], res[det][key]), f'{key} (deterministic {det}) differs from the contiguous call'
    report('B')


def test_b_multi_branch_on_slices(ops):
    """x, every dy and dx of the multi-branch launches as channel slices of (C + 5)-channel buffers: as the contiguous launches, bit for bit"""
    N, C, H, W, dils = B_N, B_C, 32, 32, (4, 8)
    d = multi_data(N, C, H, W, dils)
    shape = (N, C, H, W)
    wd = [w.to(DEV) for w in d['ws']]
    xs = Guard(shape, front=2, back=3).put(d['x'].to(DEV))
    dys = [Guard(shape, front=2, back=3).put(t.to(DEV)) for t in d['dys']]
    xc, dyc = d['x'].to(DEV), [t.to(DEV) for t in d['dys']]
    for det in (False, True):
        with det_mode(ops, det):
            multi_checks(ops, d, dils, xs, dys, 'B', lambda: out_view(shape, front=2, back=3))
            ya = [q[0] for q in ops.dwconv_multi(xs, wd, list(dils))]
            yb = [q[0] for q in ops.dwconv_multi(xc, wd, list(dils))]
            assert all(torch.equal(a, b) for a, b in zip(ya, yb))
            out = []
            for xx, dd, kw in ((xs, dys, dict(front=2, back=3)), (xc, dyc, dict(front=0, back=0))):
                gd, dx = out_view(shape, **kw)
                dws = [DwGuard(C) for _ in dils]
                ops.dwconv_multi_bwd_([q.dw for q in dws], xx, dd, wd, list(dils), dx)
                gd.intact('multi backward')
                out.append((dx, [q.dw for q in dws]))
            assert torch.equal(out[0][0], out[1][0])
            if det:
                assert all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
    report('B')


@pytest.mark.parametrize('kind', ['plane at 16k + 4 bytes', 'odd batch stride'])
@b_planes
def test_b_misaligned_operands_take_the_scalar_route(ops, route, strips, dil, H, W, kind):
    """W % 4 == 0, but one operand at a time starts 4 bytes past a 16-byte boundary, or has a batch stride of C H W + 1 floats (image 0
    aligned, image 1 not: stage_rows picks its copy per block): the call must land on strip0, match fp64 and keep its canaries.  In
    deterministic mode all variants of one call run the same kernel on the same slots, so their results are bit-identical to each other --
    an operand missing from the host's `vec` condition would run the vector kernel, whose weight-gradient sums are formed in another order"""
    d, base, res = b_base(ops, dil, H, W)
    assert W % 4 == 0 and route != 'strip0'
    shape = (B_N, B_C, H, W)
    kw = dict(front=1, back=3, lead=1) if kind.startswith('plane') else dict(front=0, back=0, odd=1)
    seen = {}
    for role in ROLES:
        t = dict(base)
        for r_ in ROLES:
            gd = Guard(shape, **kw) if r_ == role else Guard(shape)
            if r_ in ('out', 'dx'):
                t[r_], t[r_ + '_g'] = gd.view, gd
            else:
                t[r_] = gd.put(base[r_])
        t['dyo'] = Guard(shape, **(kw if role == 'dy' else {})).put(base['dyo'])
        bad = t[role]
        assert bad.data_ptr() % 16 != 0 or ops._bs(bad) % 4 != 0
        wd = d['w'].to(DEV)
        for det in (False, True):
            with det_mode(ops, det):
                if role in ('x', 'out'):
                    assert dw_route(ops, H, W, dil, [t['x'], t['out']]) == ('strip0', strips)
                    ops.dwconv(t['x'], wd, dil, out=t['out'])
                    t['out_g'].intact('forward')
                    chan_close(t['out'], d['y'], FWD, 'B', 'forward')
                    assert torch.equal(t['out'], res[det]['y'])          # the same fused multiply-adds in the same order on either route
                if role in ('dy', 'dx', 'x'):
                    dwg = DwGuard(B_C)
                    assert dw_route(ops, H, W, dil, [t['dy'], t['dx'], t['x']]) == ('strip0', strips)
                    ops.dwconv_bwd_(dwg.dw, t['x'], t['dy'], wd, dil, t['dx'])
                    t['dx_g'].intact('fused backward')
                    dwg.intact('fused backward')
                    chan_close(t['dx'], d['dx'], FWD, 'B', 'dx')
                    chan_close(dwg.dw, d['dw'], WGRAD, 'B', 'dw', cdim=0)
                    if det:
                        seen.setdefault('bwd', []).append((role, t['dx'].clone(), dwg.dw.clone()))
                if role != 'out':
                    dwg = DwGuard(B_C)
                    assert dw_route(ops, H, W, dil, [t['dyo'], t['dx'], t['x'], t['pre']], bnb=True) == ('strip0', strips)
                    ops.dwconv_bwd_(dwg.dw, t['x'], t['dyo'], wd, dil, t['dx'], bnb=(t['pre'], base['rec']))
                    t['dx_g'].intact('fused backward, bnb')
                    dwg.intact('fused backward, bnb')
                    chan_close(t['dx'], base['ref_dx_bnb'], FWD, 'B', 'dx')
                    chan_close(dwg.dw, base['ref_dw_bnb'], WGRAD, 'B', 'dw', cdim=0)
                    if det:
                        seen.setdefault('bnb', []).append((role, t['dx'].clone(), dwg.dw.clone()))
                if role in ('x', 'dy'):
                    dwg = DwGuard(B_C)
                    assert dw_route(ops, H, W, dil, [t['x'], t['dy']], wgrad=True) == ('strip0', strips)
                    ops.dwconv_wgrad_(dwg.dw, t['x'], t['dy'], dil)
                    dwg.intact('wgrad')
                    chan_close(dwg.dw, d['dw'], WGRAD, 'B', 'dw', cdim=0)
                    if det:
                        seen.setdefault('wgrad', []).append((role, None, dwg.dw.clone()))
    for call, runs in seen.items():
        for role, dx, dw in runs[1:]:
            assert dx is None or torch.equal(dx, runs[0][1]), f'{call}: dx with a misaligned {role} differs from that with a misaligned {runs[0][0]}'
            assert torch.equal(dw, runs[0][2]), f'{call}: dw with a misaligned {role} differs from that with a misaligned {runs[0][0]}'
    key = {'bwd': 'dw', 'bnb': 'dw_bnb', 'wgrad': 'wgrad'}
    print('scalar-route weight gradients differ bitwise from the vector route\'s (deterministic mode):',
          {call: not torch.equal(runs[0][2], res[True][key[call]]) for call, runs in seen.items()})
    # the multi-branch kernels have no scalar form: such an input must be refused up front
    xm = Guard(shape, **kw).put(base['x'])
    assert ops.dwconv_multi_ok(base['x'], [4, 8]) == (H * W * 4 <= LDS) and not ops.dwconv_multi_ok(xm, [4, 8])
    report('B')


def test_b_wgrad_refuses_a_batch_stride_below_one_image(ops):
    """pfst_dwconv3x3_wgrad checks its strides like its siblings: images that overlap are an argument error, not a launch"""
    from pfst_amd._lib import PfstHipError
    N, C, H, W = 2, 6, 16, 20
    x, dy = torch.randn(N, C, H, W, generator=g(1)).to(DEV), torch.randn(N, C, H, W, generator=g(3)).to(DEV)
    dwg = DwGuard(C)
    st = torch.cuda.current_stream().cuda_stream
    for x_bs, dy_bs in ((C * H * W - 4, C * H * W), (C * H * W, C * H * W - 4)):
        with pytest.raises(PfstHipError, match='_bs >= '):
            ops.call('pfst_dwconv3x3_wgrad', x.data_ptr(), x_bs, dy.data_ptr(), dy_bs, dwg.dw.data_ptr(), N, C, H, W, 1, st)
    torch.cuda.synchronize()
    assert float(dwg.dw.abs().max()) == 0.0
    dwg.intact()
    ops.call('pfst_dwconv3x3_wgrad', x.data_ptr(), C * H * W, dy.data_ptr(), C * H * W, dwg.dw.data_ptr(), N, C, H, W, 1, st)
    assert float(dwg.dw.abs().max()) > 0.0


# ================================================================================================================= C: strips at the clamp
C_N, C_C = 1, 3
# (dil, H, W, route, strips, rows staged at most)
C_CASES = [(16, 40, 512, 'strip1', 40, 33),    # 64 KiB / (4 W) - 2 dil = 0 -> one row per strip; its 33-row halo is clipped top and bottom
           (12, 40, 512, 'strip1', 5, 32),     # 8 rows per strip
           (16, 40, 510, 'strip0', 40, 33),    # the same clamp on the scalar kernel
           (1, 136, 128, 'strip3', 2, 128),    # control
           # 16 - 72 rows -> one row per strip, and the 73-row halo is clipped to the 20-row plane: 80 KiB staged, NOT refused (see the refusal test)
           (36, 20, 1024, 'strip1', 20, 20),
           # a two-row plane above 64 KiB -> one row per strip, two rows staged: 4100 quads per strip, more than the 8 x 512 the weight-gradient
           # kernel keeps in registers, so its second loop (quads from memory) runs -- reachable only with W > 16384
           (1, 2, 16400, 'strip3', 2, 2),
           (4, 2, 16400, 'strip1', 2, 2)]


@pytest.mark.parametrize('dil,H,W,route,strips,staged', C_CASES)
def test_c_strips_at_the_clamp(ops, dil, H, W, route, strips, staged):
    d = case_data(C_N, C_C, dil, H, W)
    xd, wd, dyd = dev_inputs(d)
    shape = (C_N, C_C, H, W)
    assert H * W * 4 > LDS and cdiv(H, strip_rows(H, W, dil)) == strips and strip_lds(H, W, dil) == staged * W * 4 <= 150 * 1024
    assert ops.lib().pfst_dwconv_stats_slots(H, W, dil) == strips          # the library's strip count is the helper's
    gd, out = out_view(shape)
    assert dw_route(ops, H, W, dil, [xd, out]) == (route, strips)
    sent_scratch(ops, xd.device, 'stats', 4 * C_C * C_N * strips, ops._STATS_FLOOR)
    y, st, sl = ops.dwconv(xd, wd, dil, out=out, want_stats=True, want_minmax=True)
    assert sl == C_N * strips
    chan_close(y, d['y'], FWD, 'C', 'forward')
    gd.intact('forward')
    check_partials(ops, y, st, sl, C_N * H * W, d['y'], 'C')
    for det in (False, True):
        backward_calls(ops, d, dil, 'C', route, strips, det)
    report('C')


def test_c_a_strip_beyond_the_lds_limit_is_refused(ops):
    """W = 1024, dil = 36: one row per strip and a halo of 72 rows.  With H = 80 the staged strip is 73 rows x 4 KiB = 292 KiB, above the
    150 KiB the kernels may ask for: the argument check refuses it and no kernel runs.  (With H = 20 the halo is clipped to the plane:
    strip_lds gives 20 rows = 80 KiB, the launch is legal -- that shape is the last row of C_CASES and must compute, not raise.)"""
    from pfst_amd._lib import PfstHipError
    dil, H, W = 36, 80, 1024
    assert strip_rows(H, W, dil) == 1 and strip_lds(H, W, dil) == 73 * W * 4 > 150 * 1024
    assert strip_lds(20, W, dil) == 20 * W * 4 <= 150 * 1024
    shape = (C_N, C_C, H, W)
    x = torch.randn(shape, generator=g(1)).to(DEV)
    w = torch.randn(C_C, 1, 3, 3, generator=g(2)).to(DEV)
    gd, out = out_view(shape)
    out.fill_(SENT)
    with pytest.raises(PfstHipError, match='lds <= 150'):
        ops.dwconv(x, w, dil, out=out)
    dwg = DwGuard(C_C)
    with pytest.raises(PfstHipError, match='lds <= 150'):
        ops.dwconv_bwd_(dwg.dw, x, x, w, dil, out)
    with pytest.raises(PfstHipError, match='lds <= 150'):
        ops.dwconv_wgrad_(dwg.dw, x, x, dil)
    torch.cuda.synchronize()
    assert bool((gd.flat == SENT).all()) and float(dwg.dw.abs().max()) == 0.0
    dwg.intact()


# ============================================================================================================ D: dilation beyond the plane
@pytest.mark.parametrize('dil,H,W,route', [(40, 24, 40, 'plane1'), (9, 7, 9, 'strip0')])
def test_d_dilation_beyond_the_plane(ops, dil, H, W, route):
    """every outer tap falls outside the plane: y = w[c, 1, 1] x and dx = w[c, 1, 1] dy as ONE rounded product each (a fused multiply-add
    onto zero), the eight outer weight gradients exactly zero, the centre one = sum x dy"""
    N, C = 2, 5
    assert dil >= H and dil >= W
    d = case_data(N, C, dil, H, W)
    xd, wd, dyd = dev_inputs(d)
    shape = (N, C, H, W)
    centre = wd[:, 0, 1, 1].view(1, C, 1, 1)
    gd, out = out_view(shape)
    assert dw_route(ops, H, W, dil, [xd, out]) == (route, 1)
    ops.dwconv(xd, wd, dil, out=out)
    assert torch.equal(out, centre * xd)
    gd.intact('forward')
    gd, dx = out_view(shape)
    ops.dwconv(dyd, wd, dil, flip=True, out=dx)
    assert torch.equal(dx, centre * dyd)
    gd.intact('data gradient')
    outer = torch.ones(3, 3, dtype=torch.bool)
    outer[1, 1] = False
    sxy = (d['x'].double() * d['dy'].double()).sum((0, 2, 3))
    for det in (False, True):
        with det_mode(ops, det):
            for fused in (False, True):
                dwg = DwGuard(C)
                if fused:
                    gd, dx = out_view(shape)
                    ops.dwconv_bwd_(dwg.dw, xd, dyd, wd, dil, dx)
                    assert torch.equal(dx, centre * dyd)
                    gd.intact('fused backward')
                else:
                    ops.dwconv_wgrad_(dwg.dw, xd, dyd, dil)
                dwg.intact()
                dwc = dwg.dw.cpu()
                assert bool((dwc[:, 0][:, outer] == 0.0).all()), 'an outer tap received a weight gradient'
                chan_close(dwc[:, 0, 1, 1].view(C, 1), sxy.view(C, 1), WGRAD, 'D', 'dw', cdim=0)
                chan_close(dwc, d['dw'], WGRAD, 'D', 'dw', cdim=0)
    report('D')
