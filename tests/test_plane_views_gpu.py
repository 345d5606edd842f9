"""The plane kernels of csrc/spatial.hip that read or write channel slices of concat buffers in models.py -- global_avgpool, reduce_hw,
broadcast_hw (scale, accumulate, amax), resize_bilinear and resize_bilinear_bwd (write and accumulate) -- on operands that are views:
(i) channels [2, 2 + C) of a (C + 5)-channel buffer, (ii) planes 4 bytes past a 16-byte boundary, (iii) an odd batch stride; each operand
in turn, then all.  Outputs sit in canary buffers (helpers.Guard), the parent buffers of inputs must come back unchanged.

The two resize entry points choose among five kernels on the host (spatial.hip, pfst_resize_bilinear and pfst_resize_bilinear_bwd): the
conditions are restated in resize_route / resize_bwd_route, every launch asserts the route its operands meet, and test_every_route_is_reached
asserts that the cases of this file reach all five.

References: F.interpolate in fp64 and its autograd, x.double() sums.  Bounds (reasoned, not fitted):
  resize forward   2^-24 A (12 max(Hi, Wi) d + 4), A = max |x| of the plane: the source coordinate s (o + 0.5) - 0.5 takes three fp32 roundings
                   of values up to the input size, so each of the two weights is off by at most 3 2^-24 max(Hi, Wi), and the blend moves by at
                   most 2 A per unit of either weight; three roundings of the blend and one of 1 - lambda on values up to A.  d = 0 at the
                   exact scale 1/2 (coordinates and weights exact), else 1.
  resize backward  2^-24 B (150 max(Hi, Wi) d + 270), B = max |dy| of the plane: at most 25 taps reach an input pixel at these scales, each
                   weight a product of two factors off by 3 2^-24 max(Hi, Wi) at most; at most 30 fused multiply-adds round partial sums that are at
                   most 9 B (the weights of a pixel sum to at most 9 at the border of the largest scale here).
  plane mean       2^-23 |ref| + 1e-10 (fp64 sum, one rounding of 1 / HW and one of the result: the depthwise test's bound for its fused mean);
                   the plain sum likewise.
  broadcast_hw     bit-equal to v * scale (one fp32 product), accumulated: one more fp32 add; the published maximum exact.
On top of the bounds every launch on views is bit-equal to the contiguous launch, whichever kernel it reaches: the x2 kernels evaluate the
generic kernels' expressions (bilin_blend forward; in the adjoints one rounded product and fused multiply-adds per row of taps, rows folded
in ascending order, zero-weight taps adding nothing)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_batchnorm_edges_gpu import KINDS, Operands
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, C = 3, 5
U24 = 2.0 ** -24
PLANES = [(1, 1), (9, 11), (16, 16)]
RESIZES = [((6, 10), (12, 20)), ((8, 8), (16, 16)), ((5, 7), (13, 9)), ((7, 6), (14, 12))]       # the last: odd Hi, the one-pixel x2 adjoint
kinds = pytest.mark.parametrize('kind', list(KINDS))


# ------------------------------------------------------------------------------------------------------------- the host's choice, restated
def resize_route(ops, x, y):
    """pfst_resize_bilinear: the x2 kernel (8-byte loads, 16-byte stores) or the generic gather"""
    (Hi, Wi), (Ho, Wo) = x.shape[2:], y.shape[2:]
    if (Ho == 2 * Hi and Wo == 2 * Wi and Hi > 1 and Wi > 1 and Wi % 2 == 0 and ops._bs(x) % 2 == 0 and ops._bs(y) % 4 == 0
            and x.data_ptr() % 8 == 0 and y.data_ptr() % 16 == 0):
        return 'fwd 2x'
    return 'fwd generic'


def resize_bwd_route(ops, dy, dx):
    """pfst_resize_bilinear_bwd: 2 x 2 input pixels per thread (16-byte loads of dy), one input pixel per thread (8-byte loads), or generic"""
    (Hi, Wi), (Ho, Wo) = dx.shape[2:], dy.shape[2:]
    two = Ho == 2 * Hi and Wo == 2 * Wi and Hi > 1 and Wi > 1
    if two and Hi % 2 == 0 and Wi % 2 == 0 and ops._bs(dy) % 4 == 0 and ops._bs(dx) % 2 == 0 and dy.data_ptr() % 16 == 0 and dx.data_ptr() % 8 == 0:
        return 'bwd 2x2 blocks'
    if two and ops._bs(dy) % 2 == 0 and dy.data_ptr() % 8 == 0:
        return 'bwd 2x'
    return 'bwd generic'


ROUTES = {'fwd 2x', 'fwd generic', 'bwd 2x2 blocks', 'bwd 2x', 'bwd generic'}
VIEWED = [('in',), ('out',), ('in', 'out')]


def resize_operands(kind, viewed, hi, ho):
    o = Operands(kind, viewed, (N, C) + hi)
    o2 = Operands(kind, viewed, (N, C) + ho)
    return o, o2


# ------------------------------------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def resize_case(hi, ho):
    x = (torch.randn((N, C) + hi, generator=g(1)) * 3).double().requires_grad_()
    y = F.interpolate(x, size=ho, mode='bilinear', align_corners=False)
    dy = torch.randn((N, C) + ho, generator=g(2))
    y.backward(dy.double())
    d = 0 if (ho[0] == 2 * hi[0] and ho[1] == 2 * hi[1]) else 1
    A = x.detach().abs().amax((2, 3), keepdim=True)
    B = dy.double().abs().amax((2, 3), keepdim=True)
    return dict(x=x.detach().float(), dy=dy, y=y.detach(), dx=x.grad, old=torch.randn((N, C) + hi, generator=g(3)),
                tol_y=U24 * A * (12 * max(hi) * d + 4), tol_dx=U24 * B * (150 * max(hi) * d + 270))


_CONTIG = {}


def contiguous(ops, hi, ho):
    """the launches on plain tensors, held to the fp64 references once"""
    if (hi, ho) not in _CONTIG:
        d = resize_case(hi, ho)
        xd, dyd, old = d['x'].to(DEV), d['dy'].to(DEV), d['old'].to(DEV)
        y = ops.resize_bilinear(xd, ho)
        dx = ops.resize_bilinear_bwd(dyd, hi)
        acc = ops.resize_bilinear_bwd(dyd, hi, out=old.clone(), accumulate=True)
        for got, ref, tol, what in ((y, d['y'], d['tol_y'], 'forward'), (dx, d['dx'], d['tol_dx'], 'adjoint'),
                                    (acc, d['dx'] + d['old'].double(), d['tol_dx'] + U24 * (d['dx'] + d['old'].double()).abs(), 'adjoint, accumulated')):
            err = (got.double().cpu() - ref).abs()
            print(f'resize {hi} -> {ho} {what}: worst error / bound {float((err / tol).max()):.3g}')
            assert bool((err <= tol).all()), f'resize {hi} -> {ho} {what}: {float((err / tol).max()):.3g} x the bound'
        assert torch.equal(acc, old + dx)
        _CONTIG[hi, ho] = dict(x=xd, dy=dyd, old=old, y=y, dx=dx, acc=acc)
    return _CONTIG[hi, ho]


def route_of(ops, hi, ho, kind, viewed, bwd):
    """the route a case reaches (the views are only allocated)"""
    oi, oo = resize_operands(kind, viewed, hi, ho)
    if bwd:
        return resize_bwd_route(ops, oo.dst('in'), oi.dst('out'))
    return resize_route(ops, oi.dst('in'), oo.dst('out'))


def test_every_route_is_reached(ops):
    seen = {route_of(ops, hi, ho, kind, viewed, bwd) for hi, ho in RESIZES for kind in KINDS for viewed in VIEWED + [()] for bwd in (False, True)}
    assert seen == ROUTES, ROUTES - seen
    # and the ones each view kind is here for
    assert route_of(ops, (8, 8), (16, 16), 'slice', ('in', 'out'), False) == 'fwd 2x'
    assert route_of(ops, (8, 8), (16, 16), 'slice', ('in', 'out'), True) == 'bwd 2x2 blocks'
    assert route_of(ops, (7, 6), (14, 12), 'slice', ('in', 'out'), True) == 'bwd 2x'
    assert route_of(ops, (8, 8), (16, 16), 'lead', ('in',), False) == 'fwd generic' == route_of(ops, (8, 8), (16, 16), 'odd', ('out',), False)
    assert route_of(ops, (8, 8), (16, 16), 'lead', ('in',), True) == 'bwd generic'
    assert route_of(ops, (8, 8), (16, 16), 'lead', ('out',), True) == 'bwd 2x'          # dx 4 bytes past: no 8-byte stores, dy still aligned
    assert route_of(ops, (5, 7), (13, 9), 'slice', (), False) == 'fwd generic'


@pytest.mark.parametrize('viewed', VIEWED)
@kinds
@pytest.mark.parametrize('hi,ho', RESIZES)
def test_resize_on_views(ops, hi, ho, kind, viewed):
    d = contiguous(ops, hi, ho)
    twice = ho[0] == 2 * hi[0] and ho[1] == 2 * hi[1]
    # forward
    oi, oo = resize_operands(kind, viewed, hi, ho)
    xv, yv = oi.src('in', d['x']), oo.dst('out')
    route = resize_route(ops, xv, yv)
    assert route == ('fwd 2x' if twice and hi[1] % 2 == 0 and kind == 'slice' else 'fwd generic') or (kind == 'odd' and twice)
    ops.resize_bilinear(xv, ho, out=yv)
    oi.check(f'resize_bilinear ({route})'), oo.check(f'resize_bilinear ({route})')
    assert torch.equal(yv, d['y']), f'{route}: differs from the contiguous launch'
    # adjoint, written and accumulated
    for acc in (False, True):
        oi, oo = resize_operands(kind, viewed, hi, ho)
        gv, dv = oo.src('in', d['dy']), oi.dst('out', d['old'] if acc else None)
        route = resize_bwd_route(ops, gv, dv)
        assert twice or route == 'bwd generic'
        ops.resize_bilinear_bwd(gv, hi, out=dv, accumulate=acc)
        oi.check(f'resize_bilinear_bwd ({route})'), oo.check(f'resize_bilinear_bwd ({route})')
        assert torch.equal(dv, d['acc'] if acc else d['dx']), f'{route} accumulate={acc}: differs from the contiguous launch'


@functools.lru_cache(maxsize=None)
def plane_case(H, W):
    ch = torch.arange(C, dtype=torch.float32).view(1, C, 1, 1)
    x = torch.randn(N, C, H, W, generator=g(1)) * (1 + 0.5 * ch) + 0.3 * torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1) - 0.2 * ch
    return x, torch.randn(N, C, generator=g(2)) * 2, torch.randn(N, C, H, W, generator=g(3))


@kinds
@pytest.mark.parametrize('H,W', PLANES)
def test_plane_sums_on_views(ops, H, W, kind):
    x, _, _ = plane_case(H, W)
    o = Operands(kind, ('x',), x.shape)
    xv = o.src('x', x.to(DEV))
    mean, tot = ops.global_avgpool(xv), ops.reduce_hw(xv)
    o.check('global_avgpool / reduce_hw')
    assert tuple(mean.shape) == tuple(tot.shape) == (N, C, 1, 1)
    for got, ref in ((mean, x.double().mean((2, 3))), (tot, x.double().sum((2, 3)))):
        err = (got.double().cpu().view(N, C) - ref).abs()
        assert bool((err <= 2.0 ** -23 * ref.abs() + 1e-10).all()), (err / ref.abs()).tolist()


@kinds
@pytest.mark.parametrize('H,W', PLANES)
def test_broadcast_on_views(ops, H, W, kind):
    _, v, old = plane_case(H, W)
    vd, oldd = v.to(DEV), old.to(DEV)
    scale = 0.37
    val = (vd * torch.tensor(scale, device=DEV)).view(N, C, 1, 1)          # one fp32 product, as in the kernel
    o = Operands(kind, ('out',), old.shape)
    ov = o.dst('out')
    am = ops.amax_slots(vd.device)
    ops.broadcast_hw(vd, ov, scale, amax=am)
    o.check('broadcast_hw')
    assert torch.equal(ov, val.expand(N, C, H, W))
    assert float(am.max()) == float(val.abs().max())
    o = Operands(kind, ('out',), old.shape)
    ov = o.dst('out', oldd)
    ops.broadcast_hw(vd, ov, scale, accumulate=True)
    o.check('broadcast_hw, accumulate')
    assert torch.equal(ov, oldd + val)
