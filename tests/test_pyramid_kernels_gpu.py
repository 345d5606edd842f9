"""The plane <-> pyramid-of-small-grids kernels (csrc/pyramid.hip: pfst_pyramid_reduce, pfst_pyramid_expand, pfst_copy_planes) through their four
wrappers -- pyramid_pool, pyramid_pool_bwd, pyramid_upsample, pyramid_upsample_bwd -- against fp64 torch on the CPU: F.adaptive_avg_pool2d and
F.interpolate(mode='bilinear', align_corners=False) forward, and their autograd backward.

Bound, element-wise and DERIVED (nothing here was measured first): |got - ref| <= (n + 8) 2^-24 sum |terms|, n the number of non-zero terms
(weight_row x value x weight_column products, plus the accumulated / added operands) of that output and the sum of their magnitudes taken in
fp64 -- the worst case of an n-term fp32 sum in any order, (n - 1) u sum |terms|, plus the roundings of the two fp32 weights and of their
product with the value (3 u), with room to spare.  The terms come from the host's fp64 operator tables (hip_ops.pyramid_operator), which
tests/test_baseline_heads_cpu.py holds against torch to 1e-14.

Views: every input is a channel slice of a wider buffer whose other floats are NaN (a read outside the view poisons the result); every output
lies in a SENT-filled buffer that must come back untouched outside the view.  Accumulate on and off, the published maximum exact, two runs
bit-identical.

MEASURED on an MI355X, worst ratio to the bound (1.0 would fail): pool 0.13, pool backward 0.21, upsample 0.25, upsample backward 0.19."""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import SENT, Guard

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
U = 2.0 ** -24
DEFAULT = (1, 2, 3, 6)
# (N, C, H, W, scales): ragged with overlapping bins; smaller than a scale; several row chunks of the expand kernel and an odd width; the
# full-plane form (two 64-row chunks of the reduce kernel, the float4 staging); the largest grid
CASES = [(2, 5, 13, 10, DEFAULT), (2, 5, 5, 7, DEFAULT), (2, 5, 33, 47, DEFAULT), (1, 8, 128, 128, DEFAULT), (2, 5, 13, 10, (4, 8))]
IDS = ['13x10', '5x7', '33x47', '128x128', '13x10-s48']


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from pfst_amd import hip_ops
    return hip_ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def operators(kind, h, w, scales):
    from pfst_amd.hip_ops import pyramid_operator
    dh, dw = pyramid_operator(kind, h, scales)[0], pyramid_operator(kind, w, scales)[0]
    out, o = [], 0
    for s in scales:
        out.append((torch.from_numpy(dh[o:o + s]), torch.from_numpy(dw[o:o + s])))
        o += s
    return out


def reduce_bound(kind, planes, scales):
    """planes[k]: the fp64 [N, C, H, W] operand of scale k -> per scale the (n + 8) u sum |terms| of every cell"""
    h, w = planes[0].shape[2:]
    res = []
    for (dh, dw), x in zip(operators(kind, h, w, scales), planes):
        mag = torch.einsum('iy,ncyx,jx->ncij', dh.abs(), x.abs(), dw.abs())
        cnt = torch.einsum('iy,ncyx,jx->ncij', (dh != 0).double(), (x != 0).double(), (dw != 0).double())
        res.append((cnt + 8) * U * mag)
    return res


def expand_terms(kind, grids, hw, scales):
    """per scale (sum |terms|, number of non-zero terms) of every output pixel"""
    res = []
    for (dh, dw), gk in zip(operators(kind, hw[0], hw[1], scales), grids):
        mag = torch.einsum('iy,ncij,jx->ncyx', dh.abs(), gk.abs(), dw.abs())
        cnt = torch.einsum('iy,ncij,jx->ncyx', (dh != 0).double(), (gk != 0).double(), (dw != 0).double())
        res.append((mag, cnt))
    return res


def held(got, ref, bound, what):
    err = (got.detach().double().cpu() - ref).abs()
    assert torch.isfinite(got).all(), f'{what}: not finite (a NaN from outside the view reached the result?)'
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: worst |got - ref| / bound = {ratio:.3g}')
    assert bool((err <= bound).all()), f'{what}: {ratio:.3g} x the bound'


def nan_slice(t, front=2, back=3):
    """t on the device as channels [front, front + C) of a buffer that is NaN everywhere else"""
    gd = Guard(tuple(t.shape), front=front, back=back, fill=NAN)
    gd.put(t.to(DEV))
    return gd


def flat_guard(numel):
    buf = torch.full((numel + 128,), SENT, device=DEV)
    return buf, buf[64:64 + numel]


def flat_intact(buf, numel, what):
    assert bool((buf[:64] == SENT).all()) and bool((buf[64 + numel:] == SENT).all()), f'{what}: floats outside the output were written'


@functools.lru_cache(maxsize=None)
def pool_case(n, c, h, w, scales):
    x = torch.randn(n, c, h, w, generator=gen(1)) + 0.3
    gs = [torch.randn(n, c, s, s, generator=gen(2 + s)) for s in scales]
    old = torch.randn(n, c, h, w, generator=gen(20))
    add = torch.randn(n, c, h, w, generator=gen(21))
    x64 = x.double().requires_grad_(True)
    pooled = [F.adaptive_avg_pool2d(x64, s) for s in scales]
    sum((p * g.double()).sum() for p, g in zip(pooled, gs)).backward()
    return x, gs, old, add, [p.detach() for p in pooled], x64.grad


@functools.lru_cache(maxsize=None)
def up_case(n, c, h, w, scales):
    gs = [torch.randn(n, c, s, s, generator=gen(30 + s)) + 0.2 for s in scales]
    dy = torch.randn(n, c * len(scales), h, w, generator=gen(40))
    g64 = [g.double().requires_grad_(True) for g in gs]
    ups = [F.interpolate(g, (h, w), mode='bilinear', align_corners=False) for g in g64]
    (torch.cat(ups, 1) * dy.double()).sum().backward()
    return gs, dy, torch.cat([u.detach() for u in ups], 1), [g.grad for g in g64]


@pytest.mark.parametrize('n,c,h,w,scales', CASES, ids=IDS)
def test_pyramid_pool(ops, n, c, h, w, scales):
    x, _, _, _, ref, _ = pool_case(n, c, h, w, scales)
    src = nan_slice(x)
    cells = n * c * sum(s * s for s in scales)
    buf, flat = flat_guard(cells)
    outs = ops.pyramid_pool(src.view, scales, out=flat)
    bounds = reduce_bound('pool', [x.double()] * len(scales), scales)
    for s, o, r, b in zip(scales, outs, ref, bounds):
        assert tuple(o.shape) == (n, c, s, s) and o.is_contiguous()
        held(o, r, b, f'pool {h}x{w} -> {s}')
    flat_intact(buf, cells, 'pyramid_pool')
    again = ops.pyramid_pool(src.view, scales)
    assert all(torch.equal(a, b) for a, b in zip(again, outs)), 'two runs differ'


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('n,c,h,w,scales', CASES, ids=IDS)
def test_pyramid_pool_bwd(ops, n, c, h, w, scales, accumulate):
    _, gs, old, add, _, ref = pool_case(n, c, h, w, scales)
    terms = expand_terms('pool', [g.double() for g in gs], (h, w), scales)
    mag, cnt = sum(t[0] for t in terms), sum(t[1] for t in terms)
    grids = [g.to(DEV) for g in gs]
    for with_add in (False, True):
        r, m, k = ref.clone(), mag.clone(), cnt.clone()
        if with_add:
            r, m, k = r + add.double(), m + add.double().abs(), k + 1
        if accumulate:
            r, m, k = r + old.double(), m + old.double().abs(), k + 1
        res = []
        for _ in range(2):
            gd = Guard((n, c, h, w))
            gd.put(old.to(DEV) if accumulate else torch.full((n, c, h, w), NAN, device=DEV))
            ops.pyramid_pool_bwd(grids, scales, gd.view, accumulate=accumulate, add=nan_slice(add).view if with_add else None)
            gd.intact('pyramid_pool_bwd')
            res.append(gd.view.clone())
        held(res[0], r, (k + 8) * U * m, f'pool backward {h}x{w} add={with_add} accumulate={accumulate}')
        assert torch.equal(res[0], res[1]), 'two runs differ'


@pytest.mark.parametrize('n,c,h,w,scales', CASES, ids=IDS)
def test_pyramid_upsample(ops, n, c, h, w, scales):
    gs, _, ref, _ = up_case(n, c, h, w, scales)
    terms = expand_terms('bilinear', [g.double() for g in gs], (h, w), scales)
    bound = torch.cat([(k + 8) * U * m for m, k in terms], 1)
    grids = [g.to(DEV) for g in gs]
    res = []
    for _ in range(2):
        # the pyramid's slices of a concat: 3 channels of something else in front (SENT here), canaries behind
        gd = Guard((n, c * len(scales), h, w), front=3)
        amax = ops.amax_slots(torch.device(DEV))
        ops.pyramid_upsample(grids, scales, gd.view, amax=amax)
        gd.intact('pyramid_upsample')
        assert float(amax.max()) == float(gd.view.abs().max()), 'the published maximum is not max |y| of the written slices'
        res.append(gd.view.clone())
    held(res[0], ref, bound, f'upsample -> {h}x{w}')
    assert torch.equal(res[0], res[1]), 'two runs differ'


@pytest.mark.parametrize('n,c,h,w,scales', CASES, ids=IDS)
def test_pyramid_upsample_bwd(ops, n, c, h, w, scales):
    _, dy, _, ref = up_case(n, c, h, w, scales)
    src = nan_slice(dy)
    cells = n * c * sum(s * s for s in scales)
    buf, flat = flat_guard(cells)
    outs = ops.pyramid_upsample_bwd(src.view, scales, out=flat)
    bounds = reduce_bound('bilinear', [dy[:, k * c:(k + 1) * c].double() for k in range(len(scales))], scales)
    for s, o, r, b in zip(scales, outs, ref, bounds):
        assert tuple(o.shape) == (n, c, s, s)
        held(o, r, b, f'upsample backward {h}x{w} -> {s}')
    flat_intact(buf, cells, 'pyramid_upsample_bwd')
    again = ops.pyramid_upsample_bwd(src.view, scales)
    assert all(torch.equal(a, b) for a, b in zip(again, outs)), 'two runs differ'


def test_copy_planes_into_a_slice(ops):
    x = torch.randn(2, 5, 7, 9, generator=gen(50))
    for shape in ((2, 5, 7, 9), (2, 4, 8, 8)):          # scalar and float4 form
        x = torch.randn(*shape, generator=gen(50))
        src, dst = nan_slice(x), Guard(shape)
        amax = ops.amax_slots(torch.device(DEV))
        ops.copy_planes(src.view, dst.view, amax=amax)
        dst.intact('copy_planes')
        assert torch.equal(dst.view.cpu(), x) and float(amax.max()) == float(x.abs().max())


def test_scales_outside_the_kernels_are_refused(ops):
    x = torch.zeros(1, 2, 8, 8, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.pyramid_pool(x, (1, 9))
    with pytest.raises(NotImplementedError):
        ops.pyramid_pool(x, (1, 2, 3, 4, 5, 6, 7))
