"""The feature-pyramid kernels of csrc/fpn.hip -- topdown_merge, fpn_resize_concat, fpn_resize_concat_bwd -- against the compositions of the
existing ops they replace and against fp64, on operands that are views inside canary buffers (helpers.Guard): (i) channels [2, 2 + C) of a
(C + 5)-channel buffer, (ii) planes 4 bytes past a 16-byte boundary, (iii) an odd batch stride; N = 2, C = 3 and 5.  Inputs must come back
unchanged, nothing outside an output view may be written.

Checks:
  * torch.equal against resize_bilinear + one fp32 add (merge), resize_bilinear(out=slice) per level (concat) and resize_bilinear_bwd per level,
    written and accumulated (concat_bwd): the kernels promise the same bits whichever form the host chooses;
  * the published maximum equals out.abs().max() exactly;
  * against F.interpolate in fp64 and its autograd, with the resize bounds of tests/test_plane_views_gpu.py (reasoned there):
      forward   2^-24 A (12 max(Hc, Wc) d + 4), A = max |coarse| of the plane, d = 0 at the exact scale 1/2, else 1;
                the merge adds one rounding of a sum of magnitude at most |lat| + A: + 2^-24 (|lat| + A);
      adjoint   2^-24 B (6 max(Hc, Wc) d T + (T + t_y) S), B = max |dy| of the plane.  That file's 150 max(Hi, Wi) d + 270 is this with its
                T = 25 taps, 30 fused multiply-adds and weight sum 9; the concat reaches coarser levels (3 x 3 -> 19 x 17), so here the
                counts follow the scale: t = ceil(2 Hf / Hc) + 1 taps per axis can reach a source pixel, T = t_y t_x, each weight a product
                of two factors off by 3 2^-24 max(Hc, Wc); T + t_y fused multiply-adds round partial sums of at most S B, S the largest
                total weight a source pixel receives, taken exactly from the fp64 adjoint of a plane of ones (4 at x2);
  * every form the host chooses among (hip_ops.MERGE_ROUTES, the two concat forms, the two adjoint forms) is reached by these cases."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import Guard
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N = 2
U24 = 2.0 ** -24
KINDS = {'plain': dict(front=0, back=0), 'slice': dict(front=2, back=3), 'lead': dict(front=1, back=3, lead=1), 'odd': dict(front=0, back=0, odd=1)}
# (9, 40) -> (17, 80): rows wider than a wavefront (80 pixels on the one-pixel form, 20 quads on the four-pixel one: a wave spans several rows).
# (2, 130) -> (4, 260): 65 quads per row, the exact-1/2 walk's second trip of a wave over its row
MERGES = [((1, 1), (2, 2)), ((3, 3), (5, 5)), ((5, 5), (10, 9)), ((10, 9), (19, 17)), ((4, 6), (8, 12)), ((8, 8), (16, 16)), ((9, 40), (17, 80)),
          ((2, 130), (4, 260))]
CONCATS = [(((10, 9), (5, 5), (3, 3)), (19, 17)), (((8, 8), (4, 4), (2, 2)), (16, 16)), (((5, 5),), (10, 9))]
channels = pytest.mark.parametrize('C', [3, 5])


def view(shape, kind, t=None):
    gd = Guard(shape, **KINDS[kind])
    if t is not None:
        gd.put(t)
    return gd


def unchanged(gd, before, what):
    assert torch.equal(gd.flat, before), f'{what}: a read-only operand was written'


def fwd_tol(coarse, hc, hf):
    d = 0 if (hf[0] == 2 * hc[0] and hf[1] == 2 * hc[1]) else 1
    A = coarse.double().abs().amax((2, 3), keepdim=True)
    return U24 * A * (12 * max(hc) * d + 4), A


def bwd_tol(dy, hc, hf):
    d = 0 if (hf[0] == 2 * hc[0] and hf[1] == 2 * hc[1]) else 1
    ty, tx = math.ceil(2 * hf[0] / hc[0]) + 1, math.ceil(2 * hf[1] / hc[1]) + 1
    one = torch.zeros(1, 1, *hc, dtype=torch.float64, requires_grad=True)
    F.interpolate(one, size=hf, mode='bilinear', align_corners=False).sum().backward()
    S = float(one.grad.max())
    B = dy.double().abs().amax((2, 3), keepdim=True)
    return U24 * B * (6 * max(hc) * d * ty * tx + (ty * tx + ty) * S)


# ------------------------------------------------------------------------------------------------------------------------------------ merge
@functools.lru_cache(maxsize=None)
def merge_case(hc, hf, C):
    """inputs, the composition of the existing ops on plain tensors (held to fp64 once) and its maximum"""
    from pfst_amd import hip_ops
    coarse = torch.randn((N, C) + hc, generator=g(11)) * 3
    lat = torch.randn((N, C) + hf, generator=g(12)) * 2
    ref = F.interpolate(coarse.double(), size=hf, mode='bilinear', align_corners=False) + lat.double()
    cd, ld = coarse.to(DEV), lat.to(DEV)
    want = ld + hip_ops.resize_bilinear(cd, hf)
    tol, A = fwd_tol(coarse, hc, hf)
    tol = tol + U24 * (lat.double().abs() + A)
    err = (want.double().cpu() - ref).abs()
    print(f'merge {hc} -> {hf} C={C}: worst error / bound {float((err / tol).max()):.3g}')
    assert bool((err <= tol).all()), f'merge {hc} -> {hf}: {float((err / tol).max()):.3g} x the bound'
    return dict(coarse=cd, lat=ld, want=want, amax=want.abs().max())


def merge_operands(d, kind, viewed):
    pick = lambda role, t: view(tuple(t.shape), kind if role in viewed else 'plain', t)
    return pick('lat', d['lat']), pick('coarse', d['coarse']), view(tuple(d['lat'].shape), kind if 'out' in viewed else 'plain')


def expected_merge_route(hc, hf, lat, coarse, out):
    al = lambda t, m: t.data_ptr() % m == 0 and t.stride(0) % (m // 4) == 0
    if hf[1] % 4 or not (al(lat, 16) and al(out, 16)):
        return 'pixel'
    if hf == (2 * hc[0], 2 * hc[1]) and hc[0] > 1 and hc[1] > 1 and hc[1] % 2 == 0 and al(coarse, 8):
        return 'half'
    return 'quad'


MERGE_VIEWED = [(), ('lat',), ('coarse',), ('out',), ('lat', 'coarse', 'out')]


@channels
@pytest.mark.parametrize('hc,hf', MERGES)
def test_topdown_merge_on_views(ops, hc, hf, C):
    d = merge_case(hc, hf, C)
    for kind in ('slice', 'lead', 'odd'):
        for viewed in MERGE_VIEWED:
            gl, gc, go = merge_operands(d, kind, viewed)
            before = gl.flat.clone(), gc.flat.clone()
            route = ops.topdown_merge_route(gl.view, gc.view, go.view)
            assert route == expected_merge_route(hc, hf, gl.view, gc.view, go.view), (kind, viewed, route)
            what = f'topdown_merge {hc} -> {hf} {kind} {viewed} ({route})'
            slots = ops.amax_slots(DEV)
            ops.topdown_merge(gl.view, gc.view, out=go.view, amax=slots)
            unchanged(gl, before[0], what), unchanged(gc, before[1], what)
            go.intact(what)
            assert torch.equal(go.view, d['want']), f'{what}: differs from resize_bilinear + add'
            assert float(slots.max()) == float(d['amax']), f'{what}: published {float(slots.max())!r}, max |out| {float(d["amax"])!r}'
    # without a slot group, into a tensor of its own
    assert torch.equal(ops.topdown_merge(d['lat'], d['coarse']), d['want'])


def test_merge_refuses_its_lateral_as_output(ops):
    from pfst_amd._lib import PfstHipError
    d = merge_case((8, 8), (16, 16), 3)
    lat = d['lat'].clone()
    with pytest.raises(PfstHipError):
        ops.topdown_merge(lat, d['coarse'], out=lat)
    with pytest.raises(ValueError):
        ops.topdown_merge(d['coarse'], d['lat'])               # a coarse map finer than the lateral


def test_every_merge_route_is_reached(ops):
    seen = set()
    for hc, hf in MERGES:
        d = merge_case(hc, hf, 3)
        for kind in ('slice', 'lead', 'odd'):
            for viewed in MERGE_VIEWED:
                gl, gc, go = merge_operands(d, kind, viewed)
                seen.add(ops.topdown_merge_route(gl.view, gc.view, go.view))
    assert seen == set(ops.MERGE_ROUTES), set(ops.MERGE_ROUTES) - seen
    route = lambda hc, hf, kind, viewed: ops.topdown_merge_route(*[o.view for o in merge_operands(merge_case(hc, hf, 3), kind, viewed)])
    assert route((8, 8), (16, 16), 'slice', ('lat', 'coarse', 'out')) == 'half' == route((4, 6), (8, 12), 'slice', ('out',))
    assert route((2, 130), (4, 260), 'slice', ()) == 'half'
    assert route((8, 8), (16, 16), 'lead', ('coarse',)) == 'quad' == route((9, 40), (17, 80), 'slice', ('lat', 'coarse', 'out'))
    assert route((8, 8), (16, 16), 'lead', ('out',)) == 'pixel' == route((8, 8), (16, 16), 'odd', ('lat',)) == route((10, 9), (19, 17), 'slice', ())


# ----------------------------------------------------------------------------------------------------------------------------------- concat
@functools.lru_cache(maxsize=None)
def concat_case(hs, hf, C):
    from pfst_amd import hip_ops
    K = len(hs)
    srcs = [torch.randn((N, C) + h, generator=g(21 + k)) * (k + 1) for k, h in enumerate(hs)]
    dy = torch.randn(N, K * C, *hf, generator=g(31))
    olds = [torch.randn((N, C) + h, generator=g(41 + k)) for k, h in enumerate(hs)]
    sd, dyd, od = [s.to(DEV) for s in srcs], dy.to(DEV), [o.to(DEV) for o in olds]
    ys = [hip_ops.resize_bilinear(s, hf) for s in sd]
    dxs = [hip_ops.resize_bilinear_bwd(dyd[:, k * C:(k + 1) * C], h) for k, h in enumerate(hs)]
    accs = [hip_ops.resize_bilinear_bwd(dyd[:, k * C:(k + 1) * C], h, out=od[k].clone(), accumulate=True) for k, h in enumerate(hs)]
    for k, h in enumerate(hs):
        x64 = srcs[k].double().requires_grad_()
        y64 = F.interpolate(x64, size=hf, mode='bilinear', align_corners=False)
        y64.backward(dy[:, k * C:(k + 1) * C].double())
        tol_y, tol_dx = fwd_tol(srcs[k], h, hf)[0], bwd_tol(dy[:, k * C:(k + 1) * C], h, hf)
        for got, ref, tol, what in ((ys[k], y64.detach(), tol_y, 'forward'), (dxs[k], x64.grad, tol_dx, 'adjoint'),
                                    (accs[k], x64.grad + olds[k].double(), tol_dx + U24 * (x64.grad + olds[k].double()).abs(), 'adjoint, accumulated')):
            err = (got.double().cpu() - ref).abs()
            print(f'concat level {h} -> {hf} C={C} {what}: worst error / bound {float((err / tol).max()):.3g}')
            assert bool((err <= tol).all()), f'level {h} -> {hf} {what}: {float((err / tol).max()):.3g} x the bound'
    return dict(srcs=sd, dy=dyd, olds=od, y=torch.cat(ys, 1), dxs=dxs, accs=accs)


@channels
@pytest.mark.parametrize('hs,hf', CONCATS)
def test_fpn_resize_concat_on_views(ops, hs, hf, C):
    d = concat_case(hs, hf, C)
    K = len(hs)
    seen = set()
    for kind in ('plain', 'slice', 'lead', 'odd'):
        for src_kind in ('plain', kind):
            gs = [view(tuple(s.shape), src_kind, s) for s in d['srcs']]
            before = [gd.flat.clone() for gd in gs]
            go = view((N, K * C) + hf, kind)
            route = ops.fpn_resize_concat_route(go.view)
            assert route == int(hf[1] % 4 == 0 and go.view.data_ptr() % 16 == 0 and go.view.stride(0) % 4 == 0)
            seen.add(route)
            what = f'fpn_resize_concat {hs} -> {hf} out {kind} srcs {src_kind} (route {route})'
            slots = ops.amax_slots(DEV)
            ops.fpn_resize_concat([gd.view for gd in gs], go.view, amax=slots)
            for gd, b in zip(gs, before):
                unchanged(gd, b, what)
            go.intact(what)
            assert torch.equal(go.view, d['y']), f'{what}: differs from resize_bilinear(out=slice) per level'
            assert float(slots.max()) == float(d['y'].abs().max()), what
    assert seen == ({0, 1} if hf[1] % 4 == 0 else {0})
    # the slices in another order, inside a wider buffer: channels outside them stay untouched
    wide = torch.full((N, (K + 1) * C) + hf, -3.0, device=DEV)
    off = [(K - k) * C for k in range(K)]
    ops.fpn_resize_concat(d['srcs'], wide, chan_off=off)
    assert bool((wide[:, :C] == -3.0).all())
    for k in range(K):
        assert torch.equal(wide[:, off[k]:off[k] + C], d['y'][:, k * C:(k + 1) * C])


@channels
@pytest.mark.parametrize('hs,hf', CONCATS)
def test_fpn_resize_concat_bwd_on_views(ops, hs, hf, C):
    d = concat_case(hs, hf, C)
    K = len(hs)
    seen = set()
    for kind in ('plain', 'slice', 'lead', 'odd'):
        for dy_kind in ('plain', kind):
            for acc in ([False] * K, [True] * K, [k % 2 == 0 for k in range(K)]):
                gdy = view(tuple(d['dy'].shape), dy_kind, d['dy'])
                before = gdy.flat.clone()
                gos = [view(tuple(o.shape), kind, o if a else None) for o, a in zip(d['olds'], acc)]
                routes = ops.fpn_resize_concat_bwd_routes(gdy.view, [gd.view for gd in gos])
                seen.update(routes)
                what = f'fpn_resize_concat_bwd {hs} <- {hf} dy {dy_kind} outs {kind} accumulate {acc} (routes {routes})'
                ops.fpn_resize_concat_bwd(gdy.view, [gd.view for gd in gos], accumulate=acc)
                unchanged(gdy, before, what)
                for k, gd in enumerate(gos):
                    gd.intact(what)
                    assert torch.equal(gd.view, d['accs'][k] if acc[k] else d['dxs'][k]), f'{what}: level {k} differs from resize_bilinear_bwd'
    assert seen == ({0, 1} if hs[0] == (8, 8) else {0})           # the x2 form on 2 x 2 blocks: 8 x 8 <- 16 x 16, aligned operands
    if hs[0] == (8, 8):
        plain = ops.fpn_resize_concat_bwd_routes(d['dy'], [torch.empty_like(o) for o in d['olds']])
        assert plain == [1, 0, 0]
    # one flag for every level
    outs = ops.fpn_resize_concat_bwd(d['dy'], [torch.empty_like(o) for o in d['olds']], accumulate=False)
    assert all(torch.equal(o, w) for o, w in zip(outs, d['dxs']))


def test_level_count_and_shapes_are_checked(ops):
    d = concat_case(((5, 5),), (10, 9), 3)
    out = torch.empty(N, 12, 10, 9, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.fpn_resize_concat(d['srcs'] * 4, out)
    with pytest.raises(ValueError):
        ops.fpn_resize_concat(d['srcs'], out, chan_off=[10])             # the slice runs past the buffer
    with pytest.raises(ValueError):
        ops.fpn_resize_concat([torch.empty(N, 3, 11, 9, device=DEV)], out)      # finer than the buffer
    from pfst_amd._lib import PfstHipError
    with pytest.raises(PfstHipError):
        ops.fpn_resize_concat(d['srcs'] * 2, out, chan_off=[0, 2])       # overlapping slices
