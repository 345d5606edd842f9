"""The Semantic FPN kernels of csrc/fpn.hip -- topdown_merge_nearest, nearest_resize_bwd, upsample2x_norm, fpn_level_sum -- against the
compositions of the existing ops they replace and against fp64, on operands that are views inside canary buffers (helpers.Guard), as in
tests/test_fpn_kernels_gpu.py: (i) channels [2, 2 + C) of a (C + 5)-channel buffer, (ii) planes 4 bytes past a 16-byte boundary, (iii) an odd
batch stride; N = 2, C = 3 and 5.  Inputs must come back unchanged, nothing outside an output view may be written.

Checks:
  * nearest merge: torch.equal to lat + F.interpolate(coarse, size, mode='nearest') in fp32 (one rounded add: the same bits), over that
    file's MERGES; the published maximum is exact;
  * nearest adjoint, written and accumulated, against fp64 autograd within 2^-24 (T - 1) T B: a plain sum of at most T = ceil(Hf / Hc)
    ceil(Wf / Wc) terms (the largest pre-image) of magnitude at most B = max |dy| of the plane -- T - 1 roundings of partial sums of at most
    T B; accumulated: one more rounding of the result;
  * upsample2x_norm: torch.equal to bn_apply + resize_bilinear, with and without a table (rows with both signs of sc and one channel the ReLU
    zeroes entirely); maximum exact; against fp64 within that file's fwd_tol at d = 0 (2^-24 A 4) plus the normalisation's two roundings
    (2 2^-24 A), A = max |act(pre)| of the plane;
  * fpn_level_sum: torch.equal to the composition in the stated order -- bn_apply per operand, the adds on the half grid, resize_bilinear, one
    add, one more for the addend -- for K = 0 .. 3, tables on all, some or none of the operands, with and without an addend; maximum exact;
  * every route each *_route query can answer is reached, and equals the expectation written here."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from test_fpn_kernels_gpu import MERGES, N, U24, channels, unchanged, view
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SOURCES = [(1, 1), (3, 3), (5, 5), (4, 6), (8, 8), (9, 40), (2, 130)]
HALVES = [(3, 3), (4, 6), (8, 8), (2, 130)]
VIEW_KINDS = ('slice', 'lead', 'odd')


def al(t, m):
    return t.data_ptr() % m == 0 and t.stride(0) % (m // 4) == 0


def table(C, seed):
    """[C, 4] rows (mean, invstd, sc, sh) = (0, 1, sc, sh): bn_apply(mean 0, invstd 1, gamma sc, beta sh) forms exactly these (sc, sh).  Both signs
    of sc; channel 1 is zeroed entirely by the ReLU"""
    sc = (torch.rand(C, generator=g(seed)) + 0.5) * torch.tensor([1.0, -1.0] * C)[:C]
    sh = torch.randn(C, generator=g(seed + 1)) * 0.5
    sc[1], sh[1] = -0.5, -100.0
    return torch.stack([torch.zeros(C), torch.ones(C), sc, sh], 1).contiguous().to(DEV)


def apply_table(hip_ops, x, coef):
    """what the kernels' act() must reproduce: the library's own normalisation pass"""
    if coef is None:
        return x
    return hip_ops.bn_apply(x.contiguous(), coef[:, 0].contiguous(), coef[:, 1].contiguous(), coef[:, 2].contiguous(), coef[:, 3].contiguous(), True)


# ------------------------------------------------------------------------------------------------------------------------------ nearest merge
@functools.lru_cache(maxsize=None)
def merge_case(hc, hf, C):
    coarse = torch.randn((N, C) + hc, generator=g(111)) * 3
    lat = torch.randn((N, C) + hf, generator=g(112)) * 2
    dy = torch.randn((N, C) + hf, generator=g(113))
    old = torch.randn((N, C) + hc, generator=g(114))
    want = lat + F.interpolate(coarse, size=hf, mode='nearest')
    c64 = coarse.double().requires_grad_()
    F.interpolate(c64, size=hf, mode='nearest').backward(dy.double())
    T = math.ceil(hf[0] / hc[0]) * math.ceil(hf[1] / hc[1])
    B = dy.double().abs().amax((2, 3), keepdim=True)
    return dict(coarse=coarse.to(DEV), lat=lat.to(DEV), dy=dy.to(DEV), old=old.to(DEV), old64=old.double(), want=want.to(DEV),
                amax=float(want.abs().max()), dx64=c64.grad, tol=U24 * (T - 1) * T * B)


def expected_merge_route(hc, hf, lat, coarse, out):
    if hf[1] % 4 or not (al(lat, 16) and al(out, 16)):
        return 'pixel'
    if hf == (2 * hc[0], 2 * hc[1]) and al(coarse, 8):
        return 'double'
    return 'quad'


MERGE_VIEWED = [(), ('lat',), ('coarse',), ('out',), ('lat', 'coarse', 'out')]


def merge_operands(d, kind, viewed):
    pick = lambda role, t: view(tuple(t.shape), kind if role in viewed else 'plain', t)
    return pick('lat', d['lat']), pick('coarse', d['coarse']), view(tuple(d['lat'].shape), kind if 'out' in viewed else 'plain')


@channels
@pytest.mark.parametrize('hc,hf', MERGES)
def test_topdown_merge_nearest_on_views(ops, hc, hf, C):
    d = merge_case(hc, hf, C)
    for kind in VIEW_KINDS:
        for viewed in MERGE_VIEWED:
            gl, gc, go = merge_operands(d, kind, viewed)
            before = gl.flat.clone(), gc.flat.clone()
            route = ops.topdown_merge_nearest_route(gl.view, gc.view, go.view)
            assert route == expected_merge_route(hc, hf, gl.view, gc.view, go.view), (kind, viewed, route)
            what = f'topdown_merge_nearest {hc} -> {hf} {kind} {viewed} ({route})'
            slots = ops.amax_slots(DEV)
            ops.topdown_merge_nearest(gl.view, gc.view, out=go.view, amax=slots)
            unchanged(gl, before[0], what), unchanged(gc, before[1], what)
            go.intact(what)
            assert torch.equal(go.view, d['want']), f"{what}: differs from lat + F.interpolate(mode='nearest')"
            assert float(slots.max()) == d['amax'], f'{what}: published {float(slots.max())!r}, max |out| {d["amax"]!r}'
    assert torch.equal(ops.topdown_merge_nearest(d['lat'], d['coarse']), d['want'])


def test_merge_nearest_refusals(ops):
    from pfst_amd._lib import PfstHipError
    d = merge_case((8, 8), (16, 16), 3)
    lat = d['lat'].clone()
    with pytest.raises(PfstHipError):
        ops.topdown_merge_nearest(lat, d['coarse'], out=lat)
    with pytest.raises(ValueError):
        ops.topdown_merge_nearest(d['coarse'], d['lat'])               # a coarse map finer than the lateral


def expected_bwd_route(hc, hf, dy, dx):
    return 'double' if hf == (2 * hc[0], 2 * hc[1]) and hc[1] % 2 == 0 and al(dy, 16) and al(dx, 8) else 'gather'


@channels
@pytest.mark.parametrize('hc,hf', MERGES)
def test_nearest_resize_bwd_on_views(ops, hc, hf, C):
    d = merge_case(hc, hf, C)
    worst = 0.0
    for kind in VIEW_KINDS:
        for viewed in [(), ('dy',), ('dx',), ('dy', 'dx')]:
            for acc in (False, True):
                gdy = view(tuple(d['dy'].shape), kind if 'dy' in viewed else 'plain', d['dy'])
                gdx = view(tuple(d['old'].shape), kind if 'dx' in viewed else 'plain', d['old'] if acc else None)
                before = gdy.flat.clone()
                route = ops.nearest_resize_bwd_route(gdy.view, gdx.view)
                assert route == expected_bwd_route(hc, hf, gdy.view, gdx.view), (kind, viewed, route)
                what = f'nearest_resize_bwd {hc} <- {hf} {kind} {viewed} accumulate {acc} ({route})'
                ops.nearest_resize_bwd(gdy.view, hc, out=gdx.view, accumulate=acc)
                unchanged(gdy, before, what)
                gdx.intact(what)
                ref = d['dx64'] + d['old64'] if acc else d['dx64']
                tol = d['tol'] + (U24 * ref.abs() if acc else 0.0)
                err = (gdx.view.double().cpu() - ref).abs()
                assert bool((err <= tol).all()), f'{what}: error {float(err.max()):.3g} outside the bound'
                worst = max(worst, float((err / tol.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0)
    print(f'nearest_resize_bwd {hc} <- {hf} C={C}: worst error / bound {worst:.3g}')
    assert torch.equal(ops.nearest_resize_bwd(d['dy'], hc), ops.nearest_resize_bwd(d['dy'], hc, out=torch.empty_like(d['old'])))


def test_every_nearest_route_is_reached(ops):
    merges, bwds = set(), set()
    for hc, hf in MERGES:
        d = merge_case(hc, hf, 3)
        for kind in VIEW_KINDS:
            for viewed in MERGE_VIEWED:
                gl, gc, go = merge_operands(d, kind, viewed)
                merges.add(ops.topdown_merge_nearest_route(gl.view, gc.view, go.view))
            for dyk, dxk in (('plain', 'plain'), (kind, 'plain'), ('plain', kind)):
                bwds.add(ops.nearest_resize_bwd_route(view(tuple(d['dy'].shape), dyk).view, view(tuple(d['old'].shape), dxk).view))
    assert merges == set(ops.MERGE_NEAREST_ROUTES), set(ops.MERGE_NEAREST_ROUTES) - merges
    assert bwds == set(ops.NEAREST_BWD_ROUTES), set(ops.NEAREST_BWD_ROUTES) - bwds
    route = lambda hc, hf, kind, viewed: ops.topdown_merge_nearest_route(*[o.view for o in merge_operands(merge_case(hc, hf, 3), kind, viewed)])
    assert route((8, 8), (16, 16), 'slice', ('lat', 'coarse', 'out')) == 'double' == route((2, 130), (4, 260), 'slice', ())
    assert route((8, 8), (16, 16), 'lead', ('coarse',)) == 'quad' == route((9, 40), (17, 80), 'slice', ('lat', 'coarse', 'out'))
    assert route((8, 8), (16, 16), 'lead', ('out',)) == 'pixel' == route((10, 9), (19, 17), 'slice', ()) == route((1, 1), (2, 2), 'slice', ())


# --------------------------------------------------------------------------------------------------------------------------- upsample2x_norm
@functools.lru_cache(maxsize=None)
def up_case(hc, C, tabled):
    from pfst_amd import hip_ops
    pre = torch.randn((N, C) + hc, generator=g(121)) * 2
    coef = table(C, 131) if tabled else None
    pd = pre.to(DEV)
    hf = (2 * hc[0], 2 * hc[1])
    a = apply_table(hip_ops, pd, coef)
    want = hip_ops.resize_bilinear(a, hf)
    a64 = pre.double()
    if tabled:
        a64 = torch.relu(a64 * coef[:, 2].double().cpu().view(1, C, 1, 1) + coef[:, 3].double().cpu().view(1, C, 1, 1))
        assert float(a[:, 1].abs().max()) == 0.0                        # the channel the ReLU zeroes
    ref = F.interpolate(a64, size=hf, mode='bilinear', align_corners=False)
    A = a64.abs().amax((2, 3), keepdim=True)
    tol = U24 * A * 4 + 2 * U24 * A
    err = (want.double().cpu() - ref).abs()
    print(f'upsample2x_norm {hc} C={C} table={tabled}: worst error / bound {float((err / tol.clamp_min(1e-300)).max()):.3g}')
    assert bool((err <= tol).all())
    return dict(pre=pd, coef=coef, want=want, amax=float(want.abs().max()))


def expected_up_route(hc, pre, out):
    return 'walk' if hc[0] > 1 and hc[1] > 1 and hc[1] % 2 == 0 and al(pre, 8) and al(out, 16) else 'pixel'


@channels
@pytest.mark.parametrize('tabled', [True, False])
@pytest.mark.parametrize('hc', SOURCES)
def test_upsample2x_norm_on_views(ops, hc, tabled, C):
    d = up_case(hc, C, tabled)
    for kind in VIEW_KINDS:
        for viewed in [(), ('pre',), ('out',), ('pre', 'out')]:
            gp = view(tuple(d['pre'].shape), kind if 'pre' in viewed else 'plain', d['pre'])
            go = view(tuple(d['want'].shape), kind if 'out' in viewed else 'plain')
            before = gp.flat.clone()
            route = ops.upsample2x_norm_route(gp.view, go.view)
            assert route == expected_up_route(hc, gp.view, go.view), (kind, viewed, route)
            what = f'upsample2x_norm {hc} {kind} {viewed} table={tabled} ({route})'
            slots = ops.amax_slots(DEV)
            ops.upsample2x_norm(gp.view, d['coef'], out=go.view, amax=slots)
            unchanged(gp, before, what)
            go.intact(what)
            assert torch.equal(go.view, d['want']), f'{what}: differs from bn_apply + resize_bilinear'
            assert float(slots.max()) == d['amax'], what
    assert torch.equal(ops.upsample2x_norm(d['pre'], d['coef']), d['want'])


def test_every_upsample_route_is_reached(ops):
    seen = set()
    for hc in SOURCES:
        d = up_case(hc, 3, False)
        for kind in VIEW_KINDS + ('plain',):
            seen.add(ops.upsample2x_norm_route(view(tuple(d['pre'].shape), kind).view, view(tuple(d['want'].shape), 'plain').view))
    assert seen == set(ops.UPSAMPLE2X_ROUTES)
    plain = lambda hc: ops.upsample2x_norm_route(up_case(hc, 3, False)['pre'], up_case(hc, 3, False)['want'])
    assert plain((8, 8)) == plain((4, 6)) == plain((9, 40)) == plain((2, 130)) == 'walk'
    assert plain((1, 1)) == plain((3, 3)) == plain((5, 5)) == 'pixel'
    with pytest.raises(ValueError):
        ops.upsample2x_norm(up_case((4, 6), 3, False)['pre'], torch.zeros(4, 4, device=DEV))          # a table of another channel count


# ----------------------------------------------------------------------------------------------------------------------------- fpn_level_sum
TABLES = {'all': (True, True, True, True), 'some': (True, False, True, False), 'none': (False, False, False, False)}


@functools.lru_cache(maxsize=None)
def sum_inputs(hh, C):
    full = (2 * hh[0], 2 * hh[1])
    pre0 = (torch.randn((N, C) + full, generator=g(141)) * 2).to(DEV)
    members = [(torch.randn((N, C) + hh, generator=g(142 + k)) * (k + 1)).to(DEV) for k in range(3)]
    addend = torch.randn((N, C) + full, generator=g(146)).to(DEV)
    return dict(pre0=pre0, members=members, addend=addend, tables=[table(C, 151 + 2 * k) for k in range(4)])


@functools.lru_cache(maxsize=None)
def sum_want(hh, C, K, tables, with_addend):
    """the composition, in the stated order"""
    from pfst_amd import hip_ops
    d = sum_inputs(hh, C)
    use = TABLES[tables]
    coefs = [d['tables'][k] if use[k] else None for k in range(4)]
    out = apply_table(hip_ops, d['pre0'], coefs[0])
    if K:
        s = apply_table(hip_ops, d['members'][0], coefs[1])
        for k in range(1, K):
            s = s + apply_table(hip_ops, d['members'][k], coefs[k + 1])
        out = out + hip_ops.resize_bilinear(s.contiguous(), (2 * hh[0], 2 * hh[1]))
    if with_addend:
        out = out + d['addend']
    return coefs, out.clone(), float(out.abs().max())


def expected_sum_route(hh, K, pre0, members, addend, out):
    if not (al(pre0, 16) and al(out, 16) and (addend is None or al(addend, 16))):
        return 'pixel'
    if K == 0:
        return 'quad' if (4 * hh[0] * hh[1]) % 4 == 0 else 'pixel'
    return 'quad' if hh[0] > 1 and hh[1] > 1 and hh[1] % 2 == 0 and all(al(m, 8) for m in members) else 'pixel'


SUM_VIEWED = [(), ('pre0',), ('members',), ('addend',), ('out',), ('pre0', 'members', 'addend', 'out')]


def sum_operands(d, K, with_addend, kind, viewed):
    pick = lambda role, t: view(tuple(t.shape), kind if role in viewed else 'plain', t)
    return (pick('pre0', d['pre0']), [pick('members', m) for m in d['members'][:K]], pick('addend', d['addend']) if with_addend else None,
            view(tuple(d['pre0'].shape), kind if 'out' in viewed else 'plain'))


@channels
@pytest.mark.parametrize('K', [0, 1, 2, 3])
@pytest.mark.parametrize('hh', HALVES)
def test_fpn_level_sum_on_views(ops, hh, K, C):
    d = sum_inputs(hh, C)
    seen = set()
    for tables in TABLES:
        for with_addend in (False, True):
            coefs, want, amax = sum_want(hh, C, K, tables, with_addend)
            for kind in VIEW_KINDS:
                for viewed in SUM_VIEWED:
                    if ('addend' in viewed and not with_addend) or ('members' in viewed and K == 0):
                        continue
                    g0, gm, ga, go = sum_operands(d, K, with_addend, kind, viewed)
                    before = [x.flat.clone() for x in [g0] + gm + ([ga] if ga else [])]
                    mv, av = [x.view for x in gm], None if ga is None else ga.view
                    route = ops.fpn_level_sum_route(g0.view, mv, av, go.view)
                    assert route == expected_sum_route(hh, K, g0.view, mv, av, go.view), (tables, with_addend, kind, viewed, route)
                    seen.add(route)
                    what = f'fpn_level_sum half {hh} K={K} tables {tables} addend {with_addend} {kind} {viewed} ({route})'
                    slots = ops.amax_slots(DEV)
                    ops.fpn_level_sum(g0.view, coefs[0], mv, coefs[1:K + 1], addend=av, out=go.view, amax=slots)
                    for x, b in zip([g0] + gm + ([ga] if ga else []), before):
                        unchanged(x, b, what)
                    go.intact(what)
                    assert torch.equal(go.view, want), f'{what}: differs from the composition'
                    assert float(slots.max()) == amax, what
    assert seen == ({'pixel', 'quad'} if (K == 0 or hh != (3, 3)) else {'pixel'}), seen
    coefs, want, _ = sum_want(hh, C, K, 'all', True)
    assert torch.equal(ops.fpn_level_sum(d['pre0'], coefs[0], d['members'][:K], coefs[1:K + 1], addend=d['addend']), want)


def test_level_sum_checks_its_operands(ops):
    d = sum_inputs((4, 6), 3)
    with pytest.raises(NotImplementedError):
        ops.fpn_level_sum(d['pre0'], None, d['members'] + d['members'][:1])                  # four half-grid members
    with pytest.raises(ValueError):
        ops.fpn_level_sum(d['pre0'], None, [d['pre0']])                                     # a member on the full grid
    with pytest.raises(ValueError):
        ops.fpn_level_sum(d['pre0'], None, d['members'][:1], addend=d['members'][0])         # an addend on the half grid
    from pfst_amd._lib import PfstHipError
    with pytest.raises(PfstHipError):
        ops.fpn_level_sum(d['pre0'], None, d['members'][:1], out=d['pre0'])                  # in place
