"""The exchange-unit kernels of csrc/hrnet.hip -- hr_fuse, hr_fuse_bwd -- alone, on seeded fp16-valued inputs, against the composition of the
existing ops they replace and against fp64 (tests/hrnet_oracle.py), on operands that are views inside canary buffers (helpers.Guard).

Operand sets, in branch order ('id': final values on the output grid, 's': a same-grid member, an integer: a member coarser by that ratio):
  first2  [id, 2]            the first branch of a two-branch module
  first4  [id, 2, 4, 8]      the first branch of a four-branch module (stage 4, i = 0)
  last    [s, s, s, id]      the last branch
  middle  [s, s, id, 2]      a middle branch
each with a [C, 4] table on every member and with NULL tables.  N = 2, C = 6 and 5; 16 x 16 fine maps (rows of whole quads) and 6 x 10 over
3 x 5 (Wf % 4 != 0; first4 needs an output divisible by 8 and runs on 16 x 16 only).  Views: channels [1, 1 + C) of a (C + 4)-channel buffer (an
odd channel offset, batch stride != C H W), planes 4 bytes past a 16-byte boundary, an odd batch stride.

Forward: (a) torch.equal to bn_apply(relu=False) per tabled member, resize_bilinear per coarser member, the adds in branch order, ReLU; (b) the
published maximum is exact; (c) within the oracle's bound of fp64 (2^-24 x magnitude x roundings, derived there); (d) canaries untouched, inputs
unchanged; (e) the route is 'quad' exactly where Wf % 4 == 0 and out and every output-grid operand are 16-byte aligned with a batch stride % 4 == 0.
Backward: gy and every coarse gradient torch.equal to gate-then-resize_bilinear_bwd, written and accumulated, gy also in place of d_out; against the
fp64 adjoint within tests/test_fpn_kernels_gpu.py's bound for concat_bwd (bwd_tol: T taps reach a source pixel, T + t_y fused multiply-adds round
partial sums of at most S B; an accumulated result rounds once more); canaries hold."""
import functools

import pytest
import torch

from hrnet_oracle import U24, fuse_bwd_fp64, fuse_fp64
from helpers import Guard
from test_fpn_kernels_gpu import bwd_tol, unchanged
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N = 2
SETS = {'first2': ('id', 2), 'first4': ('id', 2, 4, 8), 'last': ('s', 's', 's', 'id'), 'middle': ('s', 's', 'id', 2)}
CASES = [(s, hf) for hf in ((16, 16), (6, 10)) for s in SETS if not (s == 'first4' and hf == (6, 10))]
KINDS = {'plain': dict(front=0, back=0), 'slice': dict(front=1, back=3), 'lead': dict(front=1, back=3, lead=1), 'odd': dict(front=0, back=0, odd=1)}
VIEW_KINDS = ('slice', 'lead', 'odd')
channels = pytest.mark.parametrize('C', [6, 5])


def view(shape, kind, t=None):
    gd = Guard(tuple(shape), **KINDS[kind])
    if t is not None:
        gd.put(t)
    return gd


def al16(t):
    return t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0


def f16(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=g(seed)) * scale).half().float()


def table(C, seed):
    """[C, 4] rows (mean, invstd, sc, sh) = (0, 1, sc, sh): bn_apply(mean 0, invstd 1, gamma sc, beta sh) forms exactly these (sc, sh); both signs"""
    sc = (torch.rand(C, generator=g(seed)) + 0.5) * torch.tensor([1.0, -1.0] * C)[:C]
    sh = torch.randn(C, generator=g(seed + 1)) * 0.5
    return torch.stack([torch.zeros(C), torch.ones(C), sc, sh], 1).contiguous().to(DEV)


def member_hw(kind, hf):
    return hf if kind in ('id', 's') else (hf[0] // kind, hf[1] // kind)


@functools.lru_cache(maxsize=None)
def case(name, hf, C, tabled):
    """inputs, the composition of the existing ops on plain tensors (held to fp64 once), its maximum, and the backward's inputs and composition"""
    from pfst_amd import hip_ops
    kinds = SETS[name]
    xs = [f16((N, C) + member_hw(k, hf), 200 + j, 1.0 + 0.5 * j).to(DEV) for j, k in enumerate(kinds)]
    coefs = [table(C, 220 + 2 * j) if (tabled and k != 'id') else None for j, k in enumerate(kinds)]
    total = None
    for x, coef, k in zip(xs, coefs, kinds):
        t = x if coef is None else hip_ops.bn_apply(x, coef[:, 0].contiguous(), coef[:, 1].contiguous(), coef[:, 2].contiguous(),
                                                    coef[:, 3].contiguous(), False)
        if k not in ('id', 's'):
            t = hip_ops.resize_bilinear(t, hf)
        total = t if total is None else total + t
    want = torch.relu(total)
    ref, tol = fuse_fp64([x.cpu() for x in xs], coefs, hf)
    err = (want.double().cpu() - ref).abs()
    ratio = float((err / tol.clamp_min(1e-300)).max())
    print(f'hr_fuse {name} {hf} C={C} tables={tabled}: worst error / bound {ratio:.3g}')
    assert bool((err <= tol).all()), f'hr_fuse {name} {hf}: {ratio:.3g} x the bound'
    assert 0.2 < float((want == 0).float().mean()) < 0.8                      # the ReLU gates a good part, not all
    # backward
    d_out = f16((N, C) + hf, 260).to(DEV)
    coarse_hw = [member_hw(k, hf) for k in kinds if k not in ('id', 's')]
    gy = torch.where(want > 0, d_out, torch.zeros((), device=DEV))
    olds = [f16((N, C) + hw, 270 + i).to(DEV) for i, hw in enumerate(coarse_hw)]
    written = [hip_ops.resize_bilinear_bwd(gy, hw) for hw in coarse_hw]
    added = [hip_ops.resize_bilinear_bwd(gy, hw, out=o.clone(), accumulate=True) for hw, o in zip(coarse_hw, olds)]
    gy64, g64 = fuse_bwd_fp64(d_out.cpu(), want.cpu(), coarse_hw)
    assert torch.equal(gy.double().cpu(), gy64)
    tols = [bwd_tol(gy.cpu(), hw, hf) for hw in coarse_hw]
    for i, hw in enumerate(coarse_hw):
        for got, r64, extra in ((written[i], g64[i], 0.0), (added[i], g64[i] + olds[i].double().cpu(), None)):
            t = tols[i] + (U24 * r64.abs() if extra is None else 0.0)
            e = (got.double().cpu() - r64).abs()
            print(f'hr_fuse_bwd {name} {hf} -> {hw} C={C}: worst error / bound {float((e / t.clamp_min(1e-300)).max()):.3g}')
            assert bool((e <= t).all()), f'hr_fuse_bwd {name} {hf} -> {hw}: outside the bound'
    return dict(kinds=kinds, xs=xs, coefs=coefs, want=want, amax=float(want.abs().max()), d_out=d_out, gy=gy, coarse_hw=coarse_hw, olds=olds,
                written=written, added=added)


def expected_route(hf, kinds, op_views, out):
    same = [v for v, k in zip(op_views, kinds) if k in ('id', 's')]
    return 'quad' if hf[1] % 4 == 0 and al16(out) and all(al16(v) for v in same) else 'pixel'


@channels
@pytest.mark.parametrize('tabled', [True, False])
@pytest.mark.parametrize('name,hf', CASES)
def test_hr_fuse_on_views(ops, name, hf, tabled, C):
    d = case(name, hf, C, tabled)
    seen = set()
    for kind in VIEW_KINDS:
        for viewed in [(), ('ops',), ('out',), ('ops', 'out')]:
            gops = [view(x.shape, kind if 'ops' in viewed else 'plain', x) for x in d['xs']]
            go = view(d['want'].shape, kind if 'out' in viewed else 'plain')
            before = [x.flat.clone() for x in gops]
            vs = [x.view for x in gops]
            route = ops.hr_fuse_route(vs, go.view)
            assert route == expected_route(hf, d['kinds'], vs, go.view), (kind, viewed, route)
            seen.add(route)
            what = f'hr_fuse {name} {hf} C={C} tables={tabled} {kind} {viewed} ({route})'
            slots = ops.amax_slots(DEV)
            ops.hr_fuse(vs, d['coefs'], out=go.view, amax=slots)
            for x, b in zip(gops, before):
                unchanged(x, b, what)
            go.intact(what)
            assert torch.equal(go.view, d['want']), f'{what}: differs from the composition of the existing ops'
            assert float(slots.max()) == d['amax'], f'{what}: published {float(slots.max())!r}, max |out| {d["amax"]!r}'
    assert seen == ({'pixel', 'quad'} if hf[1] % 4 == 0 else {'pixel'}), seen
    # without a slot group, into a tensor of its own
    assert torch.equal(ops.hr_fuse(d['xs'], d['coefs'], out_hw=hf), d['want'])
    assert ops.hr_fuse_route(d['xs'], d['want']) == ('quad' if hf[1] % 4 == 0 else 'pixel')


@channels
@pytest.mark.parametrize('name,hf', CASES)
def test_hr_fuse_bwd_on_views(ops, name, hf, C):
    d = case(name, hf, C, True)
    K = len(d['coarse_hw'])
    flag_sets = [[False] * K, [True] * K] + ([[True, False, True][:K]] if K > 1 else [])
    for kind in VIEW_KINDS:
        for viewed in [(), ('in',), ('out',), ('in', 'out')]:
            for acc in flag_sets:
                gd = view(d['d_out'].shape, kind if 'in' in viewed else 'plain', d['d_out'])
                gout = view(d['want'].shape, kind if 'in' in viewed else 'plain', d['want'])
                ggy = view(d['want'].shape, kind if 'out' in viewed else 'plain')
                gcs = [view(o.shape, kind if 'out' in viewed else 'plain', o) for o in d['olds']]
                before = gd.flat.clone(), gout.flat.clone()
                what = f'hr_fuse_bwd {name} {hf} C={C} {kind} {viewed} accumulate {acc}'
                got = ops.hr_fuse_bwd(gd.view, gout.view, [x.view for x in gcs], accumulate=acc, gy=ggy.view)
                assert got is ggy.view
                unchanged(gd, before[0], what), unchanged(gout, before[1], what)
                ggy.intact(what)
                assert torch.equal(ggy.view, d['gy']), f'{what}: gy differs from the gated d_out'
                for i, x in enumerate(gcs):
                    x.intact(what)
                    assert torch.equal(x.view, (d['added'] if acc[i] else d['written'])[i]), f'{what}: level {i} differs from resize_bilinear_bwd(gy)'
    # gy in place of d_out; and buffers of its own
    dd = d['d_out'].clone()
    cs = [torch.empty_like(o) for o in d['olds']]
    assert ops.hr_fuse_bwd(dd, d['want'], cs, gy=dd) is dd and torch.equal(dd, d['gy'])
    assert all(torch.equal(c, w) for c, w in zip(cs, d['written']))
    assert torch.equal(ops.hr_fuse_bwd(d['d_out'], d['want']), d['gy'])


def test_hr_fuse_checks_its_operands(ops):
    from pfst_amd._lib import PfstHipError
    d = case('first4', (16, 16), 6, True)
    xs = d['xs']
    with pytest.raises(PfstHipError):
        ops.hr_fuse(xs, d['coefs'], out=xs[0])                                                        # in place
    with pytest.raises(ValueError):
        ops.hr_fuse([xs[0], torch.zeros(N, 6, 5, 5, device=DEV)])                                    # 16 / 5: no exact ratio
    with pytest.raises(ValueError):
        ops.hr_fuse([xs[0], torch.zeros(N, 6, 1, 1, device=DEV)])                                    # ratio 16
    with pytest.raises(ValueError):
        ops.hr_fuse(xs + xs[:1])                                                                     # five operands
    with pytest.raises(NotImplementedError):
        ops.hr_fuse([xs[1], xs[1], xs[2], xs[3]], out_hw=(16, 16))                                   # four coarser operands
    with pytest.raises(ValueError):
        ops.hr_fuse(xs, [None, torch.zeros(4, 4, device=DEV), None, None])                           # a table of another channel count
    with pytest.raises(ValueError):
        ops.hr_fuse_bwd(d['d_out'], d['want'], [torch.zeros(N, 6, 16, 16, device=DEV)])              # a "coarser" buffer on the output grid
    with pytest.raises(PfstHipError):
        ops.hr_fuse_bwd(d['d_out'], d['want'], gy=d['want'])                                         # gy over the saved output
