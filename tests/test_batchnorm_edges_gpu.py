"""The BatchNorm family (csrc/bn.hip: pfst_bn_stats, _finalize_partials, _apply, _backward, _backward_sums, _backward_dual, pfst_relu_gate)
where tests/test_hip_ops.py and tests/test_deterministic_kernels_gpu.py hold the operands contiguous, the planes small or whole and the
options off: several chunks per plane with a ragged last one, several workgroups per plane under the reversed traversal, the folded
Dropout2d factor, the residual normalised on load, the recomputed ReLU gate, operands that are channel slices of larger buffers, planes that
are misaligned although HW % 4 == 0, odd batch strides, slot tables of every length class, the two-layer backward, deterministic mode.

References: torch fp64 on the CPU from seeded inputs.  Batch statistics from x.double(); y = [relu](xhat gamma + beta [+ r | + fma(r, rsc,
rsh)]) [* post[n, c]]; gradients by the closed form dx = gs (dz - m1 - xhat m2), dgamma = sum dz xhat, dbeta = sum dz.  The ReLU gate of a
backward launch is an INPUT of that launch, so its reference is built with gate = (y_kernel > 0), the tensor bn_apply wrote: no element near
zero has to be excluded anywhere.  The forward test asserts separately that y is within its bound everywhere, that (y_kernel > 0) agrees
with (z_ref > 0) wherever |z_ref| exceeds that element's bound, and that the mask bits are exactly y_kernel > 0 in the layout documented in
csrc/bn_bwd.h.  N = 3, C = 5 (N != C, neither 1) and every per-channel vector differs per channel and per image; gamma is negative on odd
channels; post is 0 on four of the fifteen planes and 1 / 0.9 elsewhere, in a pattern that is symmetric neither in n nor in c.

Bounds, element-wise: mean |err| <= 2^-23 |ref| + 1e-10, invstd 2^-23 relative, running statistics 1e-5 (as test_batchnorm_train);
y, dx, dgamma, dbeta and the (m1, m2) record: K 2^-24 M_i with M_i the sum of the magnitudes of the terms of that element's expression
(fwd_ref, bwd_ref say which) and K measured on the CPU, see K below.  dres written: bit-equal to dy * gate; accumulated: one fp32 add.
bn_apply on the vector and on the scalar path of the same data: bit for bit.  fp64 sums read back from the scratch: slot_sum_bound.

Path conditions pinned here ("Path conditions of the BatchNorm entries"): per plane in bn_stats_kernel / bn_apply_kernel, per
launch on the host (bn_vec_route) in pfst_bn_backward / _backward_sums / _backward_dual, repeated in Python by hip_ops.bn_apply / bn_backward_dual for the
mask.  In deterministic mode the two routes of one launch differ in the order of their fp64 sums, which the tests read back from the 'bn'
scratch and from the record: every call with ONE misaligned operand must give the scalar route's bits (test_f_deterministic_routes plants a
cancelling pair per channel so that the two orders differ by construction), and the slots are added in (image, chunk) order.

Run `python tests/test_batchnorm_edges_gpu.py` on any machine (no GPU needed) to repeat the measurement behind K.

MEASURED on an MI355X, the worst error of the file in units of 2^-24 M_i (the bound is K = 29.1): dx 7.19 (the dual
backward's second layer, as in the CPU measurement), y 2.58, dgamma 1.09, dbeta 0.92, m2 0.20, m1 1.5e-9; every exact check holds as written.

Found by this file: hip_ops.bn_backward_dual asserted on a plane that is no multiple of 256 elements where pfst_bn_backward_dual answers
PFST_ERR_UNSUPPORTED and the caller is promised None (test_e_dual_declines[12-21-None]); the wrapper now repeats the C condition first.

Mutations of csrc/bn.hip tried against this file on the MI355X, each on its own (none committed):
  1. `post[n * C + c]` -> `post[c]` in bn_apply_kernel: test_b_apply_options, test_b_backward_options (their forward), every
     test_c_apply_on_views case (the post launch) fail.
  2. `b.bx` (then `bxi`) -> `blockIdx.x` for `beg` in bn_bwd_reduce_kernel: every chunk is still summed once, so only deterministic mode's slot
     order moves (chunks of an image from the other end): test_f_deterministic_slot_order fails at both shapes on `bn_backward: slots out of order`.
  3. `dres_bs` dropped from `vec` (now the operands handed to bn_vec_route) in pfst_bn_backward: the float4 kernels run on dres planes 4 and 8 bytes past alignment, the values stay
     right; test_f_deterministic_routes fails on `bn_backward with a misaligned dres (odd) did not take the scalar route`, nothing else notices.
  4. `y_bs` -> `(i64)C * HW` for `yp` in bn_apply_kernel: all test_c_apply_on_views cases with the output (or all operands) as a view fail
     (canaries written, y wrong); the writes stay inside the canary buffer, whose batch stride is at least C * HW.
  5. `done = T2 * 2` -> `done = T` in sum_partial_slots: test_d_finalize_partials and test_d_backward_partials fail for T = 1 and every odd T.
  6. `T >= 4096` -> `T > 4096` with the 256-thread instance launched on 1024 threads -- not run (it writes LDS outside `mm[2][4]`); by
     reading: waves 4 ... 15 store their extrema at mm[0][4 ... 15], which aliases mm[1][0 ... 3] and what lies behind, so thread 0 folds minima
     into `hi`: the predicted maximum of test_d_finalize_partials[4096-*] is wrong (and block_sum2_d's own slots are sized for 16 waves, so the
     statistics would survive: only the amax assertion tells).
  7. the `i < n4` guard of the mask store removed -- not run (the last plane's surplus words land behind the mask allocation); by reading:
     at (72, 64) the two workgroups' unrolled float4 offsets 1152 ... 2047 of plane p become mask words 72 ... 127 of its row, i.e. words
     0 ... 55 of plane p + 1, holding the ballots of zero loads (sh + 0 > 0, the same for every lane).  Under the reversed traversal plane
     p + 1 is written before plane p, so the surplus lands last: test_b_apply_options[72-64], test_c_apply_on_views[72-64-slice-*] and
     base() fail on `mask bits != (y > 0)`, and with them every backward gated by that mask."""
import contextlib
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from helpers import SENT, Guard
from test_hip_ops import assert_close, g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-5
U24 = 2.0 ** -24
# K: measured by measure_k() below on the CPU, over every plane size of this file, the three residual forms and both layers of the dual
# backward: the largest |same expression in fp64 from the fp32-rounded (mean, invstd, sc, sh) of the reference - pure fp64| / (2^-24 M_i)
# is 7.27 (dx of the second layer at (72, 64), whose |mean| invstd = 2: the rounding of the mean moves xhat m1 by |xhat| |mean| invstd |m1|
# 2^-24, a term M_dx does not hold); y 0.94, dgamma and m2 0.74, dbeta and m1 0 (their expressions hold no rounded coefficient).
# K = 4 x 7.27.  `python tests/test_batchnorm_edges_gpu.py` repeats the measurement without a GPU.
K = 29.1
N0, C0 = 3, 5
WORST = {}


def cdiv(a, b):
    return -(-a // b)


def bn_splits(hw, c, n):
    """bn.hip split_for: ~2048 workgroups, at least 1024 elements of a plane per split, chunks of whole float4s -> (splits, chunk)"""
    splits = max(min(2048 // (c * n), (hw + 1023) // 1024), 1)
    chunk = (cdiv(hw, splits) + 3) & ~3
    return cdiv(hw, chunk), chunk


# ------------------------------------------------------------------------------------------------------- fp32 arithmetic restated on the CPU
def _round32(fr):
    v = np.float32(float(fr))
    cands = [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    return float(min(cands, key=lambda q: (abs(Fraction(float(q)) - fr), int(np.float32(q).view(np.uint32)) & 1)))


def fma32(a, b, c):
    """the fp32 fused multiply-add of small fp32 vectors, exactly: rational arithmetic and ONE rounding to nearest even"""
    a, b, c = (t.detach().float().cpu().flatten().tolist() for t in (a, b, c))
    return torch.tensor([_round32(Fraction(p) * Fraction(q) + Fraction(s)) for p, q, s in zip(a, b, c)], dtype=torch.float32)


def bn_affine(mean, invstd, gamma, beta):
    """common.h bn_affine on fp32 CPU vectors: sc = invstd * gamma (one rounding), sh = fma(-mean, sc, beta)"""
    sc = invstd.float().cpu() * gamma.float().cpu()
    return sc, fma32(-mean.float().cpu(), sc, beta)


def bc(v):
    return v.view(1, -1, 1, 1)


def stats_ref(x):
    xx = x.double()
    mean, var = xx.mean((0, 2, 3)), xx.var((0, 2, 3), unbiased=False)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


# -------------------------------------------------------------------------------------------------------------- inputs and fp64 references
@functools.lru_cache(maxsize=None)
def case(H, W, N=N0, C=C0):
    """CPU inputs of one plane size and the fp64 statistics, computed once and never modified"""
    shape = (N, C, H, W)
    ch = torch.arange(C, dtype=torch.float32).view(1, C, 1, 1)
    d = dict(shape=shape)
    d['x'] = torch.randn(shape, generator=g(1)) * (1 + 0.3 * ch) + 0.5 - 0.2 * ch
    d['r'] = torch.randn(shape, generator=g(2)) * 1.5
    d['dy'] = torch.randn(shape, generator=g(3)) + 0.3
    d['gamma'] = (torch.rand(C, generator=g(4)) + 0.5) * torch.where(torch.arange(C) % 2 == 1, -1.0, 1.0)
    d['beta'] = torch.randn(C, generator=g(5))
    d['post'] = torch.where(torch.arange(N * C).view(N, C) % 4 == 1, 0.0, 1 / 0.9).float()
    assert int((d['post'] == 0).sum()) >= 1
    rm, _, ris = stats_ref(d['r'])
    g2 = (torch.rand(C, generator=g(6)) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    rsc, rsh = bn_affine(rm.float(), ris.float(), g2, torch.randn(C, generator=g(7)) * 0.3)
    d['rcoef'] = torch.stack([rm.float(), ris.float(), rsc, rsh], 1).contiguous()
    d['xb'] = torch.randn(shape, generator=g(8)) * 0.5 - 1.0                       # the second layer of bn_backward_dual
    d['gamma_b'] = -(torch.rand(C, generator=g(9)) + 0.5) * torch.where(torch.arange(C) % 2 == 1, -1.0, 1.0)
    d['mean'], d['var'], d['invstd'] = stats_ref(d['x'])
    return d


def fwd_ref(d, res, coef=None):
    """z = the pre-ReLU, pre-post value in fp64 and M = |x sc| + |mean sc| + |beta| (+ |r| or |r rsc| + |rsh|).  coef = (sc, sh) as fp32
    vectors: the same expression from those rounded coefficients (what measure_k compares with the pure one)"""
    x, gam, bet = d['x'].double(), d['gamma'].double(), d['beta'].double()
    sc = d['invstd'] * gam
    if coef is None:
        z = x * bc(sc) - bc(d['mean'] * sc) + bc(bet)
    else:
        z = x * bc(coef[0].double()) + bc(coef[1].double())
    M = (x * bc(sc)).abs() + bc((d['mean'] * sc).abs() + bet.abs())
    r = d['r'].double()
    if res == 'r':
        z, M = z + r, M + r.abs()
    elif res == 'coef':
        rsc, rsh = d['rcoef'][:, 2].double(), d['rcoef'][:, 3].double()
        z, M = z + r * bc(rsc) + bc(rsh), M + (r * bc(rsc)).abs() + bc(rsh.abs())
    return z, M


@functools.lru_cache(maxsize=None)
def fwd_pure(H, W, res):
    return fwd_ref(case(H, W), res)


def bwd_ref(x, dy, gamma, gate=None, post=None, mean=None, invstd=None):
    """the closed form in fp64.  dz = dy [* post[n, c]] [* gate]; mean / invstd: the pure fp64 statistics of x unless given.
    M_dx = |gs| (|dz| + |m1| + (|xhat| + |mean| invstd + 1) |m2|); M_s1 = sum |dz|; M_s2 = sum |dz| (|x| + |mean|) invstd"""
    N, C, H, W = x.shape
    x, dz, gam = x.double(), dy.double(), gamma.double()
    if post is not None:
        dz = dz * post.double().view(N, C, 1, 1)
    if gate is not None:
        dz = dz * gate.double()
    if mean is None:
        mean, _, invstd = stats_ref(x)
    xhat = (x - bc(mean)) * bc(invstd)
    cnt = N * H * W
    s1, s2 = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    m1, m2, gs = s1 / cnt, s2 / cnt, gam * invstd
    r = dict(dz=dz, cnt=cnt, s1=s1, s2=s2, m1=m1, m2=m2)
    r['dx'] = bc(gs) * (dz - bc(m1) - xhat * bc(m2))
    r['M_dx'] = bc(gs.abs()) * (dz.abs() + bc(m1.abs()) + (xhat.abs() + bc(mean.abs() * invstd) + 1) * bc(m2.abs()))
    r['M_s1'] = dz.abs().sum((0, 2, 3))
    r['M_s2'] = (dz.abs() * (x.abs() + bc(mean.abs())) * bc(invstd)).sum((0, 2, 3))
    return r


A_SIZES = [(1, 1), (1, 3), (3, 4), (12, 21), (16, 16), (32, 32), (4, 257), (72, 64), (53, 87), (4, 1153)]
A_SPLITS = {(1, 1): (1, 4), (1, 3): (1, 4), (3, 4): (1, 12), (12, 21): (1, 252), (16, 16): (1, 256), (32, 32): (1, 1024),
            (4, 257): (2, 516),        # HW % 4 == 0, the second chunk 512 long
            (72, 64): (5, 924),        # HW % 256 == 0: chunks that are no whole 256-element groups under a bitmask; two bn_apply workgroups
            (53, 87): (5, 924),        # odd HW: the scalar path, the last chunk 915 long
            (4, 1153): (5, 924)}       # HW % 4 == 0, not a multiple of 256


def measure_k():
    """the largest |expression in fp64 from the fp32-rounded (mean, invstd, sc, sh) - pure fp64| / (2^-24 M_i), per quantity, over every
    plane size of this file; CPU only"""
    worst = {}

    def note(kind, that, pure, M):
        ok = M > 0
        worst[kind] = max(worst.get(kind, 0.0), float(((that - pure).abs()[ok] / (U24 * M[ok])).max()))

    for (H, W) in A_SIZES:
        d = case(H, W)
        m32, i32 = d['mean'].float(), d['invstd'].float()
        coef = bn_affine(m32, i32, d['gamma'], d['beta'])
        for res in (None, 'r', 'coef'):
            z, M = fwd_ref(d, res)
            note('y', fwd_ref(d, res, coef)[0], z, M)
            for x, gamma, post in ((d['x'], d['gamma'], None), (d['x'], d['gamma'], d['post']), (d['xb'], d['gamma_b'], None)):
                mean, _, invstd = stats_ref(x)
                pure = bwd_ref(x, d['dy'], gamma, z > 0, post)
                that = bwd_ref(x, d['dy'], gamma, z > 0, post, mean.float().double(), invstd.float().double())
                note('dx', that['dx'], pure['dx'], pure['M_dx'])
                note('dgamma', that['s2'], pure['s2'], pure['M_s2'])
                note('dbeta', that['s1'], pure['s1'], pure['M_s1'])
                note('m1', that['m1'], pure['m1'], pure['M_s1'] / pure['cnt'])
                note('m2', that['m2'], pure['m2'], pure['M_s2'] / pure['cnt'])
    return worst


# ------------------------------------------------------------------------------------------------------------------------------ the checks
def note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)


def report():
    print(f'worst error in units of 2^-24 M (the bound is {K}):', {k: f'{v:.3g}' for k, v in sorted(WORST.items())})


def within(got, ref, M, kind, what=''):
    """|got - ref| <= K 2^-24 M for every element (where M is 0 the element must be exact)"""
    got = got.detach().double().cpu().reshape(ref.shape)
    M = M.expand_as(ref) if M.shape != ref.shape else M
    err = (got - ref).abs()
    ok = M > 0
    ratio = float((err[ok] / (U24 * M[ok])).max()) if bool(ok.any()) else 0.0
    note(kind, ratio)
    bad = err > K * U24 * M
    assert not bool(bad.any()), f'{what or kind}: {int(bad.sum())} elements beyond the bound, the worst at {ratio:.3g} x 2^-24 M (K = {K})'


def check_stats(mean, invstd, mean_ref, invstd_ref, what=''):
    m, i = mean.double().cpu(), invstd.double().cpu()
    assert bool(((m - mean_ref).abs() <= 2.0 ** -23 * mean_ref.abs() + 1e-10).all()), f'{what} mean: {(m - mean_ref).tolist()}'
    assert bool(((i - invstd_ref).abs() <= 2.0 ** -23 * invstd_ref).all()), f'{what} invstd: {((i - invstd_ref) / invstd_ref).tolist()}'


def mask_bits(mask, N, C, HW):
    """-> bool [N, C, HW] from the words of bn_apply's bitmask, layout as documented in csrc/bn_bwd.h: the 256-element group q of a plane
    has 4 words; word k, bit l <-> element 256 q + 4 l + k"""
    words = mask.cpu().numpy().view(np.uint64).reshape(N * C, HW // 256, 4)
    bits = ((words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)          # [plane][q][k][l]
    return torch.from_numpy(np.ascontiguousarray(bits.transpose(0, 1, 3, 2)).reshape(N, C, HW))


def check_forward(d, y, relu, res, post, y_nopost=None, mask=None, what=''):
    N, C, H, W = d['shape']
    z, M = fwd_pure(H, W, res)
    p = d['post'].double().view(N, C, 1, 1) if post else torch.ones(N, C, 1, 1, dtype=torch.float64)
    within(y, (z.clamp_min(0) if relu else z) * p, M * p.abs(), 'y', what)
    yk = y.detach().cpu()
    if relu:
        clear = (z.abs() > K * U24 * M) & (p != 0)
        assert bool(((yk > 0) == (z > 0))[clear].all()), f'{what}: the gate differs from the reference away from zero'
    if mask is not None:
        # the bits are formed before the folded factor: they are those of the launch without it
        gate = ((y if y_nopost is None else y_nopost) > 0).cpu().view(N, C, H * W)
        assert torch.equal(mask_bits(mask, N, C, H * W), gate), f'{what}: mask bits != (y > 0)'


@contextlib.contextmanager
def det_mode(ops, on=True):
    before = ops.is_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(before)


@functools.lru_cache(maxsize=None)
def dev(H, W):
    """the device copies of case(H, W): read-only"""
    return {k: v.to(DEV) for k, v in case(H, W).items() if torch.is_tensor(v) and v.dtype == torch.float32}


_KSTATS = {}


def kstats(ops, H, W, key='x'):
    """the kernel's own (mean, invstd) of a case's x (or xb), default mode, checked once"""
    if (H, W, key) not in _KSTATS:
        d = case(H, W)
        mean, invstd = ops.bn_stats(dev(H, W)[key])
        mr, _, ir = stats_ref(d[key])
        check_stats(mean, invstd, mr, ir, f'bn_stats {key} {(H, W)}')
        _KSTATS[H, W, key] = (mean, invstd)
    return _KSTATS[H, W, key]


def bn_ws(ops, C):
    """the fp64 sums (sum dz, sum dz xhat) [C][2] the last bn_backward / bn_stats launch of this stream left in its scratch"""
    return ops._scratch(torch.empty(0, device=DEV).device, 'bn', 2 * C, 8192, torch.float64)[:2 * C].clone().view(C, 2)


REC = np.dtype([('m1', '<f8'), ('m2', '<f8'), ('gs', '<f8'), ('mu', '<f4'), ('is', '<f4'), ('sc', '<f4'), ('sh', '<f4')])


def rec_fields(rec):
    assert REC.itemsize == 40
    return rec.cpu().numpy().view(REC)


def check_rec(rec, R, mean, invstd, gamma, beta, what=''):
    """pfst_bn_bwd_rec_t per channel: (m1, m2) within their bounds, gs = gamma * invstd exactly in fp64, (mu, is) as passed, (sc, sh) = bn_affine"""
    f = rec_fields(rec)
    within(torch.from_numpy(f['m1'].copy()), R['m1'], R['M_s1'] / R['cnt'], 'm1', what + ' m1')
    within(torch.from_numpy(f['m2'].copy()), R['m2'], R['M_s2'] / R['cnt'], 'm2', what + ' m2')
    assert torch.equal(torch.from_numpy(f['gs'].copy()), gamma.double().cpu() * invstd.double().cpu())
    assert torch.equal(torch.from_numpy(f['mu'].copy()), mean.cpu()) and torch.equal(torch.from_numpy(f['is'].copy()), invstd.cpu())
    sc, sh = bn_affine(mean, invstd, gamma, beta)
    assert torch.equal(torch.from_numpy(f['sc'].copy()), sc) and torch.equal(torch.from_numpy(f['sh'].copy()), sh)


def amax_is(am, t, what=''):
    assert float(am.max()) == float(t.abs().max()), f'{what}: published maximum {float(am.max())} != max |written| {float(t.abs().max())}'


# =============================================================================================================================== A: plane sizes
@pytest.mark.parametrize('H,W', A_SIZES)
def test_a_plane_sizes(ops, H, W):
    """bn_stats (plain, with running statistics, with the coefficient record), bn_apply and bn_backward on contiguous tensors of every
    chunking class"""
    d, t = case(H, W), dev(H, W)
    N, C, HW = N0, C0, H * W
    assert bn_splits(HW, C, N) == A_SPLITS[H, W]
    mean, invstd = kstats(ops, H, W)
    rm0, rv0 = torch.randn(C, generator=g(20)), torch.rand(C, generator=g(21)) + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    m2, i2, coef = ops.bn_stats(t['x'], rm, rv, 0.1, EPS, gamma=t['gamma'], beta=t['beta'])
    check_stats(m2, i2, d['mean'], d['invstd'], 'bn_stats with running statistics')
    cnt = N * HW
    assert_close(rm, 0.9 * rm0.double() + 0.1 * d['mean'], 1e-5, 'running_mean')
    assert_close(rv, 0.9 * rv0.double() + 0.1 * d['var'] * cnt / (cnt - 1), 1e-5, 'running_var')
    sc, sh = bn_affine(m2, i2, t['gamma'], t['beta'])
    cf = coef.cpu()
    assert torch.equal(cf[:, 0], m2.cpu()) and torch.equal(cf[:, 1], i2.cpu()) and torch.equal(cf[:, 2], sc) and torch.equal(cf[:, 3], sh)
    for relu in (True, False):
        y = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], relu)
        check_forward(d, y, relu, None, False, what=f'bn_apply relu={relu}')
        gate = (y > 0).cpu() if relu else None
        R = bwd_ref(d['x'], d['dy'], d['gamma'], gate)
        for src in (('recomputed', 'y') if relu else ('none',)):
            dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            dx = ops.bn_backward(t['dy'], y if src == 'y' else None, t['x'], mean, invstd, t['gamma'], dg, db, relu, beta=t['beta'])
            within(dx, R['dx'], R['M_dx'], 'dx', f'dx gate {src}')
            within(dg, R['s2'], R['M_s2'], 'dgamma')
            within(db, R['s1'], R['M_s1'], 'dbeta')
    report()


# ================================================================================================================================= B: options
B_SHAPES = [(72, 64), (53, 87), (3, 4)]


@pytest.mark.parametrize('H,W', B_SHAPES)
def test_b_apply_options(ops, H, W):
    """{relu} x {no residual, residual, residual normalised on load} x {post, only without residual} x {amax} x {want_mask}"""
    d, t = case(H, W), dev(H, W)
    N, C, HW = N0, C0, H * W
    mean, invstd = kstats(ops, H, W)
    for relu in (True, False):
        for res in (None, 'r', 'coef'):
            y0 = None
            for post in ((False, True) if res is None else (False,)):
                for want_amax in (False, True):
                    for want_mask in (False, True):
                        what = f'bn_apply relu={relu} res={res} post={post} amax={want_amax} mask={want_mask}'
                        am = ops.amax_slots(t['x'].device) if want_amax else None
                        out = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], relu, t['r'] if res else None, want_mask=want_mask,
                                           amax=am, post=t['post'] if post else None, residual_coef=t['rcoef'] if res == 'coef' else None)
                        y, mask = out if want_mask else (out, None)
                        assert (mask is not None) == (want_mask and relu and HW % 256 == 0), what
                        if y0 is None:
                            y0 = y
                        # the options change nothing in the values: one launch without them, then one fp32 product with the folded factor
                        assert torch.equal(y, y0 * t['post'].view(N, C, 1, 1) if post else y0), what
                        check_forward(d, y, relu, res, post, y0, mask, what)
                        if want_amax:
                            amax_is(am, y, what)
    report()


@pytest.mark.parametrize('H,W', B_SHAPES)
def test_b_backward_options(ops, H, W):
    """{gate from the mask, from y, recomputed from x and beta, relu=False} x {no dres, written, accumulated} x {post where the ABI allows it}
    x {amax}; dgamma / dbeta added into nonzero buffers, and one launch each without them; relu_gate_"""
    d, t = case(H, W), dev(H, W)
    N, C, HW = N0, C0, H * W
    mean, invstd = kstats(ops, H, W)
    fw = {}

    def forward(res, post):
        if (res, post) not in fw:
            fw[res, post] = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], True, t['r'] if res else None, want_mask=True,
                                         post=t['post'] if post else None)
        return fw[res, post]

    dg0, db0, old = torch.randn(C, generator=g(30)), torch.randn(C, generator=g(31)), torch.randn(d['shape'], generator=g(32)).to(DEV)
    zero = torch.zeros((), device=DEV)
    for gk in ('mask', 'y', 'recomputed', 'none'):
        if gk == 'mask' and HW % 256:
            continue
        for dres_mode in (None, 'write', 'acc'):
            for post in ((False, True) if dres_mode is None else (False,)):
                for want_amax in (False, True):
                    what = f'bn_backward gate={gk} dres={dres_mode} post={post} amax={want_amax}'
                    relu = gk != 'none'
                    yk, mk = forward(gk in ('mask', 'y') and not post, post) if relu else (None, None)
                    assert gk != 'mask' or mk is not None
                    gate = (yk > 0) if relu else None
                    dg, db = dg0.to(DEV), db0.to(DEV)
                    dres = None if dres_mode is None else old.clone() if dres_mode == 'acc' else torch.full(d['shape'], SENT, device=DEV)
                    am = ops.amax_slots(t['x'].device) if want_amax else None
                    dx = ops.bn_backward(t['dy'], yk if gk == 'y' else None, t['x'], mean, invstd, t['gamma'], dg, db, relu, dres, dres_mode == 'acc',
                                         beta=t['beta'] if gk == 'recomputed' else None, mask=mk if gk == 'mask' else None, amax=am,
                                         post=t['post'] if post else None)
                    R = bwd_ref(d['x'], d['dy'], d['gamma'], None if gate is None else gate.cpu(), d['post'] if post else None)
                    within(dx, R['dx'], R['M_dx'], 'dx', what)
                    within(dg, dg0.double() + R['s2'], dg0.double().abs() + R['M_s2'], 'dgamma', what + ' dgamma')
                    within(db, db0.double() + R['s1'], db0.double().abs() + R['M_s1'], 'dbeta', what + ' dbeta')
                    if dres is not None:
                        dz = t['dy'] if gate is None else torch.where(gate, t['dy'], zero)
                        assert torch.equal(dres, old + dz if dres_mode == 'acc' else dz), what + ': dres'
                    if want_amax:
                        amax_is(am, dx, what)
    # one launch each without a dgamma and without a dbeta buffer
    y, _ = forward(False, False)
    R = bwd_ref(d['x'], d['dy'], d['gamma'], (y > 0).cpu())
    for skip in ('dgamma', 'dbeta'):
        dg, db = (None, db0.to(DEV)) if skip == 'dgamma' else (dg0.to(DEV), None)
        dx = ops.bn_backward(t['dy'], None, t['x'], mean, invstd, t['gamma'], dg, db, True, beta=t['beta'])
        within(dx, R['dx'], R['M_dx'], 'dx', f'without {skip}')
        if dg is not None:
            within(dg, dg0.double() + R['s2'], dg0.double().abs() + R['M_s2'], 'dgamma')
        if db is not None:
            within(db, db0.double() + R['s1'], db0.double().abs() + R['M_s1'], 'dbeta')
    if HW % 256 == 0:
        y, mask = forward(True, False)
        gated = torch.where(y > 0, t['dy'], zero)
        out = torch.full(d['shape'], SENT, device=DEV)
        assert torch.equal(ops.relu_gate_(out, t['dy'], mask), gated)
        assert torch.equal(ops.relu_gate_(old.clone(), t['dy'], mask, accumulate=True), old + gated)
    report()


# =================================================================================================================================== C: views
C_SHAPES = [(16, 16), (72, 64), (12, 21)]
KINDS = {'slice': dict(front=2, back=3),              # (i) channels [2, 2 + C) of a (C + 5)-channel buffer: aligned planes, the parent's stride
         'lead': dict(front=1, back=3, lead=1),       # (ii) every plane 4 bytes past a 16-byte boundary
         'odd': dict(front=0, back=0, odd=1)}         # (iii) odd batch stride: image 0 aligned, images 1 and 2 not
c_views = pytest.mark.parametrize('kind', list(KINDS))
c_shapes = pytest.mark.parametrize('H,W', C_SHAPES)


def aligned(t):
    """what the host (and hip_ops, for the mask) asks of an operand before it takes the float4 route"""
    return t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0


class Operands:
    """the operands of one call: those named in `viewed` are views of `kind` inside canary buffers, the others plain tensors.  Inputs are
    snapshotted; after the call check() asserts that every input's parent buffer is unchanged and every output's canaries are intact"""

    def __init__(self, kind, viewed, shape):
        self.kind, self.viewed, self.shape, self.inputs, self.outputs = kind, viewed, shape, [], []

    def kw(self, role):
        return KINDS[self.kind] if role in self.viewed else dict(front=0, back=0)

    def src(self, role, t):
        gd = Guard(self.shape, **self.kw(role))
        gd.put(t)
        if role in self.viewed and self.kind != 'slice':
            assert not aligned(gd.view) or self.shape[2] * self.shape[3] % 4
        self.inputs.append((role, gd, gd.flat.clone()))
        return gd.view

    def dst(self, role, fill=None):
        gd = Guard(self.shape, **self.kw(role))
        if fill is not None:
            gd.put(fill)
        self.outputs.append((role, gd))
        return gd.view

    def check(self, what=''):
        for role, gd, before in self.inputs:
            assert torch.equal(gd.flat, before), f'{what}: the read-only operand {role} was written'
        for role, gd in self.outputs:
            gd.intact(f'{what}: {role}')

    def all_aligned(self):
        return self.kind == 'slice' or not self.viewed


def test_guard_kinds():
    """the three view kinds are what their names say (HW % 4 == 0 planes)"""
    shape = (N0, C0, 8, 8)
    a, b, c = (Guard(shape, **KINDS[k]).view for k in ('slice', 'lead', 'odd'))
    assert a.stride(0) == (C0 + 5) * 64 and a.data_ptr() % 16 == 0 and aligned(a)
    assert b.data_ptr() % 16 == 4 and b.stride(0) % 4 == 0
    assert c.data_ptr() % 16 == 0 and c.stride(0) == C0 * 64 + 1 and [c[n].data_ptr() % 16 for n in range(3)] == [0, 4, 8]


_BASE = {}


def base(ops, H, W):
    """the contiguous launches of one shape: forward with residual (y, mask) and its backward (dx, dres, dgamma, dbeta)"""
    if (H, W) not in _BASE:
        t = dev(H, W)
        mean, invstd = kstats(ops, H, W)
        y, mask = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], True, t['r'], want_mask=True)
        check_forward(case(H, W), y, True, 'r', False, mask=mask, what='contiguous forward')
        _BASE[H, W] = dict(y=y, mask=mask)
    return _BASE[H, W]


@pytest.mark.parametrize('which', ['x', 'residual', 'out', 'all'])
@c_views
@c_shapes
def test_c_apply_on_views(ops, H, W, kind, which):
    """bn_stats and bn_apply with x, the residual and the output in turn, then all, as views: bit for bit the contiguous launch (the vector
    and the scalar path are one fma and the same adds), a mask exactly where every operand is aligned, canaries intact, inputs unread-only"""
    d, t = case(H, W), dev(H, W)
    N, C, HW = N0, C0, H * W
    mean, invstd = kstats(ops, H, W)
    b = base(ops, H, W)
    viewed = ('x', 'residual', 'out') if which == 'all' else (which,)
    o = Operands(kind, viewed, d['shape'])
    xv, rv, ov = o.src('x', t['x']), o.src('residual', t['r']), o.dst('out')
    if 'x' in viewed:
        ms, is_ = ops.bn_stats(xv)
        check_stats(ms, is_, d['mean'], d['invstd'], f'bn_stats on a {kind} view')
    am = ops.amax_slots(xv.device)
    y, mask = ops.bn_apply(xv, mean, invstd, t['gamma'], t['beta'], True, rv, out=ov, want_mask=True, amax=am)
    what = f'bn_apply {kind} view of {which}'
    assert y.data_ptr() == ov.data_ptr()
    assert (mask is not None) == (HW % 256 == 0 and o.all_aligned()), what
    assert all(aligned(v) for v in (xv, rv, ov)) == o.all_aligned()
    o.check(what)
    assert torch.equal(y, b['y']), what + ': differs from the contiguous launch'
    check_forward(d, y, True, 'r', False, mask=mask, what=what)
    assert mask is None or torch.equal(mask, b['mask'])
    amax_is(am, y, what)
    # the residual normalised on load and the folded factor on the same views
    y2 = ops.bn_apply(xv, mean, invstd, t['gamma'], t['beta'], True, rv, out=ov, residual_coef=t['rcoef'])
    check_forward(d, y2, True, 'coef', False, what=what + ', residual_coef')
    y3 = ops.bn_apply(xv, mean, invstd, t['gamma'], t['beta'], True, out=ov, post=t['post'])
    check_forward(d, y3, True, None, True, what=what + ', post')
    o.check(what)
    report()


@pytest.mark.parametrize('which', ['dy', 'y', 'x', 'dx', 'dres', 'all'])
@c_views
@c_shapes
def test_c_backward_on_views(ops, H, W, kind, which):
    """bn_backward (gate from y; dres written, then accumulated; gate from the mask where there is one), bn_backward_sums and relu_gate_
    with each operand in turn, then all, as views"""
    d, t = case(H, W), dev(H, W)
    N, C, HW = N0, C0, H * W
    mean, invstd = kstats(ops, H, W)
    b = base(ops, H, W)
    gate = b['y'] > 0
    R = bwd_ref(d['x'], d['dy'], d['gamma'], gate.cpu())
    viewed = ('dy', 'y', 'x', 'dx', 'dres') if which == 'all' else (which,)
    old = torch.randn(d['shape'], generator=g(32)).to(DEV)
    dz = torch.where(gate, t['dy'], torch.zeros((), device=DEV))
    for mode in ('write', 'acc') + (('mask',) if HW % 256 == 0 else ()):
        what = f'bn_backward {kind} view of {which}, {mode}'
        o = Operands(kind, viewed, d['shape'])
        dyv, yv, xv = o.src('dy', t['dy']), o.src('y', b['y']), o.src('x', t['x'])
        dxv, drv = o.dst('dx'), o.dst('dres', old if mode == 'acc' else None)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        am = ops.amax_slots(xv.device)
        dx = ops.bn_backward(dyv, None if mode == 'mask' else yv, xv, mean, invstd, t['gamma'], dg, db, True, drv, mode == 'acc', dx=dxv,
                             mask=b['mask'] if mode == 'mask' else None, amax=am)
        assert dx.data_ptr() == dxv.data_ptr()
        o.check(what)
        within(dx, R['dx'], R['M_dx'], 'dx', what)
        within(dg, R['s2'], R['M_s2'], 'dgamma', what + ' dgamma')
        within(db, R['s1'], R['M_s1'], 'dbeta', what + ' dbeta')
        assert torch.equal(drv, old + dz if mode == 'acc' else dz), what + ': dres'
        amax_is(am, dx, what)
    if which in ('dy', 'x', 'all'):
        # the first half alone (the gate recomputed from x and beta: the forward without a residual)
        y1 = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], True)
        R1 = bwd_ref(d['x'], d['dy'], d['gamma'], (y1 > 0).cpu())
        o = Operands(kind, tuple(v for v in viewed if v in ('dy', 'x')), d['shape'])
        dyv, xv = o.src('dy', t['dy']), o.src('x', t['x'])
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        rec = ops.bn_backward_sums(dyv, xv, mean, invstd, t['gamma'], t['beta'], dg, db)
        o.check('bn_backward_sums')
        check_rec(rec, R1, mean, invstd, t['gamma'], t['beta'], f'bn_backward_sums {kind} view of {which}')
        within(dg, R1['s2'], R1['M_s2'], 'dgamma')
        within(db, R1['s1'], R1['M_s1'], 'dbeta')
    if HW % 256 == 0 and which in ('dy', 'dx', 'all'):
        for acc in (False, True):
            o = Operands(kind, ('g', 'out') if which == 'all' else ('g',) if which == 'dy' else ('out',), d['shape'])
            gv, ov = o.src('g', t['dy']), o.dst('out', old if acc else None)
            ops.relu_gate_(ov, gv, b['mask'], accumulate=acc)
            o.check(f'relu_gate_ {kind} view of {which}')
            assert torch.equal(ov, old + dz if acc else dz)
    report()


# ============================================================================================================================= D: slot tables
D_T = [1, 2, 3, 255, 256, 1023, 1025, 4095, 4096, 4097, 8194]
D_C, D_PER = 3, 64
SUM64 = 2.0 ** -39         # slot_sum_bound


def slot_sum_bound(M):
    """fp64 sums of at most 8194 fp32 slots, read back as fp64: each of the T - 1 adds rounds to 2^-53 of a partial sum that is at most the
    sum of the magnitudes, T 2^-53 <= 2^-39 of it in all (the products with mean and invstd add three roundings of 2^-53 each)"""
    return SUM64 * M


@functools.lru_cache(maxsize=None)
def slot_table(T):
    """part[C][T][2] = (sum, sum of squares) of T slots of D_PER values each, the (minimum, maximum) table behind it; C = 3, so that with an
    odd T channel 1 of the sums (and channels 0 and 2 of the extrema) starts on an 8-byte boundary: the scalar fallback beside the float4
    loop with its one-slot tail.  The first and the last slot carry the largest sums"""
    C = D_C
    ch = torch.arange(C, dtype=torch.float32).view(C, 1)
    s = torch.randn(C, T, generator=g(50)) * 8 + 6.4 * (ch - 0.8)
    s[:, 0] += 40
    s[:, -1] -= 55
    q = s * s / D_PER + D_PER * (torch.rand(C, T, generator=g(51)) + 0.5) * (1 + ch)
    lo = -torch.rand(C, T, generator=g(52)) * 3 - 0.01 * (1 + ch)
    hi = torch.rand(C, T, generator=g(53)) * 3 + 0.02 * (1 + ch)
    lo[:, -1] -= 2.5                       # the channel's extrema sit in the last slot and in the first
    hi[:, 0] += 1.5
    part, mm = torch.stack([s, q], 2).contiguous(), torch.stack([lo, hi], 2).contiguous()
    return part, mm


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('T', D_T)
def test_d_finalize_partials(ops, T, relu):
    """mean, invstd, coef, running statistics and the predicted maximum from synthesised slot tables: 256 / 1024 threads (T >= 4096), the odd
    tail, the scalar fallback"""
    C = D_C
    part, mm = slot_table(T)
    count = float(T * D_PER)
    stats = torch.cat([part.flatten(), mm.flatten()]).to(DEV)
    assert stats.data_ptr() % 16 == 0
    tot = part.double().sum(1)
    mean_ref = tot[:, 0] / count
    var_ref = tot[:, 1] / count - mean_ref * mean_ref
    assert float(var_ref.min()) > 0.1
    invstd_ref = 1.0 / torch.sqrt(var_ref + EPS)
    gamma, beta = torch.tensor([1.3, -0.7, 0.9]), torch.tensor([0.2, -0.4, -3.5])
    rm0, rv0 = torch.randn(C, generator=g(20)), torch.rand(C, generator=g(21)) + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    am = ops.amax_slots(stats.device)
    mean, invstd, coef = ops.bn_finalize_partials(stats, T, C, count, rm, rv, 0.1, EPS, gamma.to(DEV), beta.to(DEV), predict_amax=am, relu=relu)
    check_stats(mean, invstd, mean_ref, invstd_ref, f'bn_finalize_partials T={T}')
    assert_close(rm, 0.9 * rm0.double() + 0.1 * mean_ref, 1e-5, 'running_mean')
    assert_close(rv, 0.9 * rv0.double() + 0.1 * var_ref * count / (count - 1), 1e-5, 'running_var')
    sc, sh = bn_affine(mean, invstd, gamma, beta)
    cf = coef.cpu()
    assert torch.equal(cf[:, 0], mean.cpu()) and torch.equal(cf[:, 1], invstd.cpu()) and torch.equal(cf[:, 2], sc) and torch.equal(cf[:, 3], sh)
    # the predicted maximum: the images of the channel's extreme inputs under the returned coefficients, in fp32
    lo, hi = mm[:, :, 0].min(1)[0], mm[:, :, 1].max(1)[0]
    ya, yb = fma32(lo, sc, sh), fma32(hi, sc, sh)
    want = torch.maximum(ya, yb).clamp_min(0) if relu else torch.maximum(ya.abs(), yb.abs())
    got = am.cpu()
    assert torch.equal(got[:C], want), (got[:C].tolist(), want.tolist())
    assert float(got[C:].abs().max()) == 0.0
    assert float(want[2]) == 0.0 or not relu        # beta[2] = -3.5: both images negative, nothing to publish under the ReLU
    # without the extrema, without gamma / beta: the same statistics, bit for bit
    m3, i3 = ops.bn_finalize_partials(stats, T, C, count)
    assert torch.equal(m3, mean) and torch.equal(i3, invstd)


@pytest.mark.parametrize('T', D_T)
def test_d_backward_partials(ops, T):
    """the same tables as the (sum dz, sum dz x) partials of bn_backward and bn_backward_sums: ws[2c] = sum, ws[2c + 1] = invstd (sum dz x -
    mean sum dz) in fp64, read back from the scratch and from the record; dx, dgamma, dbeta from those sums"""
    C, N, H, W = D_C, 2, 3, 4
    part, _ = slot_table(T)
    pd = part.to(DEV)
    x = torch.randn(N, C, H, W, generator=g(60)) + 0.5
    dy = torch.randn(N, C, H, W, generator=g(61))
    mean, invstd = torch.tensor([0.31, -0.57, 1.9]), torch.tensor([0.83, 1.7, 0.45])
    gamma, beta = torch.tensor([1.3, -0.7, 0.9]), torch.tensor([0.2, -0.4, -3.5])
    md, isd, gd, bd = mean.to(DEV), invstd.to(DEV), gamma.to(DEV), beta.to(DEV)
    p64, mu, is_ = part.double(), mean.double(), invstd.double()
    s1 = p64[:, :, 0].sum(1)
    s2 = is_ * (p64[:, :, 1].sum(1) - mu * s1)
    M1 = p64[:, :, 0].abs().sum(1)
    M2 = is_ * (p64[:, :, 1].abs().sum(1) + mu.abs() * M1)

    def sums_ok(a, b, scale, what):
        assert bool(((a - s1 * scale).abs() <= slot_sum_bound(M1 * scale)).all()), f'{what} [0]: {(a - s1 * scale).tolist()}'
        assert bool(((b - s2 * scale).abs() <= slot_sum_bound(M2 * scale)).all()), f'{what} [1]: {(b - s2 * scale).tolist()}'

    dg0, db0 = torch.randn(C, generator=g(30)), torch.randn(C, generator=g(31))
    dg, db = dg0.to(DEV), db0.to(DEV)
    dx = ops.bn_backward(dy.to(DEV), None, x.to(DEV), md, isd, gd, dg, db, False, partials=pd, slots=T)
    ws = bn_ws(ops, C).cpu()
    sums_ok(ws[:, 0], ws[:, 1], 1.0, f'bn_backward partials T={T}')
    # the apply pass with the sums it was given
    cnt = N * H * W
    dz, xhat = dy.double(), (x.double() - bc(mu)) * bc(is_)
    m1, m2, gs = s1 / cnt, s2 / cnt, gamma.double() * is_
    within(dx, bc(gs) * (dz - bc(m1) - xhat * bc(m2)), bc(gs.abs()) * (dz.abs() + bc(m1.abs()) + (xhat.abs() + bc(mu.abs() * is_) + 1) * bc(m2.abs())),
           'dx', f'dx from partials T={T}')
    within(dg, dg0.double() + s2, dg0.double().abs() + M2, 'dgamma')
    within(db, db0.double() + s1, db0.double().abs() + M1, 'dbeta')
    dg, db = dg0.to(DEV), db0.to(DEV)
    rec = ops.bn_backward_sums(dy.to(DEV), x.to(DEV), md, isd, gd, bd, dg, db, partials=pd, slots=T)
    f = rec_fields(rec)
    sums_ok(torch.from_numpy(f['m1'].copy()), torch.from_numpy(f['m2'].copy()), 1.0 / cnt, f'bn_backward_sums partials T={T}')
    within(dg, dg0.double() + s2, dg0.double().abs() + M2, 'dgamma')
    within(db, db0.double() + s1, db0.double().abs() + M1, 'dbeta')
    report()


# ========================================================================================================================= E: bn_backward_dual
E_SHAPES = [(32, 32), (72, 64)]


def dual_sides(ops, H, W, dgb):
    t = dev(H, W)
    sides = {}
    for k, xk, gk in (('a', 'x', 'gamma'), ('b', 'xb', 'gamma_b')):
        mean, invstd = kstats(ops, H, W, xk)
        sides[k] = dict(mean=mean, invstd=invstd, gamma=t[gk], dgamma=dgb[k][0].to(DEV), dbeta=dgb[k][1].to(DEV))
    return sides


def slot_partials(dz, x, T_per_image=4):
    """(sum dz, sum dz x) per slot as a data-gradient epilogue would emit them: [C][N * 4][2] in fp32 (each plane in four pieces)"""
    N, C, H, W = x.shape
    a = dz.double().view(N, C, T_per_image, -1)
    b = (dz.double() * x.double()).view(N, C, T_per_image, -1)
    part = torch.stack([a.sum(3), b.sum(3)], 3).permute(1, 0, 2, 3).reshape(C, N * T_per_image, 2)
    return part.float().contiguous()


@pytest.mark.parametrize('partials', [False, True])
@pytest.mark.parametrize('amax', [False, True])
@pytest.mark.parametrize('H,W', E_SHAPES)
def test_e_dual(ops, H, W, amax, partials):
    """both layers against fp64 (different x, gamma, statistics per side), dy / xa / xb as channel slices, dgamma / dbeta into nonzero buffers"""
    d, t = case(H, W), dev(H, W)
    N, C = N0, C0
    b = base(ops, H, W)
    gate = (b['y'] > 0)
    dgb = {k: (torch.randn(C, generator=g(70 + i)), torch.randn(C, generator=g(72 + i))) for i, k in enumerate('ab')}
    sides = dual_sides(ops, H, W, dgb)
    o = Operands('slice', ('dy', 'xa', 'xb'), d['shape'])
    dyv = o.src('dy', t['dy'])
    sides['a']['x'], sides['b']['x'] = o.src('xa', t['x']), o.src('xb', t['xb'])
    if amax:
        sides['a']['amax'], sides['b']['amax'] = ops.amax_slots(dyv.device), ops.amax_slots(dyv.device)
    dzc = d['dy'].double() * gate.cpu()
    if partials:
        sides['a']['partials'], sides['a']['slots'] = slot_partials(dzc, d['x']).to(DEV), N * 4
    both = ops.bn_backward_dual(dyv, b['mask'], sides['a'], sides['b'])
    assert both is not None
    o.check('bn_backward_dual')
    for k, xk, gk, dx in (('a', 'x', 'gamma', both[0]), ('b', 'xb', 'gamma_b', both[1])):
        R = bwd_ref(d[xk], d['dy'], d[gk], gate.cpu())
        what = f'dual side {k} partials={partials}'
        within(dx, R['dx'], R['M_dx'], 'dx', what)
        within(sides[k]['dgamma'], dgb[k][0].double() + R['s2'], dgb[k][0].double().abs() + R['M_s2'], 'dgamma', what + ' dgamma')
        within(sides[k]['dbeta'], dgb[k][1].double() + R['s1'], dgb[k][1].double().abs() + R['M_s1'], 'dbeta', what + ' dbeta')
        if amax:
            amax_is(sides[k]['amax'], dx, what)
    report()


# (N, C, H, W), chunks per plane: every channel's fp64 sums have at most two addends into a zeroed ws (N * chunks <= 2), so the order of the
# atomics cannot matter (0 + a is exact, a + b commutes) and the default mode's sums are reproducible bit for bit
DUAL_EQ = [((2, 5, 16, 16), 1),        # one mask group per plane
           ((2, 5, 32, 32), 1),        # HW = 1024
           ((1, 5, 32, 64), 2)]        # two chunks per plane, walked in reversed order


@pytest.mark.parametrize('partials', [False, True])
@pytest.mark.parametrize('shape,chunks', DUAL_EQ)
def test_e_dual_equals_two_single_layers(ops, shape, chunks, partials):
    """bn_backward_dual == two bn_backward(mask=...) calls BIT FOR BIT: dx, dgamma, dbeta, the published maximum and the fp64 sums in ws, with
    and without side a's sums arriving as partials, dy / xa / xb as channel slices.  The kernels of both routes take every element's
    arithmetic from csrc/bn_bwd.h (bn_bwd_dx pins the roundings of the projection) and sum in the same order inside a workgroup; this test
    holds them to it.  pfst_bn_backward_dual is called through the C ABI with a scratch of the test's own, so that ws can be read back (the
    wrapper allocates and drops it)."""
    N, C, H, W = shape
    HW = H * W
    assert bn_splits(HW, C, N)[0] == chunks and N * chunks <= 2
    d = case(H, W, N, C)
    t = {k: d[k].to(DEV) for k in ('x', 'xb', 'r', 'dy', 'gamma', 'gamma_b', 'beta')}
    stats = {'a': ops.bn_stats(t['x']), 'b': ops.bn_stats(t['xb'])}
    y, mask = ops.bn_apply(t['x'], *stats['a'], t['gamma'], t['beta'], True, t['r'], want_mask=True)
    assert mask is not None
    dgb = {k: (torch.randn(C, generator=g(70 + i)), torch.randn(C, generator=g(72 + i))) for i, k in enumerate('ab')}
    o = Operands('slice', ('dy', 'xa', 'xb'), shape)
    dyv, xv = o.src('dy', t['dy']), {'a': o.src('xa', t['x']), 'b': o.src('xb', t['xb'])}
    gam = {'a': t['gamma'], 'b': t['gamma_b']}
    part = slot_partials(d['dy'].double() * (y > 0).cpu(), d['x']).to(DEV) if partials else None
    single = {}
    for k in 'ab':
        dg, db, am = dgb[k][0].to(DEV), dgb[k][1].to(DEV), ops.amax_slots(dyv.device)
        kw = dict(partials=part, slots=N * 4) if partials and k == 'a' else {}
        dx = ops.bn_backward(dyv, None, xv[k], *stats[k], gam[k], dg, db, True, mask=mask, amax=am, **kw)
        single[k] = dict(dx=dx, dgamma=dg, dbeta=db, amax=float(am.max()), ws=bn_ws(ops, C))
    dual = {k: dict(dx=torch.full(shape, SENT, device=DEV), dgamma=dgb[k][0].to(DEV), dbeta=dgb[k][1].to(DEV), amax=ops.amax_slots(dyv.device),
                    ws=torch.full((C, 2), SENT, dtype=torch.float64, device=DEV)) for k in 'ab'}
    A, B = dual['a'], dual['b']
    ops.call('pfst_bn_backward_dual', dyv.data_ptr(), ops._bs(dyv), mask.data_ptr(),
             xv['a'].data_ptr(), ops._bs(xv['a']), stats['a'][0].data_ptr(), stats['a'][1].data_ptr(), gam['a'].data_ptr(), A['dx'].data_ptr(), C * HW,
             A['dgamma'].data_ptr(), A['dbeta'].data_ptr(), A['ws'].data_ptr(), ops._p(part), N * 4 if partials else 0, A['amax'].data_ptr(),
             xv['b'].data_ptr(), ops._bs(xv['b']), stats['b'][0].data_ptr(), stats['b'][1].data_ptr(), gam['b'].data_ptr(), B['dx'].data_ptr(), C * HW,
             B['dgamma'].data_ptr(), B['dbeta'].data_ptr(), B['ws'].data_ptr(), B['amax'].data_ptr(), N, C, HW, ops._stream())
    o.check('bn_backward_dual')
    for k in 'ab':
        what = f'side {k} of {shape}, partials={partials}'
        for f in ('ws', 'dgamma', 'dbeta', 'dx'):
            assert torch.equal(dual[k][f], single[k][f]), f'{what}: {f} differs from the single-layer call'
        assert float(dual[k]['amax'].max()) == single[k]['amax'] == float(single[k]['dx'].abs().max()), what + ': published maximum'


@pytest.mark.parametrize('H,W,bad', [(32, 32, 'dy'), (32, 32, 'xa'), (32, 32, 'xb'), (12, 21, None)])
def test_e_dual_declines(ops, monkeypatch, H, W, bad):
    """a plane 4 bytes past a 16-byte boundary, or HW % 256 != 0: the wrapper returns None and launches nothing"""
    d, t = case(H, W), dev(H, W)
    N, C, HW = N0, C0, H * W
    dgb = {k: (torch.randn(C, generator=g(70 + i)), torch.randn(C, generator=g(72 + i))) for i, k in enumerate('ab')}
    sides = dual_sides(ops, H, W, dgb)
    o = Operands('lead', (bad,), d['shape'])
    dyv = o.src('dy', t['dy'])
    sides['a']['x'], sides['b']['x'] = o.src('xa', t['x']), o.src('xb', t['xb'])
    sides['a']['amax'], sides['b']['amax'] = ops.amax_slots(dyv.device), ops.amax_slots(dyv.device)
    mask = base(ops, H, W)['mask'] if HW % 256 == 0 else torch.full((N * C * HW // 64,), 0x5555, dtype=torch.int64, device=DEV)
    seen, call = [], ops.call
    monkeypatch.setattr(ops, 'call', lambda name, *a: (seen.append(name), call(name, *a))[1])
    assert ops.bn_backward_dual(dyv, mask, sides['a'], sides['b']) is None
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert not [name for name in seen if name != 'pfst_get_deterministic'], seen
    o.check('bn_backward_dual declined')
    for i, k in enumerate('ab'):
        assert torch.equal(sides[k]['dgamma'].cpu(), dgb[k][0]) and torch.equal(sides[k]['dbeta'].cpu(), dgb[k][1])
        assert float(sides[k]['amax'].max()) == 0.0
    assert HW % 256 == 0 or bool((mask == 0x5555).all())


# ========================================================================================================================= F: deterministic mode
def test_f_deterministic_ragged_scalar(ops):
    """(53, 87), contiguous: statistics, apply and backward twice under set_deterministic(True): bit-equal, and within the same bounds"""
    H, W = 53, 87
    d, t = case(H, W), dev(H, W)
    C = C0
    runs = []
    with det_mode(ops):
        for _ in range(2):
            mean, invstd = ops.bn_stats(t['x'])
            y = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], True)
            dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            dx = ops.bn_backward(t['dy'], None, t['x'], mean, invstd, t['gamma'], dg, db, True, beta=t['beta'])
            ws = bn_ws(ops, C)
            rec = ops.bn_backward_sums(t['dy'], t['x'], mean, invstd, t['gamma'], t['beta'], None, None)
            runs.append((mean, invstd, y, dx, dg, db, ws, rec))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    mean, invstd, y, dx, dg, db, ws, rec = runs[0]
    check_stats(mean, invstd, d['mean'], d['invstd'], 'deterministic bn_stats')
    check_forward(d, y, True, None, False, what='deterministic bn_apply')
    R = bwd_ref(d['x'], d['dy'], d['gamma'], (y > 0).cpu())
    within(dx, R['dx'], R['M_dx'], 'dx', 'deterministic dx')
    within(dg, R['s2'], R['M_s2'], 'dgamma')
    within(db, R['s1'], R['M_s1'], 'dbeta')
    check_rec(rec, R, mean, invstd, t['gamma'], t['beta'], 'deterministic bn_backward_sums')
    # the record and bn_backward's scratch hold the same ordered sums
    f = rec_fields(rec)
    inv = 1.0 / R['cnt']
    assert np.array_equal(f['m1'], (ws[:, 0].cpu() * inv).numpy()) and np.array_equal(f['m2'], (ws[:, 1].cpu() * inv).numpy())
    report()


def test_f_deterministic_routes(ops):
    """(72, 64) under set_deterministic(True).  All operands with an odd batch stride: bit-equal across two launches and within the bounds.
    Then ONE operand at a time with an odd batch stride (image 0 aligned, images 1 and 2 not) or 4 bytes past a 16-byte boundary: the
    launcher decides per launch, so each of these runs the scalar kernels, whose fp64 sums -- read back from the scratch and from the record
    -- are formed in one fixed order: bit-identical whichever operand it was, and different from the float4 kernels' on aligned operands.
    An operand missing from the host's `vec` condition runs the float4 kernels on misaligned planes: the values stay right, these bits move"""
    H, W = 72, 64
    d, t = case(H, W), dev(H, W)
    C = C0
    mean, invstd = kstats(ops, H, W)
    b = base(ops, H, W)
    # With dy = O(1) the two routes' ordered sums often coincide: a thread adds four nearly exact products, and the later, larger partial sums
    # round both orders alike.  So each channel gets 2^40 and -2^40 at elements j and j + 256 of chunk 0 of image 0, where both gates are
    # open: the scalar kernel's thread j adds them to each other first (exactly 0, its other elements keep all their bits), the float4
    # kernel's thread j / 4 adds 2^40 to its three neighbours first, which lose their bits below 2^-12 before -2^40 arrives from another
    # wave -- sum dz differs between the routes in every channel, by construction and not by luck
    y1 = ops.bn_apply(t['x'], mean, invstd, t['gamma'], t['beta'], True)
    both = ((b['y'] > 0) & (y1 > 0)).cpu().view(N0, C, H * W)
    dyc = d['dy'].clone().view(N0, C, H * W)
    for c in range(C):
        j = next(j for j in range(256) if both[0, c, j] and both[0, c, j + 256])
        dyc[0, c, j], dyc[0, c, j + 256] = 2.0 ** 40, -2.0 ** 40
    dyc = dyc.view(d['shape'])
    dyw = dyc.to(DEV)
    R = bwd_ref(d['x'], dyc, d['gamma'], (b['y'] > 0).cpu())

    def launch(kind, viewed):
        o = Operands(kind, viewed, d['shape'])
        dyv, yv, xv = o.src('dy', dyw), o.src('y', b['y']), o.src('x', t['x'])
        dxv, drv = o.dst('dx'), o.dst('dres')
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.bn_backward(dyv, yv, xv, mean, invstd, t['gamma'], dg, db, True, drv, dx=dxv)
        ws = bn_ws(ops, C)
        o.check(f'deterministic bn_backward, {kind} view of {viewed}')
        return dxv, drv, dg, db, ws

    def sums(kind, viewed):
        o = Operands(kind, viewed, d['shape'])
        rec = ops.bn_backward_sums(o.src('dy', dyw), o.src('x', t['x']), mean, invstd, t['gamma'], t['beta'], None, None)
        o.check('deterministic bn_backward_sums')
        return rec

    roles = ('dy', 'y', 'x', 'dx', 'dres')
    with det_mode(ops):
        first, second = launch('odd', roles), launch('odd', roles)
        for a, c in zip(first, second):
            assert torch.equal(a, c)
        dx, dres, dg, db, ws_scalar = first
        within(dx, R['dx'], R['M_dx'], 'dx', 'deterministic dx on views')
        within(dg, R['s2'], R['M_s2'], 'dgamma')
        within(db, R['s1'], R['M_s1'], 'dbeta')
        assert torch.equal(dres, torch.where(b['y'] > 0, dyw, torch.zeros((), device=DEV)))
        ws_vec = launch('slice', roles)[4]
        assert torch.equal(launch('slice', ())[4], ws_vec)
        assert bool((ws_vec[:, 0] != ws_scalar[:, 0]).all()), 'the two routes sum in the same order: this test cannot tell them apart'
        for kind in ('odd', 'lead'):
            for role in roles:
                assert torch.equal(launch(kind, (role,))[4], ws_scalar), f'bn_backward with a misaligned {role} ({kind}) did not take the scalar route'
        rec_scalar, rec_vec = sums('odd', ('dy', 'x')), sums('slice', ('dy', 'x'))
        assert bool((rec_fields(rec_scalar)['m1'] != rec_fields(rec_vec)['m1']).all())
        for kind in ('odd', 'lead'):
            for role in ('dy', 'x'):
                assert torch.equal(sums(kind, (role,)), rec_scalar), f'bn_backward_sums with a misaligned {role} ({kind}) did not take the scalar route'
    report()


@pytest.mark.parametrize('H,W', [(72, 64), (53, 87)])
def test_f_deterministic_slot_order(ops, H, W):
    """deterministic mode adds the slots of a channel in index order, slot (image, chunk) = n * splits + chunk (bn_stats_kernel,
    bn_bwd_reduce_kernel, the latter under the reversed traversal).  One nonzero value per chunk makes every chunk sum exact; the values
    1, e, e, e, e (e = 2^-53) in image 0 and e, e in image 2 sum to exactly 1.0 in that order in fp64 (every 1 + e is a tie that rounds to
    the even 1) and to more than 1 as soon as two of the e meet before the 1 -- chunks or images walked from the other end"""
    N, C, HW = N0, C0, H * W
    splits, chunk = bn_splits(HW, C, N)
    assert splits == 5
    e = 2.0 ** -53
    v = torch.zeros(N, C, HW)
    for c in range(C):
        for k in range(splits):
            v[0, c, k * chunk + 7 * c + 3] = 1.0 if k == 0 else e
        v[2, c, 11 + c], v[2, c, chunk + 5 * c] = e, e
    vd = v.view(N, C, H, W).to(DEV)
    t = dev(H, W)
    mean, invstd = kstats(ops, H, W)
    with det_mode(ops):
        ops.bn_stats(vd)
        assert bn_ws(ops, C)[:, 0].tolist() == [1.0] * C, 'bn_stats: slots out of order'
        ops.bn_backward(vd, None, t['x'], mean, invstd, t['gamma'], None, None, False)
        assert bn_ws(ops, C)[:, 0].tolist() == [1.0] * C, 'bn_backward: slots out of order'
        rec = ops.bn_backward_sums(vd, t['x'], mean, invstd, t['gamma'], t['beta'] + 100.0, None, None)          # (the gate open everywhere)
        assert rec_fields(rec)['m1'].tolist() == [1.0 / (N * HW)] * C, 'bn_backward_sums: slots out of order'


if __name__ == '__main__':
    print('largest |fp64 from fp32-rounded coefficients - pure fp64| / (2^-24 M):', measure_k())
