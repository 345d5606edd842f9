"""The dense convolution family on VIEWS: the fp32 implicit GEMM (csrc/conv_mfma.hip, conv_igemm_q.hip), the bf16x6 split (conv_split.hip), the
f16x3 split (conv_f16x3.hip), the weight-gradient entries (pfst_conv_wgrad, pfst_conv_wgrad_split, pfst_conv_wgrad_f16x3,
pfst_conv_wgrad_f16x3_q in group C, pfst_wino_wgrad in group E) and the Winograd transforms (conv_winograd.hip).  The model hands these
kernels channel slices of its concat buffers (a pointer and a batch stride per operand); tests/test_hip_ops.py runs them on dense tensors,
but for one aligned fp32 1x1 forward launch.

View kinds, applied to each operand in turn and then to all at once: `slice`, channels [8, 8 + C) of a wider buffer with a batch stride in
whole float4s and a 16-byte aligned first plane (what the model does; once the decoder's own geometry, 48 channels at channel offset 512 of
560); `lead`, Guard(lead=1): planes start 4 bytes behind a 16-byte boundary; `odd`, Guard(odd=1): an odd batch stride.

References: fp64 on the CPU (F.conv2d, torch.nn.grad.conv2d_input / conv2d_weight), seeded generators.  Bounds, INHERITED from
test_hip_ops.py and none raised: fp32 2e-5 (fprop / dgrad / accumulate) and 5e-5 (wgrad); bf16x6 and f16x3 2e-6 and 3e-6 (both f16x3
weight-gradient kernels); Winograd WINO_TOL[m] and twice that for dw; mean / invstd out of bn_finalize_partials 2e-5 of the vector's maximum
(x = randn + 0.3: each case asserts max |mean| > 0.1 first).  Unlike there every bound but the last is applied PER OUTPUT CHANNEL (dw: per
output and per input channel) with helpers.chan_close, so that a wrong tail channel cannot hide behind a larger one.  Condition on the
inputs, asserted per case before the bound is used (conditioned()): every channel's max |ref| is at least 0.25 of the tensor's -- met by
every seed and shape below, checked on the CPU beforehand (the worst: 0.31, the normalise-on-load case, whose gammas / betas were chosen for
it).  No bound needed the CPU-fp32 measurement: the worst channel of any kernel sits at 0.69 of its bound.

Bit-identity: the forward and data-gradient kernels have no atomics and no address-dependent route, so every view kind must give
torch.equal with the same launch on dense copies -- output, statistics partials, min / max partials, BatchNorm-backward partials.  Weight
gradients: in deterministic mode an aligned slice equals the dense launch bitwise (it takes the same K-quad / whole-line route);
misaligned operands are held to the bound, and where the entry has no other kernel (the two f16x3 entries) to a refusal that leaves a
pre-filled, SENT-guarded dw untouched.  For pfst_conv_wgrad the fall-back is visible as well: in deterministic mode the generic kernel's
sums differ bitwise from the K-quad kernel's in every case (asserted); the two bf16x6 kernels agree bitwise in all 36 launches (printed),
so pfst_conv_wgrad_split's route shows in the helper only.  pfst_wino_output refuses a misaligned `pre` of its BatchNorm-backward fold
(PFST_CHECK_ARG, stated in hip_ops.wino_conv): those cases are refusal tests.
The model cannot produce misaligned operands: every slice is whole planes with HW % 4 == 0 of an aligned buffer.  So Conv2dP.wgrad_route
not consulting the alignment for `line_f16x3` is left alone.

Canaries: every output (y, dx, dw with 9 floats either side) lies in a SENT-filled buffer and Guard.intact holds afterwards; the statistics
scratch is filled with SENT and nothing behind the partials a launch owns may change (the BatchNorm-backward partials are a tensor of
exactly their size, allocated by the wrapper: equality with the dense launch is their check); the parent buffers of inputs come back
bit-identical.  Group D puts the inputs into buffers whose every other float is NaN, with 128 NaN channels behind each slice, for the
launches that rely on out-of-range loads returning zeros (f16x3 1x1 with Cin % 32 == 16, forward and as the data gradient's contraction;
the whole-line weight gradient with rows past M = 136 and J = 72; the tile chain walked with pfst_f16x3_set_slots(2)) and once per other
family: NaN-free, within the bound, and ops.absmax of the view itself exact.

Group E adds one case to the issue's list, (2, 16, 32, 8, 12, d1): W % 4 == 0 at dilation 1 is where pfst_wino_input / pfst_wino_output
choose between vector and scalar accesses by the operand's alignment (the only address-dependent choice of the transforms, and the one the
model's layers take); `lead` and `odd` views then run the scalar form and must still equal the dense launch bit for bit.

Routes: conv_route() restates the host's choice from the C sources; every case names the route it is meant to hit and asserts the helper
agrees; test_every_route_is_reached holds the set seen against ROUTES.  fp32: generic (Cin % 16 != 0), quad with 32 / 64 / 128 rows (the
issue's "48 -> 6 with bias" has Cin % 16 == 0: it is the 32-row K-quad tile, and runs as that); bf16x6: pair, pipe, plain 32 / 64 / 128;
f16x3: small, one / not-one, big, chain, nt, bnl, bnb modes 1 / 2 / 3, y_mask, gate; weight gradients: quad / generic of the fp32 and bf16x6
entries, line / refusal of pfst_conv_wgrad_f16x3, refusal and 32 / 64 / 128 rows of pfst_conv_wgrad_f16x3_q.

MEASURED on an MI355X, worst ratio to its bound per group (1.0 would fail), per-channel norm:
  group   fp32      bf16x6    f16x3                                   mean     invstd
  A       0.061     0.61      0.39                                    0.0081   0.0084
  B       0.052     0.69      0.31      (fused BatchNorm-backward sums against the two-pass kernel: 0.021 of 1e-5)
  C       0.016     0.27      0.23 (line) 0.23 (quad)
  D       0.029     0.23      0.16 (fwd) 0.13 (dgrad) 0.15 (line wgrad) 0.13 (quad wgrad)
  E       F(2x2): forward 0.17, dx 0.14, dw 0.070; F(4x4): forward 0.24, dx 0.18, dw 0.064 (worst of plain / bf16x6 / f16x3 filters)   0.036   0.017

Mutations of csrc/ tried against this file on scratch copies (none committed):
  1. `b_rsrc` of conv_igemm_f16x3_body given the range `in_bs * 4` instead of `C * HiWi * 4` -- group D run on the MI355X: the six f16x3
     cases with a half-empty last channel block fail (48 -> 48 and 80 -> 136 forward, N = 1 and with the grid sized for two slots; 48 -> 48
     and 136 -> 80 data gradient) on `a NaN from outside the view reached the result`; the other eleven pass.  Groups A, B, C, E by
     reading: what lies behind their slices is SENT, finite, and meets zero-padded weights -- they cannot see it (and were not run on the
     mutant: its last image reads past the buffers their guards allocate).
  2. `out + n * out_bs` replaced by the dense stride `n * M * P` in conv_igemm_f16x3_body's epilogue -- run on the MI355X: all eight f16x3
     rows of test_a_forward_on_views with N = 2, the bias test, the N = 2 normalise-on-load test, five rows of test_b_dgrad_on_views, the three fused
     BatchNorm-backward tests and the gate test fail (19 tests: values and canaries of every view kind on out); the N = 1 rows and the
     other 85 tests pass.
  3. The pointer test dropped from pfst_wgrad_q_eligible -- by reading: the hardware tolerates 4-byte-aligned 16-byte loads, so values
     stay right.  pfst_conv_wgrad_f16x3_q then launches on a `lead` operand instead of refusing: test_c_wgrad_on_views[wgrad_f16q-*]
     (five cases) fail on pytest.raises, where ops.wgrad_q_operands_ok still says no.  pfst_conv_wgrad then takes the K-quad
     kernel for a `lead` operand: test_c_wgrad_on_views[wgrad-*] fail for the five stride-1 cases on `the route of misaligned operands`
     (the deterministic sums equal the dense launch's where they must differ).  Not caught through pfst_conv_wgrad_split, which does not
     use this function; its own pointer test (pfst_wgrad_split_q_eligible) cannot be caught by values, see above.
"""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import SENT, Guard, chan_close, note, out_view, report
from test_hip_ops import WINO_TOL, g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
BOUND = {'fp32': (2e-5, 5e-5), 'bf16x6': (2e-6, 3e-6), 'f16x3': (2e-6, 3e-6)}        # (fprop / dgrad / accumulate, wgrad): test_hip_ops.py
WG_BOUND = {'wgrad': 5e-5, 'wgrad_split': 3e-6, 'wgrad_f16x3': 3e-6, 'wgrad_f16q': 3e-6}
STAT = 2e-5                                                                            # mean / invstd out of bn_finalize_partials
KINDS = ('slice', 'lead', 'odd')
ROUTES = {'fp32:generic', 'fp32:quad32', 'fp32:quad64', 'fp32:quad128',
          'bf16x6:pair', 'bf16x6:pipe', 'bf16x6:plain32', 'bf16x6:plain64', 'bf16x6:plain128',
          'f16x3:small', 'f16x3:one', 'f16x3:notone', 'f16x3:big', 'f16x3:chain', 'f16x3:nt', 'f16x3:bnl', 'f16x3:bnb1', 'f16x3:bnb2',
          'f16x3:bnb3', 'f16x3:ymask', 'f16x3:gate',
          'wgrad:quad', 'wgrad:generic', 'wgrad_split:quad', 'wgrad_split:generic', 'wgrad_f16x3:line', 'wgrad_f16x3:refuse',
          'wgrad_f16q:refuse', 'wgrad_f16q:bm32', 'wgrad_f16q:bm64', 'wgrad_f16q:bm128'}
SEEN = set()


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------- the host's choice, restated
def tile_rows(m):
    return 128 if m > 64 else 64 if m > 32 else 32


def conv_route(ops, family, mode, n, cin, cout, hw, k, s, d, operands=(), **options):
    """-> the tags of the kernel the host picks for this launch of a cin -> cout layer reading hw = (H, W) with pad = d * (k // 2).
    mode 'fwd' contracts over C = cin into M = cout rows, 'dgrad' over C = cout into M = cin rows, 'wgrad' (families wgrad, wgrad_split,
    wgrad_f16x3, wgrad_f16q) looks at the operands (x, dy) as the entries' alignment gates do"""
    H, W = hw
    if mode == 'wgrad':
        aligned = all(t.data_ptr() % 16 == 0 and ops._bs(t) % 4 == 0 for t in operands)
        # conv_wgrad_q.hip pfst_wgrad_q_eligible (stride 1 'same': input and output planes agree)
        quad = s == 1 and aligned and ((H * W) % 4 == 0 if k == 1 else (W % 16 == 0 and d <= 8))
        if family == 'wgrad':                         # conv_mfma.hip pfst_conv_wgrad
            return ('quad',) if quad else ('generic',)
        if family == 'wgrad_split':                   # conv_split.hip pfst_wgrad_split_q_eligible: 1x1 only
            return ('quad',) if quad and k == 1 else ('generic',)
        if family == 'wgrad_f16x3':                   # conv_f16x3.hip pfst_conv_wgrad_f16x3: PFST_CHECK_ARG on `& 15` / `& 3`
            assert k == 1 and s == 1 and (H * W) % 4 == 0 and cout > 64
            return ('line',) if aligned else ('refuse',)
        assert family == 'wgrad_f16q' and s == 1      # conv_wgrad_q.hip pfst_conv_wgrad_f16x3_q
        return (f'bm{tile_rows(cout)}',) if quad else ('refuse',)
    C, M = (cin, cout) if mode == 'fwd' else (cout, cin)
    bm = tile_rows(M)
    if family == 'fp32':                              # conv_mfma.hip pfst_conv_igemm, conv_igemm_q.hip pfst_igemm_q_launch
        return ('generic',) if C % 16 else (f'quad{bm}',)
    if family == 'bf16x6':                            # conv_split.hip launch_split
        if bm == 128 and C * k * k >= 512:
            return ('pair',) if C % 32 == 0 else ('pipe',)
        return (f'plain{bm}',)
    assert family == 'f16x3'                          # conv_f16x3.hip pfst_conv_igemm_f16x3 and conv_igemm_f16x3_body (KP, CHAIN, nt_out)
    small = M <= 64
    one = not small and k == 1 and s == 1
    kp = cdiv(C, 32) * (1 if one else k * k)
    tags = ['small'] if small else ['one' if one else 'notone']
    if one and M % 256 == 0:
        tags.append('big')
    if one and kp % 2 == 0:
        tags.append('chain')
    if kp <= 16:
        tags.append('nt')
    if options.get('bnl') is not None:
        tags.append('bnl')
    bnb = options.get('bnb')
    if bnb is not None:
        tags.append('bnb3' if not bnb[3] else 'ymask' if len(bnb) > 4 else 'bnb2' if bnb[1] is not None else 'bnb1')
    if options.get('gate') is not None:
        tags.append('gate')
    return tuple(tags)


def hit(family, tags, expect):
    assert tuple(tags) == tuple(expect), (family, tags, expect)
    SEEN.update(f'{family}:{t}' for t in tags)


# ------------------------------------------------------------------------------------------------------------------------------ the checks
def conditioned(ref, cdim=1):
    """the per-channel bound is only used where no channel's max |ref| is below a quarter of the tensor's"""
    m = ref.abs().amax([i for i in range(ref.dim()) if i != cdim])
    assert float(m.min()) >= 0.25 * float(m.max()), (float(m.min()), float(m.max()))


def close(got, ref, bound, group, kind, cdims=(1,)):
    for cdim in cdims:
        conditioned(ref, cdim)
        chan_close(got, ref, bound, group, kind, cdim=cdim)


def vec_close(got, ref, bound, group, kind):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    ratio = float((got - ref).abs().max() / (bound * ref.abs().max()))
    note(group, kind, ratio)
    assert ratio < 1.0, f'{kind}: {ratio:.3g} x the bound {bound}'


def bits(t):
    return t.view(torch.int32)


@contextlib.contextmanager
def det_mode(ops, on=True):
    before = ops.is_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(before)


def guard(shape, kind, fill=SENT, front=8, back=4):
    """the three kinds of view of the file (module docstring); slice: `front` channels in front, at least `back` behind"""
    n, c, h, w = shape
    if kind == 'slice':
        while ((front + c + back) * h * w) % 4:
            back += 1
        gd = Guard(shape, front=front, back=back, fill=fill)
        assert gd.view.data_ptr() % 16 == 0 and gd.bs % 4 == 0
    elif kind == 'lead':
        gd = Guard(shape, front=1 if (1 + h * w) % 4 else 2, lead=1, fill=fill)        # (an odd plane: 1 + HW may be a whole float4)
        assert gd.view.data_ptr() % 16 != 0
    else:
        assert kind == 'odd'
        gd = Guard(shape, odd=1, fill=fill)
        assert gd.bs % 4 != 0
    return gd


def in_view(t, kind, fill=SENT, **kw):
    """an input inside a canary buffer, with a snapshot of the whole buffer"""
    gd = guard(tuple(t.shape), kind, fill, **kw)
    gd.put(t)
    gd.snap = gd.flat.clone()
    return gd


def unchanged(gd, what=''):
    assert torch.equal(bits(gd.flat), bits(gd.snap)), f'{what}: the parent buffer of an input changed'


class DwBuf:
    """a weight gradient with 9 SENT floats either side, zeroed or pre-filled"""

    def __init__(self, shape, init=None):
        numel = 1
        for s in shape:
            numel *= s
        self.buf = torch.full((numel + 18,), SENT, device=DEV)
        self.dw = self.buf[9:9 + numel].view(shape)
        if init is None:
            self.dw.zero_()
        else:
            self.dw.copy_(init)
        self.snap = self.buf.clone()

    def intact(self, what=''):
        assert bool((self.buf[:9] == SENT).all()) and bool((self.buf[-9:] == SENT).all()), f'{what}: floats beside dw were written'

    def untouched(self, what=''):
        assert torch.equal(bits(self.buf), bits(self.snap)), f'{what}: a refused launch wrote dw'


def sent_stats(ops):
    """the statistics scratch of the next launch, filled with SENT"""
    return ops._scratch(torch.device(DEV, torch.cuda.current_device()), 'stats', 1, ops._STATS_FLOOR).fill_(SENT)


def owned(st, used):
    """the region of the SENT-filled scratch a launch owns; nothing behind it may be written"""
    assert bool((st[used:] == SENT).all()), 'the stats scratch was written behind its partials'
    assert not bool((st[:used] == SENT).any())
    return st[:used].clone()


def check_stats(ops, part, slots, co, y, y_ref, group, minmax):
    """bn_finalize_partials of the (sum, sum of squares) partials against the fp64 reference's mean / biased variance; the extrema exactly"""
    mean, invstd = ops.bn_finalize_partials(part, slots, co, y_ref.numel() // co)
    mean_ref = y_ref.mean((0, 2, 3))
    assert float(mean_ref.abs().max()) > 0.1          # the bound is relative to this
    vec_close(mean, mean_ref, STAT, group, 'mean')
    vec_close(invstd, 1.0 / torch.sqrt(y_ref.var((0, 2, 3), unbiased=False) + 1e-5), STAT, group, 'invstd')
    if minmax:
        mm = part[2 * co * slots:4 * co * slots].view(co, slots, 2)
        assert torch.equal(mm[:, :, 0].min(dim=1)[0], y.amin(dim=(0, 2, 3))) and torch.equal(mm[:, :, 1].max(dim=1)[0], y.amax(dim=(0, 2, 3)))


# ---------------------------------------------------------------------------------------------------------------- inputs and fp64 references
def pad_of(k, d):
    return d * (k // 2)


@functools.lru_cache(maxsize=None)
def conv_case(n, ci, co, H, W, k, s, d, bias=False):
    """CPU inputs and the fp64 forward reference of one layer, computed once and never modified (x carries an offset so that the channel
    means the statistics are held to are not sums that cancel)"""
    x = torch.randn(n, ci, H, W, generator=g(1)) + 0.3
    w = torch.randn(co, ci, k, k, generator=g(2)) * 0.1
    b = torch.randn(co, generator=g(3)) if bias else None
    y = F.conv2d(x.double(), w.double(), None if b is None else b.double(), s, pad_of(k, d), d)
    dy = torch.randn(y.shape, generator=g(4))
    return dict(x=x, w=w, b=b, y=y, dy=dy)


@functools.lru_cache(maxsize=None)
def ref_dx(*case):
    c = conv_case(*case)
    k, s, d = case[5:8]
    return torch.nn.grad.conv2d_input(c['x'].shape, c['w'].double(), c['dy'].double(), s, pad_of(k, d), d)


@functools.lru_cache(maxsize=None)
def ref_dw(*case):
    c = conv_case(*case)
    k, s, d = case[5:8]
    return torch.nn.grad.conv2d_weight(c['x'].double(), c['w'].shape, c['dy'].double(), s, pad_of(k, d), d)


@functools.lru_cache(maxsize=None)
def packed(ops, fam, case):
    """-> (forward image, data-gradient image or None, weight amax or None) of the case's filter, on the device"""
    n, ci, co = case[:3]
    k = case[5]
    wd = conv_case(*case)['w'].to(DEV)
    if fam == 'fp32':
        return ops.pack_weight(wd) + (None,)
    if fam == 'bf16x6':
        return ops.pack_weight_split(wd, ci % 16 == 0, co % 16 == 0) + (None,)
    return ops.pack_weight_f16x2(wd, ops.f16x3_eligible(ci, co, k), ops.f16x3_eligible(co, ci, k))


def fprop(ops, fam, case, x, out=None, x_amax=None, **opt):
    n, ci, co, H, W, k, s, d = case[:8]
    wf, _, wa = packed(ops, fam, case)
    if fam == 'fp32':
        return ops.conv_fprop(x, wf, co, k, s, d, pad_of(k, d), out=out, **opt)
    if fam == 'bf16x6':
        return ops.conv_fprop_split(x, wf, co, k, s, d, pad_of(k, d), out=out, **opt)
    return ops.conv_fprop_f16x3(x, wf, wa, ops.absmax(x) if x_amax is None else x_amax, co, k, s, d, pad_of(k, d), out=out, **opt)


def dgrad(ops, fam, case, dy, out=None, accumulate=False, **opt):
    n, ci, co, H, W, k, s, d = case[:8]
    _, wd, wa = packed(ops, fam, case)
    if fam == 'fp32':
        return ops.conv_dgrad(dy, wd, ci, (H, W), k, s, d, pad_of(k, d), out=out, accumulate=accumulate, **opt)
    if fam == 'bf16x6':
        return ops.conv_dgrad_split(dy, wd, ci, (H, W), k, s, d, pad_of(k, d), out=out, accumulate=accumulate, **opt)
    return ops.conv_dgrad_f16x3(dy, wd, wa, ops.absmax(dy), ci, (H, W), k, s, d, pad_of(k, d), out=out, accumulate=accumulate, **opt)


def combos(names):
    """each operand viewed in turn, then all at once"""
    return [(nm,) for nm in names] + [tuple(names)]


# ======================================================================================================================= A: forward on views
# layer cases (n, cin, cout, H, W, k, stride, dil[, bias]) and the route each family takes for them
C48 = (2, 48, 48, 9, 14, 1, 1, 1)            # the f16x3 64-row tile and a single, half-empty channel block
C80 = (2, 80, 136, 9, 14, 1, 1, 1)           # three steps, the last one half empty; ragged 128-row tile
C80N1 = (1, 80, 136, 9, 14, 1, 1, 1)
C64 = (2, 64, 136, 10, 13, 1, 1, 1)          # two steps: the tile chain; two pixel tiles, the last with two pixels
C256 = (2, 64, 256, 9, 14, 1, 1, 1)          # the 256-row tile
C544 = (2, 544, 136, 9, 14, 1, 1, 1)         # 17 steps: no streaming stores; bf16x6 K = 32 pairing
C528 = (2, 528, 136, 9, 14, 1, 1, 1)         # bf16x6 K = 16 pipelined loop
D2 = (2, 64, 72, 9, 14, 3, 1, 2)
S2 = (2, 64, 72, 17, 19, 3, 2, 1)
G10 = (2, 10, 32, 17, 19, 3, 2, 1)           # Cin % 16 != 0: the generic fp32 kernel
B6 = (2, 48, 6, 9, 14, 1, 1, 1, True)        # conv_seg-like: bias, the 32-row tile (Cin % 16 == 0: the K-quad kernel, not the generic one)
A_ROWS = [
    ('fp32', C48, ('quad64',)), ('fp32', C80, ('quad128',)), ('fp32', C80N1, ('quad128',)), ('fp32', C64, ('quad128',)),
    ('fp32', C256, ('quad128',)), ('fp32', C544, ('quad128',)), ('fp32', C528, ('quad128',)), ('fp32', D2, ('quad128',)),
    ('fp32', S2, ('quad128',)), ('fp32', G10, ('generic',)), ('fp32', B6, ('quad32',)),
    ('bf16x6', C48, ('plain64',)), ('bf16x6', C80, ('plain128',)), ('bf16x6', C80N1, ('plain128',)), ('bf16x6', C64, ('plain128',)),
    ('bf16x6', C256, ('plain128',)), ('bf16x6', C544, ('pair',)), ('bf16x6', C528, ('pipe',)), ('bf16x6', D2, ('pair',)),
    ('bf16x6', S2, ('pair',)), ('bf16x6', B6, ('plain32',)),
    ('f16x3', C48, ('small', 'nt')), ('f16x3', C80, ('one', 'nt')), ('f16x3', C80N1, ('one', 'nt')), ('f16x3', C64, ('one', 'chain', 'nt')),
    ('f16x3', C256, ('one', 'big', 'chain', 'nt')), ('f16x3', C544, ('one',)), ('f16x3', C528, ('one',)), ('f16x3', D2, ('notone',)),
    ('f16x3', S2, ('notone',)),
]


def row_id(v):
    return 'x'.join(str(int(i)) for i in v) if isinstance(v, tuple) and v and isinstance(v[0], int) else None


@pytest.mark.parametrize('fam,case,route', A_ROWS, ids=row_id)
def test_a_forward_on_views(ops, fam, case, route):
    """output, fused statistics (f16x3: and the min / max partials) of every view kind on x, on out and on both: those of the dense launch"""
    n, ci, co, H, W, k, s, d = case[:8]
    cd = conv_case(*case)
    xd = cd['x'].to(DEV)
    hit(fam, conv_route(ops, fam, 'fwd', n, ci, co, (H, W), k, s, d), route)
    bias = None if cd['b'] is None else cd['b'].to(DEV)
    stats, minmax = bias is None, fam == 'f16x3' and bias is None
    shape = tuple(cd['y'].shape)

    def launch(x, out):
        if not stats:
            return fprop(ops, fam, case, x, out=out, bias=bias), None, 0
        opt = dict(want_stats=True, want_minmax=True) if minmax else dict(want_stats=True)
        st0 = sent_stats(ops)
        y, st, sl = fprop(ops, fam, case, x, out=out, **opt)
        assert st.data_ptr() == st0.data_ptr()
        return y, owned(st, (4 if minmax else 2) * co * sl), sl

    y0, p0, sl = launch(xd, None)
    close(y0, cd['y'], BOUND[fam][0], 'conv-A', f'{fam} forward')
    if stats:
        check_stats(ops, p0, sl, co, y0, cd['y'], 'conv-A', minmax)
    views = [(kind, which) for kind in KINDS for which in combos(('x', 'out'))]
    for kind, which in views:
        xg = in_view(xd, kind) if 'x' in which else None
        og = guard(shape, kind) if 'out' in which else None
        y, p, sl1 = launch(xg.view if xg else xd, og.view if og else None)
        assert sl1 == sl and torch.equal(y, y0), (kind, which, 'output')
        assert p0 is None or torch.equal(bits(p), bits(p0)), (kind, which, 'partials')
        if xg:
            unchanged(xg, f'{kind} x')
        if og:
            og.intact(f'{kind} out')
    if co == 48:
        # the decoder's c1_bottleneck: 48 channels at channel offset 512 of the 560-channel concat buffer
        og, out = out_view(shape, front=512, back=0)
        y, p, _ = launch(xd, out)
        assert torch.equal(y, y0) and torch.equal(bits(p), bits(p0))
        og.intact('channels [512, 560) of 560')
    report('conv-A')


def test_a_f16x3_bias_with_an_output_view(ops):
    case = C48 + (True,)
    cd = conv_case(*case)
    xd, bias = cd['x'].to(DEV), cd['b'].to(DEV)
    y0 = fprop(ops, 'f16x3', case, xd, bias=bias)
    close(y0, cd['y'], BOUND['f16x3'][0], 'conv-A', 'f16x3 forward')
    for kind in KINDS:
        og = guard(tuple(cd['y'].shape), kind)
        assert torch.equal(fprop(ops, 'f16x3', case, xd, out=og.view, bias=bias), y0)
        og.intact(kind)


@pytest.mark.parametrize('n', [2, 1])
def test_a_f16x3_normalise_on_load_reads_a_view(ops, n):
    """bnl: x is the viewed PRE-normalisation tensor; against bn_apply followed by the plain launch, bit for bit"""
    case = (n,) + C256[1:]
    _, ci, co, H, W, k, s, d = case
    pre = (torch.randn(n, ci, H, W, generator=g(11)) * 1.5).to(DEV)
    # gammas of both signs and one zero; the post-ReLU means are kept small against the spread, so that no output channel is dominated
    # by (channel means) x (its filter's sum) and the per-channel condition holds (min / max of the channels' max |ref|: 0.38 and 0.31)
    gamma = ((torch.rand(ci, generator=g(12)) * 0.6 + 0.5) * torch.where(torch.arange(ci) % 5 == 0, -1.0, 1.0)).to(DEV)
    gamma[0] = 0.0
    beta = (torch.randn(ci, generator=g(13)) * 0.3 - 0.3).to(DEV)
    mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
    ya = ops.amax_slots(pre.device)
    ymat = ops.bn_apply(pre, mean, invstd, gamma, beta, True, amax=ya)
    hit('f16x3', conv_route(ops, 'f16x3', 'fwd', n, ci, co, (H, W), k, s, d, bnl=coef), ('one', 'big', 'chain', 'nt', 'bnl'))
    opt = dict(want_stats=True, want_minmax=True)
    sent_stats(ops)
    y0, st, sl = fprop(ops, 'f16x3', case, ymat, x_amax=ya, **opt)
    p0 = owned(st, 4 * co * sl)
    y_ref = F.conv2d(ymat.double().cpu(), conv_case(*case)['w'].double())
    close(y0, y_ref, BOUND['f16x3'][0], 'conv-A', 'f16x3 forward')
    for kind in KINDS:
        for which in combos(('x', 'out')):
            pg = in_view(pre, kind) if 'x' in which else None
            og = guard(tuple(y0.shape), kind) if 'out' in which else None
            sent_stats(ops)
            y, st, sl1 = fprop(ops, 'f16x3', case, pg.view if pg else pre, out=og.view if og else None, x_amax=ya, bnl=coef, **opt)
            assert sl1 == sl and torch.equal(y, y0) and torch.equal(bits(owned(st, 4 * co * sl)), bits(p0)), (kind, which)
            if pg:
                unchanged(pg, kind)
            if og:
                og.intact(kind)
    report('conv-A')


# ================================================================================================================= B: data gradient on views
L48 = C48
L80 = (2, 136, 80, 9, 14, 1, 1, 1)           # the data gradient contracts over the 80 output channels: a last half block
L64 = (2, 136, 64, 10, 13, 1, 1, 1)
L256 = (2, 256, 64, 9, 14, 1, 1, 1)
LD2 = (1, 72, 64, 10, 13, 3, 1, 2)
LS2 = (2, 72, 64, 17, 19, 3, 2, 1)
B_ROWS = [
    ('fp32', L48, ('quad64',)), ('fp32', L80, ('quad128',)), ('fp32', LD2, ('quad128',)), ('fp32', LS2, ('quad128',)),
    ('bf16x6', L48, ('plain64',)), ('bf16x6', L80, ('plain128',)), ('bf16x6', LD2, ('pair',)), ('bf16x6', LS2, ('pair',)),
    ('f16x3', L48, ('small', 'nt')), ('f16x3', L80, ('one', 'nt')), ('f16x3', L64, ('one', 'chain', 'nt')),
    ('f16x3', L256, ('one', 'big', 'chain', 'nt')), ('f16x3', LD2, ('notone',)), ('f16x3', LS2, ('notone',)),
]


@pytest.mark.parametrize('fam,case,route', B_ROWS, ids=row_id)
def test_b_dgrad_on_views(ops, fam, case, route):
    """dx of every view kind on dy, on out, on out with accumulation into a pre-filled view, and on both: that of the dense launch"""
    n, ci, co, H, W, k, s, d = case
    cd = conv_case(*case)
    xd, dyd = cd['x'].to(DEV), cd['dy'].to(DEV)
    hit(fam, conv_route(ops, fam, 'dgrad', n, ci, co, (H, W), k, s, d), route)
    dx0 = dgrad(ops, fam, case, dyd)
    close(dx0, ref_dx(*case), BOUND[fam][0], 'conv-B', f'{fam} dx')
    acc0 = dgrad(ops, fam, case, dyd, out=xd.clone(), accumulate=True)
    close(acc0, ref_dx(*case) + cd['x'].double(), BOUND[fam][0], 'conv-B', f'{fam} dx accumulate')
    for kind in KINDS:
        for which in combos(('dy', 'out')):
            dg = in_view(dyd, kind) if 'dy' in which else None
            og = guard(tuple(xd.shape), kind) if 'out' in which else None
            dx = dgrad(ops, fam, case, dg.view if dg else dyd, out=og.view if og else None)
            assert torch.equal(dx, dx0), (kind, which)
            if og:
                og.intact(f'{kind} out')
                acc = dgrad(ops, fam, case, dg.view if dg else dyd, out=og.put(xd), accumulate=True)
                assert torch.equal(acc, acc0), (kind, which, 'accumulate')
                og.intact(f'{kind} out, accumulate')
            if dg:
                unchanged(dg, f'{kind} dy')
    report('conv-B')


LBNB = (2, 128, 64, 9, 14, 1, 1, 1)          # the BatchNorm layer's 128 channels are the launch's rows; whole 128-row tiles
BNB_ROUTE = {'fp32': ('quad128',), 'bf16x6': ('plain128',), 'f16x3': ('one', 'chain', 'nt')}


@pytest.mark.parametrize('mode', ['bnb2', 'bnb1', 'bnb3'])
@pytest.mark.parametrize('fam', ['fp32', 'bf16x6', 'f16x3'])
def test_b_fused_bn_backward_sums_on_views(ops, fam, mode):
    """pfst_bnb_fuse_t carries a batch stride for pre and for y, the launch one for out: each viewed in turn, then all; gradient and
    partials are those of the dense launch, and bn_backward from the partials is bn_backward with its own reduction pass"""
    case = LBNB
    n, c, co, H, W, k, s, d = case
    cd = conv_case(*case)
    dyd = cd['dy'].to(DEV)
    relu = mode != 'bnb3'
    pre = (torch.randn(n, c, H, W, generator=g(21)) * 1.7 + 0.8).to(DEV)
    gamma = (0.6 + 0.8 * torch.rand(c, generator=g(22))).to(DEV)
    beta = (0.3 * torch.randn(c, generator=g(23))).to(DEV)
    res = torch.randn(n, c, H, W, generator=g(24)).to(DEV) if mode == 'bnb2' else None
    mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
    y = ops.bn_apply(pre, mean, invstd, gamma, beta, relu, res) if mode == 'bnb2' else None
    bnb = (pre, y, coef, relu)
    tags = conv_route(ops, fam, 'dgrad', n, c, co, (H, W), k, s, d, bnb=bnb)
    hit(fam, tags, BNB_ROUTE[fam] + ((mode,) if fam == 'f16x3' else ()))
    plain = dgrad(ops, fam, case, dyd)
    dx0, part0, sl = dgrad(ops, fam, case, dyd, bnb=bnb)
    assert torch.equal(dx0, plain), 'the data gradient itself must not depend on the fusion'
    close(dx0, ref_dx(*case), BOUND[fam][0], 'conv-B', f'{fam} dx')
    outs = []
    for p, sl_ in ((None, 0), (part0, sl)):
        dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
        outs.append((ops.bn_backward(dx0, y, pre, mean, invstd, gamma, dg, db, relu, beta=beta, partials=p, slots=sl_), dg, db))
    for a, b, what in zip(outs[1], outs[0], ('dL/dpre', 'dgamma', 'dbeta')):
        vec_close(a, b, 1e-5, 'conv-B', f'bnb {what} against the two-pass kernel')        # test_bn_backward_fused_gpu.py's bound
    names = ('pre', 'y', 'out') if y is not None else ('pre', 'out')
    for kind in KINDS:
        for which in combos(names):
            pg = in_view(pre, kind) if 'pre' in which else None
            yg = in_view(y, kind) if 'y' in which else None
            og = guard(tuple(pre.shape), kind) if 'out' in which else None
            dx, part, sl1 = dgrad(ops, fam, case, dyd, out=og.view if og else None, bnb=(pg.view if pg else pre, yg.view if yg else y, coef, relu))
            assert sl1 == sl and torch.equal(dx, dx0) and torch.equal(bits(part), bits(part0)), (kind, which)
            for gd in (pg, yg):
                if gd:
                    unchanged(gd, f'{kind} {which}')
            if og:
                og.intact(f'{kind} {which}')
    report('conv-B')


def test_b_f16x3_gate_reads_a_view(ops):
    """out = data gradient + (mask bit ? g : 0) with g viewed (the mask stays dense); once with the BatchNorm-backward sums in the y_mask form"""
    case = (2, 128, 64, 16, 16, 1, 1, 1)
    n, ci, co, H, W, k, s, d = case
    cd = conv_case(*case)
    dyd = cd['dy'].to(DEV)
    gsrc = torch.randn(n, ci, H, W, generator=g(31))
    pre = torch.randn(n, ci, H, W, generator=g(32)).to(DEV)
    one, zero = torch.ones(ci, device=DEV), torch.zeros(ci, device=DEV)
    mean, invstd, _ = ops.bn_stats(pre, gamma=one, beta=zero)
    yb, mask = ops.bn_apply(pre, mean, invstd, one, zero, True, residual=torch.zeros_like(pre), want_mask=True)
    assert mask is not None and ops.dgrad_gate_ok(ci, (H, W))
    gdev = gsrc.to(DEV)
    hit('f16x3', conv_route(ops, 'f16x3', 'dgrad', n, ci, co, (H, W), k, s, d, gate=(gdev, mask)), ('one', 'chain', 'nt', 'gate'))
    dx = dgrad(ops, 'f16x3', case, dyd)
    dxg0 = dgrad(ops, 'f16x3', case, dyd, gate=(gdev, mask))
    assert torch.equal(dxg0, dx + ops.relu_gate_(torch.empty_like(gdev), gdev, mask))
    ref = ref_dx(*case) + torch.where(yb.cpu() > 0, gsrc, torch.zeros_like(gsrc)).double()
    close(dxg0, ref, BOUND['f16x3'][0], 'conv-B', 'f16x3 dx')
    # the y_mask form: a residual layer's gate bits instead of its y, the sums of the gated total
    pre2 = torch.randn(n, ci, H, W, generator=g(33)).to(DEV)
    m2, i2, coef2 = ops.bn_stats(pre2, gamma=one, beta=zero)
    y2, mask2 = ops.bn_apply(pre2, m2, i2, one, zero, True, residual=torch.randn(n, ci, H, W, generator=g(34)).to(DEV), want_mask=True)
    bnb = (pre2, y2, coef2, True, mask2)
    hit('f16x3', conv_route(ops, 'f16x3', 'dgrad', n, ci, co, (H, W), k, s, d, gate=(gdev, mask), bnb=bnb), ('one', 'chain', 'nt', 'ymask', 'gate'))
    out_m, part_m, _ = dgrad(ops, 'f16x3', case, dyd, bnb=bnb, gate=(gdev, mask))
    out_y, part_y, _ = dgrad(ops, 'f16x3', case, dyd, bnb=bnb[:4], gate=(gdev, mask))
    assert torch.equal(out_m, dxg0) and torch.equal(out_y, dxg0) and torch.equal(bits(part_m), bits(part_y))
    for kind in KINDS:
        gg = in_view(gdev, kind)
        og = guard(tuple(gdev.shape), kind)
        assert torch.equal(dgrad(ops, 'f16x3', case, dyd, gate=(gg.view, mask)), dxg0), kind
        assert torch.equal(dgrad(ops, 'f16x3', case, dyd, out=og.view, gate=(gg.view, mask)), dxg0), kind
        og.intact(kind)
        pg, yg = in_view(pre2, kind), in_view(y2, kind)
        out, part, _ = dgrad(ops, 'f16x3', case, dyd, bnb=(pg.view, yg.view, coef2, True, mask2), gate=(gg.view, mask))
        assert torch.equal(out, dxg0) and torch.equal(bits(part), bits(part_m)), kind
        for gd in (gg, pg, yg):
            unchanged(gd, kind)
    report('conv-B')


# ================================================================================================================ C: weight gradients on views
W24 = (2, 48, 24, 12, 20, 1, 1, 1)
W136 = (2, 64, 136, 12, 20, 1, 1, 1)
W200 = (1, 72, 200, 12, 20, 1, 1, 1)
W3D1 = (2, 16, 40, 9, 16, 3, 1, 1)
W3D2 = (2, 16, 40, 9, 16, 3, 1, 2)
W3S2 = (2, 32, 32, 17, 19, 3, 2, 1)          # stride 2: the generic kernels whatever the operands
C_ROWS = ([('wgrad', c) for c in (W24, W136, W200, W3D1, W3D2, W3S2)] + [('wgrad_split', c) for c in (W24, W136, W200, W3D1, W3D2, W3S2)]
          + [('wgrad_f16x3', c) for c in (W136, W200)] + [('wgrad_f16q', c) for c in (W24, W136, W200, W3D1, W3D2)])


def wgrad_call(ops, entry, dw, x, dy, case, amax=None):
    k, s, d = case[5:8]
    if entry == 'wgrad':
        return ops.conv_wgrad_(dw, x, dy, k, s, d, pad_of(k, d))
    if entry == 'wgrad_split':
        return ops.conv_wgrad_split_(dw, x, dy, k, s, d, pad_of(k, d))
    xa, da = amax if amax is not None else (ops.absmax(x), ops.absmax(dy))
    if entry == 'wgrad_f16x3':
        return ops.conv_wgrad_f16x3_(dw, x, dy, xa, da)
    return ops.conv_wgrad_f16q_(dw, x, dy, xa, da, k, d)


def aligned_route(entry, case):
    """the route of dense (or aligned-slice) operands"""
    n, ci, co, H, W, k, s, d = case
    quad = s == 1 and (k == 1 or entry != 'wgrad_split')
    if entry == 'wgrad_f16x3':
        return ('line',)
    if entry == 'wgrad_f16q':
        return (f'bm{tile_rows(co)}',)
    return ('quad',) if quad else ('generic',)


@pytest.mark.parametrize('entry,case', C_ROWS, ids=row_id)
def test_c_wgrad_on_views(ops, entry, case):
    """aligned slices: the dense launch bit for bit (deterministic mode); misaligned planes or batch strides: the generic kernel within the
    bound (pfst_conv_wgrad, pfst_conv_wgrad_split) or a refusal that leaves dw alone (the f16x3 entries); accumulation into a non-zero dw"""
    from pfst_amd._lib import PfstHipError
    n, ci, co, H, W, k, s, d = case
    cd = conv_case(*case)
    xd, dyd = cd['x'].to(DEV), cd['dy'].to(DEV)
    ref, bound, kind_name = ref_dw(*case), WG_BOUND[entry], f'{entry} dw'
    w0 = torch.randn(ref.shape, generator=g(41)).to(DEV)
    route = lambda x, dy: conv_route(ops, entry, 'wgrad', n, ci, co, (H, W), k, s, d, (x, dy))      # noqa: E731
    hit(entry, route(xd, dyd), aligned_route(entry, case))
    assert ops.wgrad_q_operands_ok(xd, dyd)
    with det_mode(ops):
        b0 = DwBuf(ref.shape)
        wgrad_call(ops, entry, b0.dw, xd, dyd, case)
        b0.intact('dense')
        close(b0.dw, ref, bound, 'conv-C', kind_name, cdims=(0, 1))
        for which in combos(('x', 'dy')):
            xg = in_view(xd, 'slice') if 'x' in which else None
            dg = in_view(dyd, 'slice') if 'dy' in which else None
            xv, dv = xg.view if xg else xd, dg.view if dg else dyd
            assert ops.wgrad_q_operands_ok(xv, dv)
            hit(entry, route(xv, dv), aligned_route(entry, case))
            b = DwBuf(ref.shape)
            wgrad_call(ops, entry, b.dw, xv, dv, case)
            assert torch.equal(b.dw, b0.dw), f'an aligned slice of {which} left the dense launch\'s route'
            b.intact(f'slice {which}')
            for gd in (xg, dg):
                if gd:
                    unchanged(gd, f'slice {which}')
    b = DwBuf(ref.shape, init=w0)
    wgrad_call(ops, entry, b.dw, xd, dyd, case)
    close(b.dw, ref + w0.double().cpu(), bound, 'conv-C', kind_name, cdims=(0, 1))
    b.intact('accumulate')
    for kind in ('lead', 'odd'):
        for which in combos(('x', 'dy')):
            xg = in_view(xd, kind) if 'x' in which else None
            dg = in_view(dyd, kind) if 'dy' in which else None
            xv, dv = xg.view if xg else xd, dg.view if dg else dyd
            assert not ops.wgrad_q_operands_ok(xv, dv)
            b = DwBuf(ref.shape, init=w0)
            if entry in ('wgrad', 'wgrad_split'):
                hit(entry, route(xv, dv), ('generic',))
                wgrad_call(ops, entry, b.dw, xv, dv, case)
                close(b.dw, ref + w0.double().cpu(), bound, 'conv-C', kind_name, cdims=(0, 1))
                b.intact(f'{kind} {which}')
                # the fall-back made visible: in deterministic mode the generic kernel's sums differ bitwise from the K-quad kernel's
                # (and are the dense launch's where that one is generic itself)
                with det_mode(ops):
                    bz = DwBuf(ref.shape)
                    wgrad_call(ops, entry, bz.dw, xv, dv, case)
                same = torch.equal(bz.dw, b0.dw)
                if entry == 'wgrad':
                    assert same == (aligned_route(entry, case) == ('generic',)), (kind, which, 'the route of misaligned operands')
                else:           # the bf16x6 kernels add the same products in the same order on either route: nothing to tell them apart by
                    print(f'{entry} {kind} {which}: bitwise equal to the dense launch: {same}')
            else:
                hit(entry, route(xv, dv), ('refuse',))
                amax = (ops.absmax(xv), ops.absmax(dv))
                with pytest.raises(PfstHipError):
                    wgrad_call(ops, entry, b.dw, xv, dv, case, amax)
                b.untouched(f'{kind} {which}')
            for gd in (xg, dg):
                if gd:
                    unchanged(gd, f'{kind} {which}')
    report('conv-C')


# ================================================================================================================== D: poisoned neighbours
# inputs are slices of buffers whose every other float is NaN: a load that should have returned an out-of-range zero, or one masked by a
# predicate, that instead reads the neighbouring slice multiplies a NaN into the result
WLINE = (2, 72, 136, 12, 20, 1, 1, 1)        # rows past M = 136 and past J = 72 inside the last 128-row tile
D_ROWS = [('fwd', 'f16x3', C48, 0), ('fwd', 'f16x3', C80, 0), ('fwd', 'f16x3', C80N1, 0), ('dgrad', 'f16x3', L48, 0), ('dgrad', 'f16x3', L80, 0),
          ('fwd', 'f16x3', C64, 2), ('dgrad', 'f16x3', L64, 2), ('fwd', 'f16x3', C256, 2), ('fwd', 'f16x3', C80, 2),
          ('fwd', 'fp32', C80, 0), ('fwd', 'bf16x6', C80, 0), ('dgrad', 'fp32', L80, 0), ('dgrad', 'bf16x6', L80, 0),
          ('wgrad_f16x3', 'f16x3', WLINE, 0), ('wgrad_f16q', 'f16x3', W24, 0), ('wgrad', 'fp32', WLINE, 0), ('wgrad_split', 'bf16x6', WLINE, 0)]


@pytest.mark.parametrize('mode,fam,case,slots', D_ROWS, ids=row_id)
def test_d_poisoned_neighbours(ops, mode, fam, case, slots):
    """slots > 0: the grid is sized for that many workgroups (pfst_f16x3_set_slots), so that the tile chain is walked: its load-ahead into
    the next tile (of the next image, too) and the loads past the last pair of the final tile"""
    cd = conv_case(*case)
    xd, dyd = cd['x'].to(DEV), cd['dy'].to(DEV)
    # 128 NaN channels behind every slice: whatever a 32-channel block or a 128-row tile reaches past the view is still inside the buffer
    xg, dg = in_view(xd, 'slice', fill=NAN, back=128), in_view(dyd, 'slice', fill=NAN, back=128)
    assert bool(torch.isnan(xg.flat).any()) and not bool(torch.isnan(xg.view).any())
    for gd, t in ((xg, cd['x']), (dg, cd['dy'])):
        assert float(ops.absmax(gd.view).max()) == float(t.abs().max()), 'absmax of a view read outside it'
    try:
        ops.set_f16x3_slots(slots)
        if mode == 'fwd':
            got, ref, bound, cdims = fprop(ops, fam, case, xg.view), cd['y'], BOUND[fam][0], (1,)
        elif mode == 'dgrad':
            got, ref, bound, cdims = dgrad(ops, fam, case, dg.view), ref_dx(*case), BOUND[fam][0], (1,)
        else:
            got = torch.zeros(cd['w'].shape, device=DEV)
            wgrad_call(ops, mode, got, xg.view, dg.view, case)
            ref, bound, cdims = ref_dw(*case), WG_BOUND[mode], (0, 1)
    finally:
        ops.set_f16x3_slots(0)
    assert not bool(torch.isnan(got).any()), 'a NaN from outside the view reached the result'
    close(got, ref, bound, 'conv-D', f'{mode} {fam}', cdims=cdims)
    unchanged(xg)
    unchanged(dg)
    report('conv-D')


# ========================================================================================================== E: Winograd transforms on views
WN1 = (2, 16, 32, 9, 13, 1)                  # ragged tiles
WN2 = (1, 32, 16, 10, 14, 2)                 # sub-grids of different sizes
WN16 = (2, 96, 96, 9, 13, 1)
WNV = (2, 16, 32, 8, 12, 1)                  # W % 4 == 0 at dilation 1: aligned operands take the transforms' vector loads / stores, `lead` and `odd` the scalar ones
E_ROWS = [(f, c) for c in (WN1, WN2) for f in ('plain', 'bf16x6')] + [('f16x3', WN16), ('plain', WNV)]


@functools.lru_cache(maxsize=None)
def wino_case(n, ci, co, H, W, d):
    x = torch.randn(n, ci, H, W, generator=g(1)) + 0.3
    w = torch.randn(co, ci, 3, 3, generator=g(2)) * 0.1
    dy = torch.randn(n, co, H, W, generator=g(4))
    r = dict(x=x, w=w, dy=dy, y=F.conv2d(x.double(), w.double(), None, 1, d, d))
    r['dx'] = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), 1, d, d)
    r['dw'] = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), 1, d, d)
    r['pre'] = torch.randn(n, ci, H, W, generator=g(51)) * 1.5
    r['gamma'] = (torch.rand(ci, generator=g(52)) + 0.5) * torch.where(torch.arange(ci) % 5 == 0, -1.0, 1.0)
    r['beta'] = torch.randn(ci, generator=g(53)) * 0.5 + 0.3
    return r


@pytest.mark.parametrize('m', [2, 4])
@pytest.mark.parametrize('filt,case', E_ROWS, ids=row_id)
def test_e_winograd_on_views(ops, filt, case, m):
    """pfst_wino_input reads x (plain and normalised on load), pfst_wino_output writes out (write, accumulate, statistics, BatchNorm-backward
    sums with pre viewed), pfst_wino_dy reads dy: every view kind, against the dense launch bit for bit and against fp64"""
    from pfst_amd._lib import PfstHipError
    n, ci, co, H, W, d = case
    cd = wino_case(*case)
    tol = WINO_TOL[m]
    xd, wd, dyd = cd['x'].to(DEV), cd['w'].to(DEV), cd['dy'].to(DEV)
    f16 = filt == 'f16x3'
    if filt == 'plain':
        (uf, ud), af, ad = ops.wino_pack_weight(wd, m=m), None, None
    elif filt == 'bf16x6':
        (uf, ud), af, ad = ops.wino_pack_weight_split(wd, m=m), None, None
    else:
        uf, ud, af, ad = ops.wino_pack_weight_f16(wd, m=m)
    shape, kind_name = (n, co, H, W), f'm{m} {filt}'

    def fwd(x, out=None, **kw):
        return ops.wino_conv(x, uf, co, d, out=out, m=m, u_amax=af, **kw)

    def bwd(dy, out=None, **kw):
        return ops.wino_conv(dy, ud, ci, d, out=out, m=m, u_amax=ad, **kw)

    def with_stats(x, out):
        sent_stats(ops)
        y, st, sl = fwd(x, out, want_stats=True, want_minmax=True)
        return y, owned(st, 4 * co * sl), sl

    # ---- forward: x viewed, out viewed, both; statistics; accumulate
    y0, p0, sl = with_stats(xd, None)
    close(y0, cd['y'], tol, 'conv-E', f'{kind_name} forward')
    check_stats(ops, p0, sl, co, y0, cd['y'], 'conv-E', True)
    acc0 = fwd(xd, out=dyd.clone(), accumulate=True)
    close(acc0, cd['y'] + cd['dy'].double(), tol, 'conv-E', f'{kind_name} forward')
    for kind in KINDS:
        for which in combos(('x', 'out')):
            xg = in_view(xd, kind) if 'x' in which else None
            og = guard(shape, kind) if 'out' in which else None
            y, p, sl1 = with_stats(xg.view if xg else xd, og.view if og else None)
            assert sl1 == sl and torch.equal(y, y0) and torch.equal(bits(p), bits(p0)), (kind, which)
            if og:
                og.intact(f'{kind} out')
                assert torch.equal(fwd(xg.view if xg else xd, out=og.put(dyd), accumulate=True), acc0), (kind, which, 'accumulate')
                og.intact(f'{kind} out, accumulate')
            if xg:
                unchanged(xg, f'{kind} x')
    # ---- normalise-on-load of a viewed pre-normalisation tensor
    pre, gamma, beta = cd['pre'].to(DEV), cd['gamma'].to(DEV), cd['beta'].to(DEV)
    mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
    ya = ops.amax_slots(pre.device)
    ymat = ops.bn_apply(pre, mean, invstd, gamma, beta, True, amax=ya)
    amax = dict(x_amax=ya) if f16 else {}
    yb0 = fwd(pre, bnl=coef, **amax)
    close(yb0, F.conv2d(ymat.double().cpu(), cd['w'].double(), None, 1, d, d), tol, 'conv-E', f'{kind_name} forward')
    for kind in KINDS:
        pg = in_view(pre, kind)
        assert torch.equal(fwd(pg.view, bnl=coef, **amax), yb0), (kind, 'bnl')
        unchanged(pg, f'{kind} pre')
    # ---- data gradient with the BatchNorm-backward sums: out viewed, pre viewed (whole float4s of aligned planes, else refused)
    dx0, part0, bsl = bwd(dyd, bnb=(pre, coef, True))
    assert torch.equal(dx0, bwd(dyd))
    close(dx0, cd['dx'], tol, 'conv-E', f'{kind_name} dx')
    for kind in KINDS:
        dg, og = in_view(dyd, kind), guard(tuple(xd.shape), kind)
        dx, part, _ = bwd(dg.view, out=og.view, bnb=(pre, coef, True))
        assert torch.equal(dx, dx0) and torch.equal(bits(part), bits(part0)), (kind, 'bnb, dy and out viewed')
        og.intact(f'{kind} out, bnb')
        unchanged(dg, f'{kind} dy')
        pg, og = in_view(pre, kind), guard(tuple(xd.shape), kind)
        if kind == 'slice':
            dx, part, _ = bwd(dyd, out=og.view, bnb=(pg.view, coef, True))
            assert torch.equal(dx, dx0) and torch.equal(bits(part), bits(part0)), (kind, 'bnb, pre viewed')
        else:
            with pytest.raises(PfstHipError):
                bwd(dyd, out=og.view, bnb=(pg.view, coef, True))
            assert bool((og.view == SENT).all()), 'a refused launch wrote its output'
        og.intact(f'{kind} pre, bnb')
        unchanged(pg, f'{kind} pre')
    # ---- weight gradient: x into pfst_wino_input, dy into pfst_wino_dy
    if ops.wino_tiles(H, W, d, m) % 4 == 0:
        split = {'plain': False, 'bf16x6': True, 'f16x3': 2}[filt]
        with det_mode(ops):
            b0 = DwBuf(cd['w'].shape)
            ops.wino_wgrad_(b0.dw, xd, dyd, d, m=m, split=split)
            close(b0.dw, cd['dw'], 2 * tol, 'conv-E', f'{kind_name} dw', cdims=(0, 1))
            b0.intact('dense')
            for kind in KINDS:
                for which in combos(('x', 'dy')):
                    xg = in_view(xd, kind) if 'x' in which else None
                    dg = in_view(dyd, kind) if 'dy' in which else None
                    b = DwBuf(cd['w'].shape)
                    ops.wino_wgrad_(b.dw, xg.view if xg else xd, dg.view if dg else dyd, d, m=m, split=split)
                    if kind == 'slice':
                        assert torch.equal(b.dw, b0.dw), (kind, which)
                    else:
                        close(b.dw, cd['dw'], 2 * tol, 'conv-E', f'{kind_name} dw', cdims=(0, 1))
                    b.intact(f'{kind} {which}')
                    for gd in (xg, dg):
                        if gd:
                            unchanged(gd, f'{kind} {which}')
    report('conv-E')


def test_every_route_is_reached():
    assert SEEN == ROUTES, (sorted(ROUTES - SEEN), sorted(SEEN - ROUTES))
