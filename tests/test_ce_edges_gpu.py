"""Every kernel of csrc/loss.hip against float64 (tests/ce_oracle.py): the fused bilinear resize + cross-entropy + accuracy and its gradient on
all seven kernels behind pfst_ce_upsample_fwd / _bwd, pseudo_label, label_presence, class_mask, class_mix and confusion_hist -- at ragged,
anisotropic, down-sampling, ratio-1, ratio-2 and 1 x 1 maps, around the C == 8 / 9 switch, with ignore_index a class index, with labels in
[C, 255], in the write and the accumulate form.  Every output is written through a raw call into canary buffers (helpers.Guard for float
planes, Pad below for the rest), every input must come back unchanged.

The host's choice of kernel (loss.hip, pfst_ce_upsample_fwd / _bwd) is restated in ce_route; every launch asserts the route it is there for and
test_every_route_is_reached asserts that the cases reach all three forward and all four backward kernels.

Bounds (reasoned, not fitted).  u = 2^-24, A = the image's max |logit|, m = max(h, w), d = 0 when h / H and w / W are powers of two, else 1.
  tol_z    u A (12 m d + 4), an interpolated logit: the resize bound of test_plane_views_gpu.py (three float32 roundings of the source coordinate,
           values up to m, move each weight by 3 u m and the blend by 2 A per unit of weight; four roundings of the blend).
  tol_lse  tol_z + u (2 C + 8) + u |ref|.  lse = mx + logf(sum_c expf(z_c - mx)): log-sum-exp moves by at most the largest logit error (tol_z).
           The sum S lies in [1, C].  Relative to S: each z_c - mx is rounded once, which scales its term by 1 +- u t, t = mx - z_c, and
           t e^-t <= 1/e per term: <= 0.37 C u; expf is within 2 ulp = 4 u of each term, hence of S: 4 u; C - 1 adds round partial sums <= S:
           (C - 1) u.  So log S is off by (1.37 C + 3) u, logf adds 2 ulp of a value <= log C: 4 u log C, and the final add half an ulp of
           the result: u |ref|.  (1.37 C + 3 + 4 log C) <= 2 C + 8 for every C >= 1 (largest at C = 8: 22.3 against 24).
  acc[0]   sum over valid pixels of w_p (tol_lse + tol_z + 2 u |nll_p|) + u |ref|: per pixel lse - z_label carries both errors and one rounding,
           the product with w_p another (w_p is the float32 product pix_weight * class_weight the kernel forms, the reference uses the same);
           the terms are summed in float64.  ce_finalize: the same bound times loss_weight / numel plus one float32 rounding; the accuracy
           within 100 near_tie / valid of float64 plus a rounding; the bad-label count exact.
  acc[1]   differs from float64 by at most the number of valid pixels whose float64 top-2 logit gap is below 2 tol_z; acc[2], acc[3] exact.
  gradient |got - ref| <= 1e-4 max |ref| + 1e-3 |ref| per element (the per-link bound of DESIGN section 7); at ratio 1 (g_same), where a cell
           receives one term of weight 1, |scale w_p| (p_c (tol_lse + 4 u) + 2 u |p_c - 1{l = c}|): expf(z - lse) moves by p_c times the error
           of lse and is within 2 ulp; p - 1{l = c}, the product with the weight and the product with the scale round once each (the
           difference p - 1 is exact by Sterbenz for p >= 1/2 and an ulp of a value below 1 otherwise).
  accumulate form bit-equal to old + dx; one class: loss and gradient exactly 0, lse the resized logit bit for bit.
  pseudo-labels: max_prob within tol_z + 4 u of float64 (|dp| <= 1/2 max |dz|, then expf, the sum and the division); the label equals the
           float64 arg-max where the float64 top-2 probability gap exceeds 2 tol_z + 8 u, elsewhere either of the two; conf_mask agrees
           where |p_max - thr| > tol_z + 4 u; count == conf_mask.sum().
  label kernels: exact.

Worst measured ratio to each bound, MI355X (kernel; torch's own float32 CPU autograd on the same inputs in brackets, for scale) -- printed by
every test (pytest -s):
  case     lse              loss sum (worst of unweighted / weighted)   gradient
  g_up     0.084 [0.081]    0.0006 [0.0017]                             0.0026 [0.0028]
  g_c9     0.073 [0.079]    0.0004 [0.0011]                             0.0021 [0.0024]
  g_c33    0.082 [0.082]    0.0006 [0.0011]                             0.0015 [0.0015]   (one near tie, the correct count equal)
  g_down   0.037 [0.035]    0.0004 [0.0008]                             0.0070 [0.0069]
  g_same   0.115 [0.115]    0.0039 [0.041]                              0.0016 [0.0012]; against the one-tap bound 0.67 [0.76]
  g_x2     0.201 [0.189]    0.0019 [0.043]                              0.0007 [0.0004]
  g_one    0.032 [0.114]    0.0089 [0.014]                              0.0003 [0.0004]
  g_mixed  0.274 [0.280]    0.0024 [0.017]                              0.0005 [0.0005]
  x4       0.233 [0.233]    0.0031 [0.029]                              0.0005 [0.0006]   (ignore_index 2 and 0 included)
  x8       0.288 [0.288]    0.0026 [0.048]                              0.0005 [0.0008]   (ignore_index 2 and 0 included)
  x4_c1    0.223 [0.169]    0 [0]                                       0 [0]
  ce_finalize: loss at most 0.021, accuracy at most 0.61 (one float32 rounding of a value near 100); the counts equal in every case.
  block kernels against the generic ones (odd label address, misaligned lse, the 8 + 1 class twin): lse bit-equal, gradient 2.8e-7 (x4) and
  5.0e-7 (x8) of the maximum against the 2e-6 allowed; the 6 + 3 class twin of g_up bit-equal in lse and gradient.
  pseudo-labels: max_prob at most 0.087 (g_x2) of the bound; no label off the float64 arg-max in any case.
The lse ratios are largest at the exact ratios, where d = 0 leaves 4 u A for the blend and u (2 C + 8) for the sum: the bound is then within
a factor of four of the error.  The per-link gradient bound is loose at these sizes (few taps per cell); the one-tap bound shows the margin a
bound derived for the shape leaves.
"""

import numpy as np
import pytest
import torch

import ce_oracle as O
from helpers import Guard
from test_hip_ops import g, ops  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = O.U
FILL = {torch.float32: -7777.0, torch.float64: -7777.0, torch.int64: -7777, torch.int32: -7777, torch.uint8: 0xA5}


class Pad:
    """`numel` dense elements of `dtype`, `lead` elements past a 16-byte boundary, between two runs of 64 canary elements"""

    def __init__(self, numel, dtype, lead=0, src=None):
        self.lo, self.n = 64 + lead, numel
        self.flat = torch.full((64 + lead + numel + 64,), FILL[dtype], dtype=dtype, device=DEV)
        assert self.flat.data_ptr() % 16 == 0
        self.view = self.flat[self.lo:self.lo + numel]
        if src is not None:
            self.view.copy_(src.reshape(-1))
        self.src = None if src is None else self.view.clone()

    def ptr(self):
        return self.view.data_ptr()

    def intact(self, what=''):
        out = torch.cat([self.flat[:self.lo], self.flat[self.lo + self.n:]])
        assert bool((out == FILL[self.flat.dtype]).all()), f'{what}: elements outside the {self.flat.dtype} buffer were written'
        if self.src is not None:
            assert torch.equal(self.view, self.src), f'{what}: an input was changed'


def worst(err, bound):
    """the largest ratio of an error to its bound (a bound of 0 admits an error of 0 only)"""
    err, bound = torch.as_tensor(err, dtype=torch.float64), torch.as_tensor(bound, dtype=torch.float64)
    bound = bound.expand_as(err) if bound.dim() else bound
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------- the host's choice, restated
FWD, BWD = {'fwd generic', 'fwd blocks x4', 'fwd blocks x8'}, {'bwd per class', 'bwd cells', 'bwd blocks x4', 'bwd blocks x8'}


def ce_route(C, lo, hi, lse_ptr, pw_ptr, label_ptr, bwd):
    """pfst_ce_upsample_fwd / _bwd: the inter-cell block kernels at the exact ratios 4 and 8 on both axes (C <= 8, 8-byte aligned lse and
    pixel weights for the float2 accesses, 2-byte aligned labels, h within the grid), else one pixel per thread forward and, backward, one
    thread per cell (C <= 8) or per cell and class"""
    (h, w), (H, W) = lo, hi
    blocks_ok = C <= 8 and (lse_ptr | pw_ptr) % 8 == 0 and label_ptr % 2 == 0 and h < 65535 * (15 if bwd else 16)
    for S in (4, 8):
        if blocks_ok and H == S * h and W == S * w:
            return f'{"bwd" if bwd else "fwd"} blocks x{S}'
    if not bwd:
        return 'fwd generic'
    return 'bwd cells' if C <= 8 else 'bwd per class'


EXPECT = {'g_up': ('fwd generic', 'bwd cells'), 'g_c9': ('fwd generic', 'bwd per class'), 'g_c33': ('fwd generic', 'bwd per class'),
          'g_down': ('fwd generic', 'bwd cells'), 'g_same': ('fwd generic', 'bwd cells'), 'g_x2': ('fwd generic', 'bwd cells'),
          'g_one': ('fwd generic', 'bwd cells'), 'g_mixed': ('fwd generic', 'bwd cells'), 'x4': ('fwd blocks x4', 'bwd blocks x4'),
          'x8': ('fwd blocks x8', 'bwd blocks x8'), 'x4_c1': ('fwd blocks x4', 'bwd blocks x4')}


# ------------------------------------------------------------------------------------------------------------------------------ the launches
def p(t):
    return 0 if t is None else t.ptr()


def launch(ops, logits, label, pw, cw, ign, scale, old, lse_lead=0, label_lead=0):
    """forward, backward (write) and backward (accumulate onto `old`) through the C ABI, every output in canaries -> dict"""
    N, C, h, w = logits.shape
    H, W = label.shape[-2:]
    s = ops._stream()
    x = Pad(logits.numel(), torch.float32, src=logits.to(DEV))
    lab = Pad(label.numel(), torch.uint8, lead=label_lead, src=label.to(DEV))
    pwd = None if pw is None else Pad(pw.numel(), torch.float32, src=pw.to(DEV))
    cwd = None if cw is None else Pad(cw.numel(), torch.float32, src=cw.to(DEV))
    g_lse = Guard((1, N, H, W), lead=lse_lead)
    acc = Pad(4, torch.float64, src=torch.zeros(4, dtype=torch.float64, device=DEV))
    acc.src = None
    route = tuple(ce_route(C, (h, w), (H, W), g_lse.view.data_ptr(), p(pwd), lab.ptr(), bwd) for bwd in (False, True))
    ops.call('pfst_ce_upsample_fwd', x.ptr(), N, C, h, w, lab.ptr(), p(pwd), p(cwd), H, W, ign, g_lse.view.data_ptr(), acc.ptr(), s)
    g_dl, g_da = Guard((1, N * C, h, w)), Guard((1, N * C, h, w))
    g_da.put(old.to(DEV).view(1, N * C, h, w))
    for gd, accumulate in ((g_dl, 0), (g_da, 1)):
        ops.call('pfst_ce_upsample_bwd', x.ptr(), N, C, h, w, lab.ptr(), p(pwd), p(cwd), H, W, ign, g_lse.view.data_ptr(), scale,
                 gd.view.data_ptr(), accumulate, s)
    torch.cuda.synchronize()
    what = f'CE {route}'
    for b in (g_lse, g_dl, g_da, acc, x, lab) + tuple(b for b in (pwd, cwd) if b is not None):
        b.intact(what)
    return dict(route=route, lse=g_lse.view[0].clone(), acc=acc.view.clone(), dl=g_dl.view.view(N, C, h, w).clone(),
                dl_acc=g_da.view.view(N, C, h, w).clone(), old=old.to(DEV))


_RUNS = {}


def run(ops, name, weighted, ign=255, lse_lead=0, label_lead=0):
    key = (name, weighted, ign, lse_lead, label_lead)
    if key not in _RUNS:
        d = O.inputs(name)
        _RUNS[key] = launch(ops, d['logits'], d['label'], d['pw'] if weighted else None, d['cw'] if weighted else None, ign, O.scale_of(name),
                            d['old'], lse_lead, label_lead)
    return _RUNS[key]


def test_every_route_is_reached(ops):
    seen = set()
    for name in O.CASES:
        r = run(ops, name, True)
        assert r['route'] == EXPECT[name], (name, r['route'])
        seen |= set(r['route'])
    assert seen == FWD | BWD, (FWD | BWD) - seen
    # the mixed ratio and the exact ratio 2 stay on the generic kernels whatever the alignment; C == 9 at an exact ratio too
    assert ce_route(6, (8, 6), (32, 48), 0, 0, 0, False) == 'fwd generic' and ce_route(6, (8, 6), (32, 48), 0, 0, 0, True) == 'bwd cells'
    assert ce_route(6, (12, 10), (24, 20), 0, 0, 0, True) == 'bwd cells'
    assert ce_route(9, (5, 17), (40, 136), 0, 0, 0, False) == 'fwd generic' and ce_route(9, (5, 17), (40, 136), 0, 0, 0, True) == 'bwd per class'


# ------------------------------------------------------------------------------------------------------------------------- against float64
def check_case(ops, name, weighted, ign):
    C, (h, w), (H, W), N = O.CASES[name]
    ref, t32 = O.reference(name, weighted, ign), O.torch32(name, weighted, ign)
    r = run(ops, name, weighted, ign)
    assert r['route'] == EXPECT[name]
    tag = f'{name} weighted={weighted} ignore={ign} {r["route"]}'
    # log-sum-exp, per pixel
    e_lse = (r['lse'].double().cpu() - ref['lse']).abs()
    q_lse, q_lse32 = worst(e_lse, ref['tol_lse']), worst((t32['lse'].double() - ref['lse']).abs(), ref['tol_lse'])
    # the sums
    acc = r['acc'].cpu()
    q_loss, q_loss32 = worst(abs(float(acc[0]) - ref['loss']), ref['tol_loss']), worst(abs(t32['loss'] - ref['loss']), ref['tol_loss'])
    near = int(ref['near_tie'].sum())
    # gradient, per element
    e_g = (r['dl'].double().cpu() - ref['grad']).abs()
    e_g32 = (t32['grad'].double() - ref['grad']).abs()
    q_g, q_g32 = worst(e_g, O.grad_bound(ref['grad'])), worst(e_g32, O.grad_bound(ref['grad']))
    print(f'{tag}: worst ratio to the bound: lse {q_lse:.3g} [{q_lse32:.3g}]  loss sum {q_loss:.3g} [{q_loss32:.3g}]  gradient {q_g:.3g} [{q_g32:.3g}]'
          f'  correct {int(acc[1])} vs {ref["correct"]} (near ties {near})')
    assert q_lse <= 1.0, f'{tag}: lse {q_lse:.3g} x the bound'
    assert q_loss <= 1.0, f'{tag}: loss sum {q_loss:.3g} x the bound'
    assert float(acc[2]) == ref['n_valid'] and float(acc[3]) == ref['n_bad'], (acc.tolist(), ref['n_valid'], ref['n_bad'])
    assert ref['n_bad'] > 0
    assert abs(float(acc[1]) - ref['correct']) <= near, (float(acc[1]), ref['correct'], near)
    assert q_g <= 1.0, f'{tag}: gradient {q_g:.3g} x the bound'
    if name == 'g_same':
        q_s, q_s32 = worst(e_g, O.grad_bound_same(name, ref)), worst(e_g32, O.grad_bound_same(name, ref))
        print(f'{tag}: gradient against the one-tap bound {q_s:.3g} [{q_s32:.3g}]')
        assert q_s <= 1.0, f'{tag}: gradient {q_s:.3g} x the one-tap bound'
    # the accumulate form adds the written form's value, bit for bit
    assert torch.equal(r['dl_acc'], r['old'] + r['dl']), f'{tag}: accumulate differs from old + dx'
    # ce_finalize
    numel, lw = N * H * W, float(np.float32(O.LOSS_WEIGHT))
    out = ops.ce_finalize(r['acc'], numel, O.LOSS_WEIGHT).double().cpu()
    ref0 = lw * ref['loss'] / numel
    eps = 1.1920928955078125e-07
    ref1 = (ref['correct'] + eps) * 100.0 / (ref['n_valid'] + eps)
    q_f0 = worst(abs(float(out[0]) - ref0), lw * ref['tol_loss'] / numel + U * abs(ref0))
    q_f1 = worst(abs(float(out[1]) - ref1), 100.0 * near / ref['n_valid'] + U * abs(ref1))
    print(f'{tag}: ce_finalize loss {q_f0:.3g}  accuracy {q_f1:.3g}')
    assert q_f0 <= 1.0 and q_f1 <= 1.0 and float(out[2]) == ref['n_bad'], (out.tolist(), ref0, ref1, ref['n_bad'])
    if C == 1:
        d = O.inputs(name)
        up = ops.resize_bilinear(d['logits'].to(DEV), (H, W))[:, 0]
        assert torch.equal(r['lse'], up), 'one class: lse is the resized logit'
        assert float(acc[0]) == 0.0 and float(r['dl'].abs().max()) == 0.0 and float(out[0]) == 0.0


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('name', list(O.CASES))
def test_ce_against_fp64(ops, name, weighted):
    check_case(ops, name, weighted, 255)


@pytest.mark.parametrize('name,ign', O.IGNORE_CASES)
def test_ce_with_a_class_as_ignore_index(ops, name, ign):
    """255 is then a bad label like any other in [C, 255]: no term, counted in acc[3]"""
    ref = O.reference(name, True, ign)
    assert int((ref['lab'] == ign).sum()) > 0 and int((ref['bad'] & (ref['lab'] == 255)).sum()) > 0
    check_case(ops, name, True, ign)
    assert float(run(ops, name, True, ign)['acc'][3]) > float(run(ops, name, True)['acc'][3])


# --------------------------------------------------------------------------------------------------------------------- promised identities
@pytest.mark.parametrize('name,extra', [('g_up', 3), ('x8', 1)])
def test_padding_classes_change_nothing(ops, name, extra):
    """the case's classes plus classes of constant logit -1e30 that are never labelled.  g_up (6 + 3): the two-pass forward against the register
    path and ce_bwd_kernel against ce_bwd_cells_kernel, bit for bit.  x8 (8 + 1): the generic kernels against the block kernels -- lse bit for
    bit, the gradient in another summation order"""
    C = O.CASES[name][0]
    d, a = O.inputs(name), run(ops, name, True)
    cw = torch.cat([d['cw'], torch.full((extra,), 1.5)])
    old = torch.cat([d['old'], torch.zeros(d['old'].shape[0], extra, *d['old'].shape[2:])], 1)
    b = launch(ops, O.padded_twin(name, extra), d['label'], d['pw'], cw, 255, O.scale_of(name), old)
    assert b['route'] == ('fwd generic', 'bwd per class') and a['route'] == EXPECT[name]
    assert torch.equal(a['lse'], b['lse']), f'{name}: lse of the padded twin differs'
    assert torch.equal(a['acc'][1:], b['acc'][1:])
    assert float(b['dl'][:, C:].abs().max()) == 0.0, 'padded classes receive no gradient'
    if name == 'g_up':
        assert float(a['acc'][0]) == float(b['acc'][0]) or abs(float(a['acc'][0] - b['acc'][0])) <= 1e-12 * abs(float(a['acc'][0]))   # fp64 atomics: order
        assert torch.equal(a['dl'], b['dl'][:, :C]), 'ce_bwd_kernel differs from ce_bwd_cells_kernel'
        assert torch.equal(a['dl_acc'], b['dl_acc'][:, :C])
    else:
        e = float((a['dl'] - b['dl'][:, :C]).abs().max() / a['dl'].abs().max())
        print(f'{name}: block gradient against the per-class gather of the padded twin: {e:.3g} of the maximum')
        assert e < 2e-6


@pytest.mark.parametrize('name', ['x4', 'x8'])
def test_odd_label_address_and_misaligned_lse_take_the_generic_route(ops, name):
    a = run(ops, name, True)
    odd = run(ops, name, True, label_lead=1)
    off = run(ops, name, True, lse_lead=1)
    assert a['route'] == EXPECT[name] and odd['route'] == off['route'] == ('fwd generic', 'bwd cells')
    for b, what in ((odd, 'label map at an odd address'), (off, 'lse 4 bytes past an 8-byte boundary')):
        assert torch.equal(a['lse'], b['lse']), f'{name}, {what}: lse differs from the block kernel'
        assert torch.equal(a['acc'][1:], b['acc'][1:])
        assert abs(float(a['acc'][0] - b['acc'][0])) <= 1e-12 * abs(float(a['acc'][0]))
        e = float((a['dl'] - b['dl']).abs().max() / b['dl'].abs().max())
        print(f'{name}, {what}: block gradient against the per-cell gather: {e:.3g} of the maximum')
        assert e < 2e-6
    assert torch.equal(odd['dl'], off['dl']) and torch.equal(odd['dl_acc'], off['dl_acc'])


def test_backward_wrapper_refuses_what_the_forward_wrapper_refuses(ops):
    d = O.inputs('g_up')
    N, C, h, w = d['logits'].shape
    big = torch.randn(N, C + 2, h, w, device=DEV)
    view = big[:, 1:C + 1]
    l8, pw, cw = d['label'].to(DEV), d['pw'].to(DEV), d['cw'].to(DEV)
    assert not view.is_contiguous()
    with pytest.raises(ValueError, match='contiguous'):
        ops.ce_upsample_fwd(view, l8)
    lse, _ = ops.ce_upsample_fwd(view.contiguous(), l8, pw, cw)
    with pytest.raises(ValueError, match='contiguous'):
        ops.ce_upsample_bwd(view, l8, lse, 0.01)
    with pytest.raises(ValueError, match='contiguous'):
        ops.ce_upsample_bwd(view.contiguous(), l8[:, :, ::2], lse, 0.01)
    with pytest.raises(ValueError, match='contiguous'):
        ops.ce_upsample_bwd(view.contiguous(), l8, lse, 0.01, torch.rand(N, 50, 74, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError, match='contiguous'):
        ops.ce_upsample_bwd(view.contiguous(), l8, lse, 0.01, pw, torch.rand(2 * C, device=DEV)[::2])
    with pytest.raises(TypeError):
        ops.ce_upsample_bwd(view.contiguous(), l8.long(), lse, 0.01)
    with pytest.raises(TypeError):
        ops.ce_upsample_bwd(view.contiguous().double(), l8, lse, 0.01)
    with pytest.raises(TypeError):
        ops.ce_upsample_bwd(view.contiguous(), l8, lse, 0.01, pw.double())
    with pytest.raises(TypeError):
        ops.ce_upsample_bwd(view.contiguous(), l8, lse, 0.01, pw, cw.double())
    with pytest.raises(TypeError):
        ops.ce_upsample_fwd(view.contiguous(), l8, pw, cw.double())
    got = ops.ce_upsample_bwd(view.contiguous(), l8, lse, 0.01, pw, cw)
    assert got.shape == (N, C, h, w) and bool(torch.isfinite(got).all())


# --------------------------------------------------------------------------------------------------------------------------- pseudo-labels
@pytest.mark.parametrize('name', list(O.PSEUDO))
def test_pseudo_label_against_fp64(ops, name):
    C, (h, w), (H, W), N = O.PSEUDO[name]
    ref = O.pseudo_reference(name)
    x = Pad(N * C * h * w, torch.float32, src=O.inputs(name)['logits'].to(DEV))
    n = N * H * W
    for thr in O.THRESHOLDS:
        l64, l8, cnt = Pad(n, torch.int64), Pad(n, torch.uint8), Pad(1, torch.int64)
        conf, prob = Guard((1, N, H, W)), Guard((1, N, H, W), lead=1)
        ops.call('pfst_pseudo_label', x.ptr(), N, C, h, w, H, W, thr, l64.ptr(), l8.ptr(), cnt.ptr(), conf.view.data_ptr(), prob.view.data_ptr(),
                 ops._stream())
        torch.cuda.synchronize()
        for b in (x, l64, l8, cnt, conf, prob):
            b.intact(f'pseudo_label {name} thr={thr}')
        lab = l64.view.view(N, H, W).cpu()
        assert torch.equal(lab, l8.view.view(N, H, W).cpu().long()), 'the u8 and the i64 map differ'
        assert bool(((lab == ref['first']) | (~ref['sure'] & (lab == ref['second']))).all()), \
            f'{name}: {int((lab != ref["first"]).sum())} labels differ from the float64 arg-max, {int((~ref["sure"]).sum())} pixels are near ties'
        pm, cm = prob.view[0].double().cpu(), conf.view[0].cpu()
        q_p = worst((pm - ref['pmax']).abs(), ref['tol_p'])
        print(f'pseudo_label {name} thr={thr}: worst ratio to the bound, max_prob {q_p:.3g}; labels off the float64 arg-max: {int((lab != ref["first"]).sum())}')
        assert q_p <= 1.0, f'{name}: max_prob {q_p:.3g} x the bound'
        assert bool(((cm == 0) | (cm == 1)).all())
        clear = (ref['pmax'] - thr).abs() > ref['tol_p']
        assert torch.equal(cm[clear], (ref['pmax'] >= thr).float()[clear]), 'conf_mask differs from float64 away from the threshold'
        assert int(cnt.view[0]) == int(cm.sum())
        assert thr != 0.0 or int(cnt.view[0]) == n
        assert thr != 1.5 or int(cnt.view[0]) == 0
        if C == 1:
            assert bool((pm == 1.0).all()) and bool((lab == 0).all())
    if O.is_pow2_ratio((h, w), (H, W)):
        # exact coordinates and weights: torch's device softmax -> max of the resized logits, bit for bit (the rule of the existing tie test)
        up = ops.resize_bilinear(x.view.view(N, C, h, w), (H, W))
        assert worst((up.double().cpu() - O.upsampled(O.inputs(name)['logits'], (H, W))).abs(), O.tol_z(name).unsqueeze(1)) <= 1.0
        p_dev, l_dev = torch.max(torch.softmax(up, 1), 1)
        assert torch.equal(l64.view.view(N, H, W), l_dev), f'{name}: the map differs from torch.max(torch.softmax) on the device'


def test_pseudo_label_without_the_optional_outputs(ops):
    """null conf_mask / max_prob / i64 pointers: the other outputs are the same"""
    name = 'g_up'
    C, (h, w), (H, W), N = O.PSEUDO[name]
    x = O.inputs(name)['logits'].to(DEV)
    l64, l8, cnt, conf, prob = ops.pseudo_label(x, (H, W), 0.9, want_conf=True, want_prob=True)
    none, l8b, cntb = ops.pseudo_label(x, (H, W), 0.9, want_i64=False)
    assert none is None and torch.equal(l8, l8b) and torch.equal(cnt, cntb) and int(cnt) == int(conf.sum())


# ---------------------------------------------------------------------------------------------------------------------------- label kernels
@pytest.mark.parametrize('n', [1, 255, 2000])
def test_label_presence(ops, n):
    maps = [torch.randint(0, 6, (n,), generator=g(n), dtype=torch.uint8)]
    maps[0][-1] = 200                                                            # a value that occurs only in the last element
    maps.append(((torch.arange(n) + 1) % 256).to(torch.uint8))                   # n = 2000: all 256 values; 255: every value but 0
    for m in maps:
        got = ops.label_presence(m.to(DEV)).cpu()
        assert got.dtype == torch.int32 and torch.equal(got.long(), (torch.bincount(m.long(), minlength=256) > 0).long())
    assert n < 256 or int(got.sum()) == 256


MASK_ROWS = {1: [[2], [255], [300], [-1]],
             4: [[0, 3, 255, -1], [1, 1, 2, 300], [5, 4, 0, 1], [-1, -1, -1, -1]],
             256: [list(range(256)), list(range(100, 356)), [7] * 256, [-1] * 255 + [9]]}


def mask_reference(gt, classes):
    """gt long [N, HW], classes [N, K] -> long [N, HW]: 1 where the pixel's label is one of the image's classes in [0, 256)"""
    ref = torch.zeros_like(gt)
    for i, row in enumerate(classes.tolist()):
        for c in set(row):
            if 0 <= c < 256:
                ref[i] |= (gt[i] == c).long()
    return ref


def label_maps(N, HW, seed):
    gt = torch.randint(0, 12, (N, HW), generator=g(seed))
    gt[torch.rand(N, HW, generator=g(seed + 1)) < 0.1] = 255
    gt[:, ::17] = torch.randint(0, 256, gt[:, ::17].shape, generator=g(seed + 2))
    return gt


@pytest.mark.parametrize('K', [1, 4, 256])
@pytest.mark.parametrize('HW', [63, 2000])
def test_class_mask(ops, HW, K):
    N = 4
    gt = label_maps(N, HW, 7)
    classes = torch.tensor(MASK_ROWS[K], dtype=torch.int32)
    gtd = Pad(N * HW, torch.uint8, src=gt.to(torch.uint8).to(DEV))
    cls = Pad(N * K, torch.int32, src=classes.to(DEV))
    mask = Pad(N * HW, torch.uint8, lead=1)
    ops.call('pfst_class_mask', gtd.ptr(), cls.ptr(), K, mask.ptr(), N, HW, ops._stream())
    torch.cuda.synchronize()
    for b in (gtd, cls, mask):
        b.intact(f'class_mask HW={HW} K={K}')
    ref = mask_reference(gt, classes)
    assert torch.equal(mask.view.view(N, HW).cpu().long(), ref)
    assert 0 < int(ref.sum()) < ref.numel()
    assert torch.equal(ops.class_mask(gtd.view.view(N, 1, 1, HW), cls.view.view(N, K)).view(N, HW), mask.view.view(N, HW))


@pytest.mark.parametrize('Cimg', [1, 3, 4])
@pytest.mark.parametrize('HW', [63, 2000])
def test_class_mix(ops, HW, Cimg):
    N = 3
    gt, pl = label_maps(N, HW, 11), torch.randint(0, 6, (N, HW), generator=g(12))
    m = (torch.rand(N, HW, generator=g(13)) < 0.4).long()
    m[1] = 0
    img, trg = torch.randn(N, Cimg, HW, generator=g(14)), torch.randn(N, Cimg, HW, generator=g(15))
    tw = torch.rand(N, HW, generator=g(16))
    src = [Pad(t.numel(), dt, src=t.to(dt).to(DEV)) for t, dt in ((img, torch.float32), (trg, torch.float32), (gt, torch.uint8), (pl, torch.uint8),
                                                                   (m, torch.uint8), (tw, torch.float32))]
    ref_img = torch.where(m.bool().unsqueeze(1), img, trg)
    ref_lbl = torch.where(m.bool(), gt, pl)
    for count, use_tw, want64 in ((0, False, True), (N * HW, False, False), (1, False, True), (777, True, True), (5, True, False)):
        cnt = Pad(1, torch.int64, src=torch.tensor([count], device=DEV))
        mimg, mw = Guard((1, N * Cimg, 1, HW), lead=1), Guard((1, N, 1, HW))
        ml, ml64 = Pad(N * HW, torch.uint8, lead=1), Pad(N * HW, torch.int64)
        ops.call('pfst_class_mix', src[0].ptr(), src[1].ptr(), src[2].ptr(), src[3].ptr(), src[4].ptr(), cnt.ptr(), src[5].ptr() if use_tw else 0,
                 mimg.view.data_ptr(), ml.ptr(), ml64.ptr() if want64 else 0, mw.view.data_ptr(), N, Cimg, HW, ops._stream())
        torch.cuda.synchronize()
        what = f'class_mix Cimg={Cimg} HW={HW} count={count} trg_weight={use_tw} i64={want64}'
        for b in src + [cnt, mimg, mw, ml, ml64]:
            b.intact(what)
        assert torch.equal(mimg.view.view(N, Cimg, HW).cpu(), ref_img), what
        assert torch.equal(ml.view.view(N, HW).cpu().long(), ref_lbl), what
        if want64:
            assert torch.equal(ml64.view.view(N, HW).cpu(), ref_lbl), what
        else:
            assert bool((ml64.view == FILL[torch.int64]).all()), 'a null i64 pointer: nothing written'
        q = torch.tensor(np.float32(count / (N * HW)))                  # the reference's Python double, stored into a float32 tensor
        ref_w = torch.where(m.bool(), torch.ones(N, HW), tw if use_tw else q.expand(N, HW))
        assert torch.equal(mw.view.view(N, HW).cpu(), ref_w), what
    assert float(np.float32(1 / (N * HW))) > 0


def hist_reference(pred, label, C, ignore):
    keep = label != ignore
    p, l = pred[keep], label[keep]
    inter = torch.bincount(p[(p == l) & (p < C)], minlength=C)
    return torch.cat([inter, torch.bincount(p[p < C], minlength=C), torch.bincount(l[l < C], minlength=C)])


@pytest.mark.parametrize('C', [1, 6, 255])
@pytest.mark.parametrize('n', [1, 2000])
def test_confusion_hist(ops, n, C):
    hi = min(C + 3, 256)
    for ignore in (255, 0 if C == 1 else 2):
        hist = Pad(3 * C, torch.int64, src=torch.zeros(3 * C, dtype=torch.int64, device=DEV))
        hist.src = None
        ref = torch.zeros(3 * C, dtype=torch.int64)
        for call in range(2):                                                       # two calls accumulate into one histogram
            pred = torch.randint(0, hi, (n,), generator=g(20 + call))              # predictions >= C occur
            label = torch.where(torch.rand(n, generator=g(22 + call)) < 0.6, pred, torch.randint(0, hi, (n,), generator=g(24 + call)))
            label[torch.rand(n, generator=g(26 + call)) < 0.1] = 255
            if n == 1:
                pred[0] = label[0] = (C - 1 if call else min(C, 254))
            pd, ld = Pad(n, torch.uint8, lead=1, src=pred.to(torch.uint8).to(DEV)), Pad(n, torch.uint8, src=label.to(torch.uint8).to(DEV))
            ops.confusion_hist_(hist.view, pd.view, ld.view, C, ignore)
            torch.cuda.synchronize()
            for b in (hist, pd, ld):
                b.intact(f'confusion_hist C={C} n={n}')
            ref += hist_reference(pred, label, C, ignore)
            assert torch.equal(hist.view.cpu(), ref), (C, n, ignore, call)
        assert n == 1 or int(ref.sum()) > 0
