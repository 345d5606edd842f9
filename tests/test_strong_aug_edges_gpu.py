"""The kernels of csrc/strong_aug.hip -- color_jitter_kernel and blur_pass_kernel -- against the float64 reference of
tests/strong_aug_oracle.py, at the planes, parameters and reaches where they can go wrong.  EVERY element is held to the bound: no share of
pixels is exempt.  tests/test_strong_aug_cpu.py shows on the CPU that these very inputs move by more than ten times the bound under each of
eleven wrong variants of the reference, and that the formulas evaluated in float32 stay within half the jitter bound.

Jitter.  Images are uint8-derived (integer pixels, normalised in float32 as the loader does) with planted black, white, grey, two-channel
tie, primary / secondary and 1-next-to-0 pixels; the 24 op orders are the parameter rows of one n = 24 launch (so row i of `params` must
reach image i), times nine parameter sets (the shipped extremes, factors 0 and 2, hue +-pi, the identity), with and without the
de-normalisation; planes of HW = 1, 15, 1023, 1025 and one 1450 x 1450 plane, where the grid is capped and the stride loop runs.
  bound, per channel in normalised units: 64 x 2^-24 x 255 / std_c x max(1, contrast) x max(1, saturation factor), unit scale without the
  de-normalisation.  64 counts the fp32 roundings of the longest op chain (44) with the eight roundings of an angle at their mean weight
  of 3, and the fp32 2 pi; a factor above 1 multiplies the error a value carries.  The derivation stands at K_JITTER in the oracle module.
  Pixels that reach an HSV step as a black residue (fp64 |max + 1e-8| < 1e-6) get an absolute term of at most 3.8e-7 in unit scale on
  top (jitter_bound: |v| (1 + |s|) of the reference plus what fp32 without FMA can return, x 4).  Out of gamut the bound scales with
  max(1, |s|) of the reference.
  float32 restatement on the CPU, same inputs: 0.29 of the bound (in gamut, both scales), 0.30 (1450 x 1450), 0.27 (out of gamut).
Blur.  Reference: the full-tap separable filter in fp64 on the float32 taps the kernel receives.
  bound per plane: 2^-24 A (nx + ny + 2), A = max |x| of the plane, nx and ny the taps the kernel loops (blur_bound in the oracle module).
  Cases: truncated as production truncates (7 of 9 and 7 of 13 taps), a reach shared by two sigmas (27 of 29 and 27 of 31), untruncated,
  reach 0 (bit-equal to two rounded products), K = 1 (bit-equal to the input), HW = 1023 and 1025 with the border frame and the four
  corner blocks asserted on their own, K / 2 >= n (the reflection wraps more than once), one taps row per image.  The input comes back
  bit-unchanged from every launch.

Worst ratio to the bound measured on the MI355X (every group must stay below 1):
  jitter, de-normalised   1 x 1 0.067, 3 x 5 0.14, 31 x 33 0.24, 25 x 41 0.26, 1450 x 1450 0.30 (its second sweep 0.21); identity against the
                          input 0.26.  Per parameter set at 25 x 41: hi 0.25, lo 0.16, sat0 0.045, sat2 0.17, con2 0.21, con0 / bri0 / bri2
                          below 0.01, ident 0.26
  jitter, unit scale      1 x 1 0.068, 3 x 5 0.14, 31 x 33 0.23, 25 x 41 0.25
  jitter, out of gamut    0.19
  blur                    truncated 0.0006, shared 0.016, full 0.094, HW = 1023 0.069 (frame 0.054, corners 0.023), HW = 1025 0.091 (0.047,
                          0.027), periods 0.028, one_row 0.039, per_image 0.12 (0.12, 0.072, 0.033 by image); reach 0 and K = 1 bit-equal
No pixel of any launch came near the bound: the kernel stays at or below what the float32 restatement shows on the CPU."""
import pytest
import torch

import strong_aug_oracle as SO
from helpers import note, report

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


def run_jitter(ops, img, prm, denorm):
    mean, std = torch.tensor(SO.MEAN, device=DEV), torch.tensor(SO.STD, device=DEV)
    x = img.clone().to(DEV)
    out = ops.color_jitter_(x, prm.to(DEV), mean, std, denorm)
    assert out is x
    out = out.cpu()
    assert bool(torch.isfinite(out).all())
    return out


# ------------------------------------------------------------------------------------------------------------------------------ colour jitter
@pytest.mark.parametrize('denorm', [True, False], ids=['denorm', 'unit'])
@pytest.mark.parametrize('plane', SO.JITTER_PLANES, ids=lambda p: f'{p[0]}x{p[1]}')
def test_jitter_every_order_and_parameter_set(ops, plane, denorm):
    img = SO.jitter_input(24, *plane, denorm)
    group = 'jitter ' + ('denorm' if denorm else 'unit')
    ratios = {}
    for name in SO.PARAM_SETS:
        prm = SO.params_for(name)
        out = run_jitter(ops, img, prm, denorm)
        ratios[name], _, bound = SO.jitter_ratio(out, img, prm, denorm)
        note(group, f'{plane[0]}x{plane[1]}', ratios[name])
        if name == 'ident' and denorm:                  # identity parameters return the input
            back = float(((out.double() - img.double()).abs() / bound).max())
            note(group, 'identity returns the input', back)
            ratios['ident, against the input'] = back
    print(f'{group} {plane}:', {k: f'{v:.3g}' for k, v in ratios.items()})
    report(group)
    assert max(ratios.values()) < 1.0, ratios


def test_jitter_capped_grid(ops):
    """HW = 2 102 500: cdiv(HW, 1024) = 2054 blocks' worth on a grid capped at 2048 -- the elements past 2048 x 1024 come from the stride loop"""
    h, w = SO.JITTER_BIG
    assert (h * w + 1023) // 1024 > 2048
    img = SO.jitter_input(1, h, w, True)
    prm = SO.params_for('hi', 1)[:, [0, 1, 2, 3, 6, 4, 7, 5]]          # order 2 0 3 1
    out = run_jitter(ops, img, prm, True)
    ratio, ref, bound = SO.jitter_ratio(out, img, prm)
    tail = float(((out.double() - ref).abs() / bound).flatten(2)[..., 2048 * 1024:].max())
    note('jitter denorm', '1450x1450', ratio), note('jitter denorm', '1450x1450, elements of the second sweep', tail)
    print(f'1450 x 1450: {ratio:.3g} of the bound, the second sweep {tail:.3g}')
    report('jitter denorm')
    assert ratio < 1.0
    assert not torch.equal(out.flatten(2)[..., 2048 * 1024:], img.flatten(2)[..., 2048 * 1024:]), 'the tail was processed'


def test_jitter_out_of_gamut(ops):
    img, prm = SO.out_of_gamut_input(), SO.out_of_gamut_params()
    out = run_jitter(ops, img, prm, True)
    ratio = SO.jitter_ratio(out, img, prm, True, out_of_gamut=True)[0]
    note('jitter out of gamut', '9x11', ratio)
    report('jitter out of gamut')
    assert ratio < 1.0


# ------------------------------------------------------------------------------------------------------------------------------ gaussian blur
def run_blur(ops, name):
    img, ty, tx, reach = SO.blur_case(name)
    x = img.to(DEV)
    keep = x.clone()
    out = ops.gaussian_blur(x, ty.to(DEV), tx.to(DEV), reach)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32)), 'the input was written'
    assert out.data_ptr() != x.data_ptr() and out.shape == x.shape
    return img, ty, tx, reach, out.cpu()


@pytest.mark.parametrize('name', ['truncated', 'shared', 'full', 'tail_1023', 'tail_1025', 'periods', 'one_row', 'per_image'])
def test_blur_against_the_full_tap_reference(ops, name):
    img, ty, tx, reach, out = run_blur(ops, name)
    ky, kx = ty.shape[1], tx.shape[1]
    if name in ('truncated', 'shared'):
        assert SO.looped(ky, reach) < ky and SO.looped(kx, reach) < kx, 'the kernel truncates both passes'
    assert bool(torch.isfinite(out).all())
    rel = (out.double() - SO.blur(img, ty, tx)).abs() / SO.blur_bound(img, ky, kx, reach)
    per_image = rel.amax((1, 2, 3))
    note('blur', name, float(rel.max()))
    fy, fx = max(ky // 2, 1), max(kx // 2, 1)
    inner = rel[:, :, fy:-fy, fx:-fx]
    frame = rel.clone()
    frame[:, :, fy:-fy, fx:-fx] = 0.0
    corners = torch.stack([rel[:, :, ys, xs].amax() for ys in (slice(0, fy), slice(-fy, None)) for xs in (slice(0, fx), slice(-fx, None))])
    note('blur', name + ', border frame', float(frame.max())), note('blur', name + ', corner blocks', float(corners.max()))
    print(f'blur {name}: per image {[f"{float(v):.3g}" for v in per_image]}, frame {float(frame.max()):.3g}, corners '
          f'{float(corners.max()):.3g}, interior {float(inner.max()) if inner.numel() else 0.0:.3g}')
    report('blur')
    assert float(per_image.max()) < 1.0, 'every image against its own taps'
    assert float(frame.max()) < 1.0 and float(corners.max()) < 1.0


def test_blur_reach_zero_is_the_centre_tap(ops):
    """reach 0: each pass is fmaf(tap, x, 0) -- one rounded product -- of the centre tap"""
    img, ty, tx, reach, out = run_blur(ops, 'centre')
    assert reach == 0 and (ty.shape[1], tx.shape[1]) == (1, 3)
    want = (img * tx[:, 1].view(-1, 1, 1, 1)) * ty[:, 0].view(-1, 1, 1, 1)
    assert torch.equal(out, want)


@pytest.mark.parametrize('name', ['k1', 'k1_row'])
def test_blur_single_tap_returns_the_input(ops, name):
    img, ty, tx, reach, out = run_blur(ops, name)
    assert ty.tolist() == [[1.0]] * 2 and tx.tolist() == [[1.0]] * 2
    assert torch.equal(out.view(torch.int32), img.view(torch.int32))
