"""The fp64 reference of the strong-augmentation tests (tests/strong_aug_oracle.py) against independent known answers, the host helpers of
pfst_amd/strong_aug.py, and two statements about the GPU tests' own inputs: (i) this module's formulas evaluated in float32 on the CPU stay
within HALF the jitter bound on them (so the bound's count of roundings is not too small, and whatever a kernel shows beyond it is the
kernel's), (ii) every deliberately wrong variant of the reference moves them by more than ten times the bound (so the shapes and parameters
are ones where a wrong kernel shows).  No GPU.

Measured here (the only measured inputs of the bounds):
  float32 restatement vs fp64, worst ratio to the jitter bound over every plane, parameter set, order and pixel:
      de-normalised 0.293, unit scale 0.294, the 1450 x 1450 plane 0.297, out of gamut 0.265       (allowed: 0.5)
  fp64 weight of the taps dropped at the host's reach, K = 103: 7.7e-155 for sigma 0.15, 4.3e-43 for 0.5, 4.6e-33 for 1.15 (allowed: 2^-60)"""
import colorsys
import math

import numpy as np
import pytest
import torch

import strong_aug_oracle as SO
from strong_aug_oracle import TWO_PI


# ------------------------------------------------------------------------------------------------------------- the oracle's known answers
def _gamut_pixels(n=400):
    g = torch.Generator().manual_seed(5)
    x = torch.rand(n, 3, generator=g, dtype=torch.float64)
    x[:40, 1] = x[:40, 0]                      # r == g
    x[40:80, 2] = x[40:80, 1]                  # g == b
    x[80:120, 2] = x[80:120, 0]                # r == b
    x[120:130] = x[120:130, :1]                # greys
    return x[x.amax(1) >= 0.1]


def test_hsv_matches_colorsys():
    """colorsys has s = d / max: ours differs by the 1e-8, i.e. by 1e-8 / (max + 1e-8) <= 1e-7 relative at max >= 0.1; hue and value are the
    same expressions up to fp64 rounding (a few 2^-53 of values <= 6)"""
    x = _gamut_pixels()
    assert x.shape[0] > 300
    h, s, v = SO.rgb_to_hsv(x[:, 0], x[:, 1], x[:, 2])
    back = SO.hsv_to_rgb(h, s, v)
    for i, (r, g, b) in enumerate(x.tolist()):
        ch, cs, cv = colorsys.rgb_to_hsv(r, g, b)
        assert float(v[i]) == cv
        assert abs(float(s[i]) - cs) <= 1e-8 / (cv + 1e-8) * cs + 1e-15
        if cs > 0:
            assert abs(float(h[i]) - TWO_PI * ch) <= 1e-13
        want = colorsys.hsv_to_rgb(float(h[i]) / TWO_PI, float(s[i]), float(v[i]))
        assert max(abs(float(back[c, i]) - want[c]) for c in range(3)) <= 1e-14
        assert max(abs(float(back[c, i]) - (r, g, b)[c]) for c in range(3)) <= 1.1e-7      # the round trip: the 1e-8 again


def test_jitter_identities():
    x = _gamut_pixels().t().reshape(1, 3, 1, -1)
    n = x.shape[-1]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        ident = torch.tensor([[1.0, 1.0, 1.0, 0.0] + order])
        assert float((SO.jitter(x, ident, denorm=False) - x).abs().max()) <= 1.1e-7
        grey = SO.jitter(x, torch.tensor([[1.0, 1.0, 0.0, 0.0] + order]), denorm=False)
        assert torch.equal(grey[0, 0], grey[0, 1]) and torch.equal(grey[0, 1], grey[0, 2])
        assert float((grey[0, 0] - x[0].amax(0)).abs().max()) <= 1e-15
    prim = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], dtype=torch.float64).t().reshape(1, 3, 1, 3)
    rot = SO.jitter(prim, torch.tensor([[1.0, 1.0, 1.0, TWO_PI / 3, 0, 1, 2, 3]]), denorm=False)       # red -> green -> blue -> red
    assert float((rot - prim.roll(1, 1)).abs().max()) <= 1e-6          # float32 parameter row: 2 pi / 3 to 2^-24
    # the normalised route: identity parameters return the input
    img = SO.jitter_input(24, 31, 33, True)
    assert float((SO.jitter(img, SO.params_for('ident')) - img.double()).abs().max()) <= 1.1e-7 * 255 / min(SO.STD)
    assert n > 300


def test_blur_known_answers():
    ty, tx = SO._explicit_taps(2, 7, 11), SO._explicit_taps(2, 5, 12)
    const = torch.full((2, 3, 9, 8), 2.5)
    assert float((SO.blur(const, ty, tx) - 2.5).abs().max()) <= 1e-6           # the float32 taps sum to 1 within 2^-22
    imp = torch.zeros(2, 1, 21, 17)
    imp[:, :, 10, 8] = 1.0
    out = SO.blur(imp, ty, tx)
    for i in range(2):
        want = torch.zeros(21, 17, dtype=torch.float64)
        want[7:14, 6:11] = ty[i].double().flip(0).view(7, 1) * tx[i].double().flip(0).view(1, 5)
        assert float((out[i, 0] - want).abs().max()) <= 1e-16
    # an impulse one pixel from the left border of a row, K = 5: position 0 collects taps 1 and 3 (index -1 folds onto 1), position 1 taps
    # 0 and 2 (its index -1 likewise), then taps 1 and 0 directly
    row = torch.zeros(1, 1, 1, 8)
    row[..., 1] = 1.0
    t = tx[:1].double()[0]
    got = SO.blur(row, torch.ones(1, 1), tx[:1])[0, 0, 0]
    want = torch.tensor([t[1] + t[3], t[0] + t[2], t[1], t[0], 0, 0, 0, 0], dtype=torch.float64)
    assert float((got - want).abs().max()) <= 1e-16
    # more than one period: n = 3, indices -4 .. 6 fold onto 0 1 2 1 0 1 2 1 0 1 2
    assert SO.reflect_table(3, 9)[0].tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert SO.reflect_table(1, 5).tolist() == [[0] * 5]
    assert SO.reflect_table(4, 3).tolist() == [[1, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 2]]


# ------------------------------------------------------------------------------------------------------------- the host helpers
def test_blur_kernel_size_sweep():
    from pfst_amd.strong_aug import _blur_kernel_size
    for n in range(1, 2049):
        k = _blur_kernel_size(n)
        assert k == int(np.floor(np.ceil(0.1 * n) - 0.5 + np.ceil(0.1 * n) % 2))         # dacs_transforms.py:94-101
        assert k % 2 == 1 and k >= 1
        assert 2 * (k // 2) < n                       # the reflection never wraps twice at a size the step can see
    assert _blur_kernel_size(1024) == 103


@pytest.mark.parametrize('k', [1, 3, 9, 13, 31, 103])
@pytest.mark.parametrize('sigma', [0.15, 0.5, 1.15])
def test_gauss_taps(k, sigma):
    from pfst_amd.strong_aug import _gauss_taps
    t = _gauss_taps(k, sigma)
    assert t.dtype == torch.float32 and t.shape == (k,)
    assert torch.equal(t, t.flip(0))
    assert abs(float(t.sum()) - 1.0) <= 2.0 ** -22
    want = torch.from_numpy(SO.gauss_taps64(k, sigma))
    normal = want >= 2.0 ** -126                   # below float32's normal range a tap is held to the subnormal spacing instead
    rel = float(((t.double() - want).abs() / want)[normal].max())
    print(f'K {k} sigma {sigma}: worst relative difference from fp64 {rel / 2.0 ** -23:.3g} x 2^-23')
    assert rel <= 2.0 ** -23
    assert float((t.double() - want).abs()[~normal].max() if bool((~normal).any()) else 0.0) <= 2.0 ** -149


@pytest.mark.parametrize('sigma', [0.15, 0.5, 1.15])
def test_dropped_taps_weigh_nothing(sigma):
    from pfst_amd.strong_aug import _blur_kernel_size
    K = _blur_kernel_size(1024)
    reach = SO.host_reach([sigma])
    assert reach == {0.15: 3, 0.5: 6, 1.15: 13}[sigma] and K // 2 > reach
    w = SO.gauss_taps64(K, sigma)
    dropped = float(w[:K // 2 - reach].sum() + w[K // 2 + reach + 1:].sum())
    print(f'sigma {sigma}: reach {reach}, fp64 weight of the dropped taps {dropped:.3g}')
    assert dropped < 2.0 ** -60


# ------------------------------------------------------------------------------------------------------------- float32 headroom
def _fp32_ratio(img, prm, denorm, out_of_gamut=False):
    got = SO.jitter_ex(img, prm, denorm=denorm, dtype=torch.float32)[0]
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    return SO.jitter_ratio(got, img, prm, denorm, out_of_gamut)[0]


@pytest.mark.parametrize('denorm', [True, False])
def test_float32_restatement_stays_within_half_the_jitter_bound(denorm):
    worst = 0.0
    for h, w in SO.JITTER_PLANES:
        img = SO.jitter_input(24, h, w, denorm)
        for name in SO.PARAM_SETS:
            worst = max(worst, _fp32_ratio(img, SO.params_for(name), denorm))
    print(f'denorm {denorm}: float32 restatement at {worst:.3g} of the bound')
    assert worst <= 0.5


def test_float32_restatement_big_plane_and_out_of_gamut():
    img = SO.jitter_input(1, *SO.JITTER_BIG, True)
    big = _fp32_ratio(img, SO.params_for('hi', 1)[:, [0, 1, 2, 3, 6, 4, 7, 5]], True)
    oog = _fp32_ratio(SO.out_of_gamut_input(), SO.out_of_gamut_params(), True, out_of_gamut=True)
    print(f'float32 restatement: 1450 x 1450 at {big:.3g} of the bound, out of gamut at {oog:.3g}')
    assert big <= 0.5 and oog <= 0.5


def test_input_conditions():
    """black pixels exist and their residues are off the singularity of s; the out-of-gamut group is as the bound assumes"""
    img = SO.jitter_input(24, 31, 33, True)
    _, allow, smax = SO.jitter_ex(img, SO.params_for('hi'))
    black = allow > 0
    assert int(black.sum()) >= 24 and float(smax[black].max()) <= SO.BLACK_S_MAX
    assert float(allow.max()) <= 1e-6, 'the absolute term stays at a few 1e-7'
    print(f'absolute term at most {float(allow.max()):.3g}, |s| at black pixels at most {float(smax[black].max()):.3g}')
    x = SO.out_of_gamut_input().double() * torch.tensor(SO.STD).view(1, 3, 1, 1) + torch.tensor(SO.MEAN).view(1, 3, 1, 1)
    x = x / 255.0
    assert float(x.min()) >= -0.5 - 1e-6 and float(x.max()) <= 1.5 + 1e-6 and float(x.amax(1).min()) >= 0.05
    assert float(x.min()) < -0.3 and float(x.max()) > 1.3
    assert {int(r[4]) for r in SO.out_of_gamut_params()} == {2, 3}
    assert 1.0 < float(SO.jitter_ex(SO.out_of_gamut_input(), SO.out_of_gamut_params())[2].max()) < 40.0


# ------------------------------------------------------------------------------------------------------------- sensitivity
JITTER_SEES = {
    'hue_sign': ['hi', 'lo', 'con2'],                      # (+-pi is its own negative)
    'no_sat_clamp': ['hi', 'sat2'],
    'order_shift': ['hi', 'lo', 'sat2', 'con2'],
    'std_swap': ['hi', 'lo', 'sat0', 'con2'],
    'next_params': ['hi', 'lo', 'sat2'],                    # the rows of one set differ in the order only
    'sector_swap': ['hi', 'lo', 'sat2', 'con2'],             # (under identity parameters the two HSV steps undo the swap)
}


@pytest.mark.parametrize('wrong', SO.JITTER_WRONG)
def test_wrong_jitter_variants_show_on_the_gpu_inputs(wrong):
    assert set(JITTER_SEES) == set(SO.JITTER_WRONG)
    for plane in [(31, 33), (25, 41)]:
        img = SO.jitter_input(24, *plane, True)
        for name in JITTER_SEES[wrong]:
            prm = SO.params_for(name)
            bad = SO.jitter_ex(img, prm, wrong=wrong)[0]
            ratio = SO.jitter_ratio(bad, img, prm)[0]
            print(f'{wrong} on {plane} {name}: {ratio:.3g} x the bound')
            assert ratio > 10.0


BLUR_SEES = {
    'edge_repeat': ['shared', 'full', 'tail_1023', 'tail_1025', 'periods', 'one_row', 'per_image'],
    'shift': ['truncated', 'shared', 'full', 'tail_1023', 'tail_1025', 'periods', 'per_image'],
    'short_reach': ['shared'],                              # 13 - ceil(10 x 1.15) = 1
    'next_taps': ['shared', 'full', 'per_image', 'periods'],
    'swap_xy': ['per_image'],                               # sigma 1.15 in image 2, K = 5 against 7: the shorter window cuts real weight
}


@pytest.mark.parametrize('wrong', SO.BLUR_WRONG)
def test_wrong_blur_variants_show_on_the_gpu_inputs(wrong):
    assert set(BLUR_SEES) == set(SO.BLUR_WRONG)
    for name in BLUR_SEES[wrong]:
        img, ty, tx, reach = SO.blur_case(name)
        ref = SO.blur(img, ty, tx)
        if wrong == 'short_reach':
            sig = SO.BLUR_CASES[name][1]
            bad = SO.blur(img, ty, tx, reach=reach - int(math.ceil(10.0 * max(sig))))
        else:
            bad = SO.blur(img, ty, tx, wrong=wrong)
        ratio = float(((bad - ref).abs() / SO.blur_bound(img, ty.shape[1], tx.shape[1], reach)).max())
        print(f'{wrong} on {name}: {ratio:.3g} x the bound')
        assert ratio > 10.0
    if wrong == 'next_taps':                                 # every image of the per-image case, not only the worst
        img, ty, tx, reach = SO.blur_case('per_image')
        d = (SO.blur(img, ty, tx, wrong=wrong) - SO.blur(img, ty, tx)).abs() / SO.blur_bound(img, ty.shape[1], tx.shape[1], reach)
        assert float(d.amax((1, 2, 3)).min()) > 10.0


def test_truncation_at_the_host_reach_is_invisible():
    """the full-tap reference and the reference truncated as the kernel truncates agree far below the bound on the truncated cases"""
    for name in ('truncated', 'shared'):
        img, ty, tx, reach = SO.blur_case(name)
        assert SO.looped(ty.shape[1], reach) < ty.shape[1] and SO.looped(tx.shape[1], reach) < tx.shape[1]
        assert reach == SO.host_reach(SO.BLUR_CASES[name][1])
        d = (SO.blur(img, ty, tx) - SO.blur(img, ty, tx, reach=reach)).abs() / SO.blur_bound(img, ty.shape[1], tx.shape[1], reach)
        assert float(d.max()) < 1e-6


def test_draws_replay_the_entry_point_streams():
    """draw_params / draw_sigmas consume what the generators hand out next: replayed beside direct draws from the global generators"""
    torch.manual_seed(3)
    np.random.seed(3)
    ts, ns = torch.get_rng_state(), np.random.get_state()
    b = torch.empty(1).uniform_(0.8, 1.2)
    torch.empty(1).uniform_(0.8, 1.2), torch.empty(1).uniform_(0.8, 1.2)
    hu = torch.empty(1).uniform_(-0.2, 0.2) * 2 * math.pi
    perm = torch.randperm(4)
    assert torch.equal(SO.draw_params(1, 0.2, ts, end_state=True)[1], torch.get_rng_state())       # ... and leave the generator where they do
    prm = SO.draw_params(2, 0.2, ts)
    assert float(prm[0, 0]) == float(b) and float(prm[0, 3]) == float(hu) and prm[0, 4:].tolist() == perm.float().tolist()
    assert sorted(prm[1, 4:].tolist()) == [0.0, 1.0, 2.0, 3.0] and prm.dtype == torch.float32
    d = SO.draw_params(1, dict(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.5), ts)
    assert 0.0 <= float(d[0, 0]) <= 2.0 and abs(float(d[0, 3])) <= math.pi * (1 + 1e-6)
    s0, s1 = np.random.uniform(0.15, 1.15), np.random.uniform(0.15, 1.15)
    sig, reach, end = SO.draw_sigmas(2, ns, end_state=True)
    assert all(np.array_equal(a, b) for a, b in zip(end, np.random.get_state()))
    assert sig == [s0, s1] and reach == int(math.ceil(10 * max(s0, s1))) + 1
