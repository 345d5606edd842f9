"""The float64 references of tests/spatial_oracle.py against torch and against hand-written answers, and the conditions on the case tables of
tests/test_spatial_edges_gpu.py: the route mirrors send its launches to all four max-pool kernels and both axpy_ branches, the dyadic grids make
the sums they are used for exact, and no comparison leaves out a pixel but the constructed NaN rows of the softmax."""
import pytest
import torch
import torch.nn.functional as F

import spatial_oracle as O

NAN, INF = O.NAN, O.INF


def flat_to_tap(flat, H, W):
    """F.max_pool2d's flat input index of a window's winner -> its tap ty * 3 + tx"""
    Ho, Wo = flat.shape[2:]
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    return (flat // W - (2 * oy - 1)) * 3 + (flat % W - (2 * ox - 1))


# ---------------------------------------------------------------------------------------------------------------------------- max-pool
@pytest.mark.parametrize('H,W', O.POOL_SHAPES)
def test_maxpool_ref_is_torchs_pool_on_tie_free_inputs(H, W):
    n = O.PN * O.PC * H * W
    x = (torch.randperm(n, generator=O.g(H * 100 + W)).double().view(O.PN, O.PC, H, W) - n // 2).requires_grad_()          # no two values equal
    y, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    yr, tap = O.maxpool_ref(x.detach())
    assert tuple(yr.shape[2:]) == O.out_hw(H, W)
    assert torch.equal(yr, y.detach()) and torch.equal(tap, flat_to_tap(flat, H, W))
    dy = torch.randn(y.shape, generator=O.g(3)).double()
    y.backward(dy)
    assert torch.equal(O.maxpool_bwd_ref(dy, tap, (H, W)), x.grad)


def test_maxpool_ref_ties_and_nans_by_hand():
    x = torch.zeros(1, 1, 4, 4)
    y, tap = O.maxpool_ref(x)          # every window a tie: the first VALID tap
    assert tap[0, 0].tolist() == [[4, 3], [1, 0]] and bool((y == 0).all())
    x = torch.tensor([[1., 5., 2., 0.], [5., 0., 5., 0.], [0., 5., 5., 9.], [0., 0., 9., 1.]]).view(1, 1, 4, 4)
    y, tap = O.maxpool_ref(x)
    # window (0, 0): rows 0..1, cols 0..1 -> first 5 at (0, 1) = tap (1, 2) = 5; window (0, 1): cols 1..3 -> (0, 1) = tap (1, 0) = 3
    # window (1, 0): rows 1..3, cols 0..1 -> (1, 0) = tap (0, 1) = 1;           window (1, 1): rows 1..3, cols 1..3 -> first 9 at (2, 3) = tap (1, 2) = 5
    assert tap[0, 0].tolist() == [[5, 3], [1, 5]] and y[0, 0].tolist() == [[5., 5.], [5., 9.]]
    x = torch.full((1, 1, 3, 3), -INF)
    y, tap = O.maxpool_ref(x)
    assert tap[0, 0].tolist() == [[4, 3], [1, 0]] and bool((y == -INF).all())
    x = torch.arange(16.).view(1, 1, 4, 4)
    x[0, 0, 1, 1] = NAN
    x[0, 0, 3, 2] = NAN
    y, tap = O.maxpool_ref(x)          # (1, 1) is tap 8 of window (0, 0), 6 of (0, 1), 2 of (1, 0), 0 of (1, 1); (3, 2) is tap 7 of (1, 1): the last NaN
    assert tap[0, 0].tolist() == [[8, 6], [2, 7]] and bool(torch.isnan(y).all())
    # torch agrees on NaN propagation and, with one NaN per window, on the tap
    x = O.pool_inputs(8, 6)['NaN at tap 4 of window (1, 1)'].double()
    yt, flat = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    yr, tap = O.maxpool_ref(x)
    assert torch.equal(torch.isnan(yr), torch.isnan(yt)) and torch.equal(tap, flat_to_tap(flat, 8, 6))
    assert int(tap[0, 0, 1, 1]) == 4 and bool(torch.isnan(yr[:, :, 1, 1]).all())


def test_the_pool_case_table():
    assert O.POOL_SHAPES == [(1, 1), (1, 2), (2, 1), (3, 3), (2, 4), (4, 4), (2, 8), (5, 8), (8, 6), (6, 12), (17, 22), (72, 72)]
    assert O.out_hw(72, 72) == (36, 36) and 36 * 36 > 1024, 'one size past a grid pass of 1024-element plane blocks'
    assert [s for s in O.POOL_SHAPES if O.pool_eligible(*s)] == [(2, 4), (4, 4), (2, 8), (6, 12), (72, 72)]
    for H, W in O.POOL_SHAPES:
        fam = O.pool_inputs(H, W)
        assert len(fam) == (18 if O.has_interior(H, W) else 9)
        c = O.pool_case(H, W)
        assert c['x'].shape == (len(fam) * O.PN, O.PC, H, W)
        k = c['names'].index('two NaNs in a window') * O.PN
        # pixel (a, b) is tap (a + 1) * 3 + (b + 1) of window (0, 0)
        assert int(c['tap'][k, 0, 0, 0]) == 4 + 3 * min(1, H - 1) + min(1, W - 1), 'the last NaN of the window wins'
        if O.has_interior(H, W):
            assert int(c['tap'][k, 0, 1, 1]) == 8          # (3, 3) after (2, 1)
            for t in range(9):
                k = c['names'].index(f'NaN at tap {t} of window (1, 1)') * O.PN
                assert bool((c['tap'][k:k + O.PN, :, 1, 1] == t).all())
        k = c['names'].index('all -inf') * O.PN
        assert bool((c['tap'][k:k + O.PN, :, 0, 0] == 4).all()) and bool((c['y'][k:k + O.PN] == -INF).all())
        k = c['names'].index('columns constant') * O.PN
        if H > 1:
            assert bool((c['tap'][k:k + O.PN, :, 0] // 3 == 1).all()), 'ties between rows go to the first valid row'


def test_every_route_is_reached():
    fwd = {O.route_maxpool(H, W, 4 * dx, 4 * dy, di) for H, W in O.POOL_SHAPES for _, dx, dy, di in O.POOL_VIEWS}
    bwd = {O.route_maxpool_bwd(H, W, 4 * d) for H, W in O.POOL_SHAPES for _, d in O.BWD_VIEWS}
    assert fwd | bwd == O.POOL_ROUTES
    for H, W in O.POOL_SHAPES:
        routes = [O.route_maxpool(H, W, 4 * dx, 4 * dy, di) for _, dx, dy, di in O.POOL_VIEWS]
        assert routes == (['fwd pair'] + ['fwd generic'] * 3 if O.pool_eligible(H, W) else ['fwd generic'] * 4), 'each misalignment alone leaves the pair kernel'
        even = H % 2 == 0 and W % 2 == 0
        assert [O.route_maxpool_bwd(H, W, 4 * d) for _, d in O.BWD_VIEWS] == (['bwd 2x2', 'bwd generic'] if even else ['bwd generic'] * 2)
    assert O.route_maxpool(4, 4, 0, 8, 2) == 'fwd pair' and O.route_maxpool(4, 4, 8, 0, 0) == 'fwd generic'
    assert {O.route_axpy(4 * a, 4 * b) for a, b in O.AXPY_VIEWS} == O.AXPY_ROUTES
    assert [O.route_axpy(4 * a, 4 * b) for a, b in O.AXPY_VIEWS] == ['axpy float4'] + ['axpy scalar'] * 3
    assert sorted(n % 4 for n in O.AXPY_N[:4]) == [0, 1, 2, 3] and O.AXPY_N[4] // 4 > O.GRID_CAP and O.AXPY_N[4] % 4 == 3
    assert max(O.FILL_N) > O.GRID_CAP


def test_dyadic_grids_are_exact():
    for H, W in O.POOL_SHAPES:
        c = O.bnl_case(H, W)
        x = c['x']
        assert bool((x * 8 == (x * 8).round()).all()) and float(x.abs().max()) <= 4
        for coef, y, tap in c['coefs']:
            sc, sh = coef[:, 2], coef[:, 3]
            assert all(abs(float(s)) in (0.0, 0.25, 0.5, 1.0, 2.0) for s in sc) and bool((sh * 8 == (sh * 8).round()).all()) and float(sh.abs().max()) <= 4
            f32 = (x * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).clamp_min(0)          # two float32 roundings: equal only if both are exact
            assert torch.equal(f32.double(), O.bn_on_load_ref(x, coef))
            z = sc == 0
            if z.any():
                first = O.maxpool_ref(torch.zeros_like(x))[1]
                assert torch.equal(tap[:, z], first[:, z]), 'sc = 0: every tap equal, the first valid tap wins'
        assert any(bool((coef[:, 2] < 0).any()) for coef, _, _ in c['coefs']) and any(bool((coef[:, 2] == 0).any()) for coef, _, _ in c['coefs'])
    dy = O.dyadic((4, 3, 9, 9), 5, 2.0 ** -6, 8.0)
    assert float(dy.abs().max()) <= 8 and bool((dy * 64 == (dy * 64).round()).all())          # four terms: < 2^12 steps of 2^-6, exact in float32
    assert float(dy.abs().max()) * 64 * 64 < 2 ** 24, 'an 8 x 8 block of them sums exactly too (nearest up-sampling)'


# ------------------------------------------------------------------------------------------------------------------ nearest up-sampling
@pytest.mark.parametrize('hw,u', O.UPS_CASES)
def test_upsample_refs_are_torchs(hw, u):
    x = torch.randn(2, 3, *hw, generator=O.g(1)).double().requires_grad_()
    y = F.interpolate(x, scale_factor=u, mode='nearest')
    assert torch.equal(O.upsample_ref(x.detach(), u), y.detach())
    dy = torch.randn(y.shape, generator=O.g(2)).double()
    y.backward(dy)
    assert float((O.upsample_bwd_ref(dy, u) - x.grad).abs().max()) <= 1e-14 * u * u * float(dy.abs().max())


# -------------------------------------------------------------------------------------------------------------------- softmax, arg-max
@pytest.mark.parametrize('C', O.SM_C)
def test_torchs_float32_softmax_passes_the_assertion(C):
    worst = 0.0
    for HW in O.SM_HW:
        for fam in O.SM_FAMILIES:
            x = O.softmax_inputs(C, HW, fam)
            ref = O.softmax_reference(x)
            p = torch.softmax(x, 1)
            assert bool(torch.isfinite(ref['p']).all()) and bool(torch.isfinite(ref['bound']).all())
            r = O.softmax_ratio(p, ref)
            worst = max(worst, r)
            assert r < 1.0, (C, HW, fam, r)
            assert float((p.double().sum(1) - 1).abs().max()) <= C * O.U
            if fam == 'one class 120 below':
                assert C == 1 or (bool((p[:, C // 2] == 0).all()) and float(ref['zmax'].min()) > 100)
            if fam == '-inf classes' and C > 1:
                assert bool((p[:, 1::2] == 0).all()) and bool((ref['p'][:, 1::2] == 0).all())
        x, rows = O.softmax_special(C, HW)
        nan = torch.isnan(torch.softmax(x, 1))
        assert torch.equal(nan, rows.expand_as(nan)), 'the constructed rows, whole, and no other'
        assert int(rows.sum()) == 2
    print(f'C = {C}: torch float32 softmax at {worst:.3g} of the bound')


def test_argmax_ref():
    x = torch.tensor([[1., 3., 3., 2.], [NAN, 5., NAN, 0.], [0., INF, NAN, NAN], [-INF, -INF, -INF, -INF]]).t().reshape(1, 4, 4, 1)
    assert O.argmax_ref(x).flatten().tolist() == [1, 0, 2, 0]
    for C in O.AM_C:
        for HW in O.AM_HW:
            for fam in O.AM_FAMILIES:
                x = O.argmax_inputs(C, HW, fam)
                assert x.shape == (O.AM_N, C, HW, 1)
                assert torch.equal(O.argmax_ref(x), x.argmax(1)), 'torch.argmax: the first NaN, else the first maximum'
            x = O.argmax_inputs(C, HW, 'NaN classes')
            assert bool(torch.isnan(x).any(1).all())
            if C > 2:
                assert bool((O.argmax_ref(O.argmax_inputs(C, HW, 'NaN after +inf')) == C // 2).all())
        assert int(O.argmax_ref(O.argmax_inputs(C, 1025, 'NaN classes')).max()) == C - 1, 'a NaN in every class index, the last included'
        x, win = O.pair_ties(C)
        assert x.shape[2] % 4 == 0 and torch.equal(O.argmax_ref(x)[0, :, 0], win) and torch.equal(x.argmax(1)[0, :, 0], win)
        if C > 1:
            top = x.amax(1, keepdim=True)
            assert bool(((x == top).sum(1) == 2).all())
            pairs = {(int(a), int(b)) for a, b in zip(win, (x == top).long().cumsum(1).argmax(1)[0, :, 0])}
            assert len(pairs) == C * (C - 1) // 2, 'every pair of classes'


# ----------------------------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize('H,W', O.CANVASES)
def test_the_window_table(H, W):
    wins = O.windows(H, W)
    assert wins[-1] == (0, 0, H, W) and (H - 1, W - 1, 1, 1) in wins and any(hc * wc > 1024 for _, _, hc, wc in wins[:-1])
    assert all(y1 >= 0 and x1 >= 0 and y1 + hc <= H and x1 + wc <= W for y1, x1, hc, wc in wins)
    assert {(y1 == 0, x1 == 0, y1 + hc == H, x1 + wc == W) for y1, x1, hc, wc in wins} >= {(True, True, False, False), (True, False, False, True),
                                                                                        (False, True, True, False), (False, False, True, True)}
    assert all(y1 < 0 or x1 < 0 or y1 + hc > H or x1 + wc > W for y1, x1, hc, wc in O.refused_windows(H, W))
    c = O.window_case(H, W, 1)
    count = c['steps'][-2][1]
    assert int((count == 0).sum()) > 0 and float(count.max()) >= 3 and float(c['steps'][-1][1].min()) == 1
    assert bool(torch.isnan(c['steps'][-2][0] / count).any()), '0 / 0 at a pixel no window covered'
