"""The data gradient of an f16x3 Winograd layer from the weight gradient's transform dM = A dY A^T (layers.WINO_SHARE_DY): pfst_wino_dy once,
pfst_wino_gemm_f16x3 with the transposed forward filter sets, pfst_wino_dx (B P B^T per tile, overlap-added as a gather).  Checked against
the fp64 direct data gradient with the metric and bound of test_hip_ops.py::test_winograd_on_the_f16x3_gemm, and against the route it
replaces (the flipped-filter pipeline on B^T dY B)."""
import pytest
import torch

from test_hip_ops import WINO_TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = WINO_TOL[4]

# n, Cout (channels of dy), Cin (channels of dx), H, W, dilation
SHAPES = {
    1: (2, 64, 128, 8, 8, 1),         # 2 x 2 tiles: every tile touches the border
    2: (2, 64, 128, 12, 20, 1),       # non-square, no multiple of a workgroup's strip
    3: (2, 64, 128, 40, 40, 1),       # 10 x 10 tiles: every kind of neighbour inside ONE workgroup (100 <= 256 tiles: a single strip)
    4: (2, 64, 128, 10, 14, 1),       # partial tiles in both directions (3 x 4 tiles of a 10 x 14 plane)
    5: (2, 64, 128, 24, 24, 2),       # four 12 x 12 sub-grids
    6: (2, 128, 128, 16, 16, 1),      # the in-model case
    # more than 256 tiles per sub-grid row group: several workgroups per plane, the rims of tiles OUTSIDE a workgroup formed from P
    7: (2, 64, 128, 64, 72, 1),       # 16 x 18 tiles: strips of 14 + 2 tile rows (rim rows and corners across the strip border)
    8: (2, 64, 128, 108, 40, 1),      # 27 x 10 tiles: strips of 25 + 2 rows
    9: (2, 64, 128, 8, 1040, 1),      # 2 x 260 tiles: 256 + 4 columns, one tile row per workgroup (rim columns, rows and corners)
    10: (1, 64, 128, 4, 1048, 2),     # dilation 2, 2 x 131 interleaved columns = 256 + 6: the column neighbour is two threads away
}
STRIPS = {7: 2, 8: 2, 9: 4, 10: 4}    # workgroups per image and channel (pfst_wino_dx_slots) of the multi-workgroup shapes
MULTI = sorted(STRIPS)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from pfst_amd import hip_ops
    return hip_ops


def g(seed=0):
    return torch.Generator().manual_seed(seed)


_cases = {}


def case(ops, k):
    """operands, the fp64 reference and both packed filter images of shape k, made once"""
    if k not in _cases:
        n, co, ci, H, W, d = SHAPES[k]
        w = torch.randn(co, ci, 3, 3, generator=g(2)) * 0.1
        dy = torch.randn(n, co, H, W, generator=g(4)) * 1e-5
        ref = torch.nn.grad.conv2d_input((n, ci, H, W), w.double(), dy.double(), 1, d, d)
        wd = w.to(DEV)
        _, ut, _, at = ops.wino_pack_weight_f16(wd, False, True, shared_dy=True)
        _, ud, _, ad = ops.wino_pack_weight_f16(wd, False, True)
        _cases[k] = dict(dy=dy.to(DEV), ref=ref, ut=ut, at=at, ud=ud, ad=ad)
    return _cases[k]


def new_route(ops, k, **kw):
    n, co, ci, H, W, d = SHAPES[k]
    c = case(ops, k)
    dm, dm_amax = ops.wino_dy(c['dy'], d)
    return ops.wino_dgrad_shared(dm, dm_amax, c['ut'], c['at'], n, co, ci, (H, W), d, **kw)


@pytest.mark.parametrize('k', sorted(SHAPES))
def test_shared_dy_data_gradient_vs_fp64_and_the_flipped_filter_route(ops, k):
    n, co, ci, H, W, d = SHAPES[k]
    assert ops.wino_tiles(H, W, d) > 0            # (every plane here is one pfst_wino_tiles accepts: shape 4 runs with partial tiles)
    c = case(ops, k)
    assert ops.wino_dx_slots(H, W, d) == STRIPS.get(k, d), 'the shape no longer tiles into the workgroups it was chosen for'
    dx = new_route(ops, k)
    old = ops.wino_conv(c['dy'], c['ud'], ci, d, u_amax=c['ad'])
    from test_hip_ops import rel_err
    print(f'shape {k}: new vs fp64 {rel_err(dx, c["ref"]):.3e}  old vs fp64 {rel_err(old, c["ref"]):.3e}  new vs old {rel_err(dx, old):.3e}')
    assert_close(dx, c['ref'], TOL, 'shared-dM dgrad vs fp64')
    assert_close(dx, old, 2 * TOL, 'shared-dM dgrad vs the flipped-filter route')


@pytest.mark.parametrize('k', [2, 5] + MULTI)
def test_accumulate_into_a_prefilled_gradient(ops, k):
    c = case(ops, k)
    out = c['ref'].float().to(DEV)
    res = new_route(ops, k, out=out, accumulate=True)
    assert res.data_ptr() == out.data_ptr()
    assert_close(out, 2 * c['ref'], TOL, 'accumulate')


@pytest.mark.parametrize('k', [2, 5, 7, 9])
def test_channel_slice_output_leaves_its_neighbours_alone(ops, k):
    n, co, ci, H, W, d = SHAPES[k]
    c = case(ops, k)
    big = torch.full((n, ci + 24, H, W), 7.0, device=DEV)
    new_route(ops, k, out=big[:, 8:8 + ci])
    assert_close(big[:, 8:8 + ci], c['ref'], TOL, 'slice')
    assert bool((big[:, :8] == 7.0).all()) and bool((big[:, 8 + ci:] == 7.0).all()), 'canary channels were written'


@pytest.mark.parametrize('k,acc,relu', [(2, False, True), (5, True, False), (7, True, True), (8, False, False), (9, False, True), (10, True, True)])
def test_wino_dx_emits_the_bn_backward_sums(ops, k, acc, relu):
    """pfst_wino_dx(bnb_x): the partials summed by pfst_bn_backward(bwd_partials) give the dx / dgamma / dbeta of the call that runs its own
    reduction pass, within the bounds test_bn_backward_fused_gpu.py sets for the pfst_wino_output partials"""
    from test_bn_backward_fused_gpu import rel
    n, co, c, h, w, dil = SHAPES[k]
    gen = g(c + co + h)
    pre = (torch.randn(n, c, h, w, generator=gen) * 1.7 + 0.8).to(DEV)
    gamma = (0.6 + 0.8 * torch.rand(c, generator=gen)).to(DEV)
    beta = (0.3 * torch.randn(c, generator=gen)).to(DEV)
    wc = (torch.randn(co, c, 3, 3, generator=gen) * (2.0 / (c * 9)) ** 0.5).to(DEV)
    dyc = torch.randn(n, co, h, w, generator=gen).to(DEV)
    old = torch.randn(n, c, h, w, generator=gen).to(DEV) if acc else None
    mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
    _, ut, _, at = ops.wino_pack_weight_f16(wc, False, True, shared_dy=True)
    dm, dm_amax = ops.wino_dy(dyc, dil)
    args = (dm, dm_amax, ut, at, n, co, c, (h, w), dil)
    plain = ops.wino_dgrad_shared(*args, out=old.clone() if acc else None, accumulate=acc)
    fused, part, slots = ops.wino_dgrad_shared(*args, out=old.clone() if acc else None, accumulate=acc, bnb=(pre, coef, relu))
    assert slots == n * ops.wino_dx_slots(h, w, dil) and part.numel() == 2 * c * slots
    assert torch.equal(fused, plain)
    outs = []
    for p, s in ((None, 0), (part, slots)):
        dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
        dx = ops.bn_backward(plain, None, pre, mean, invstd, gamma, dg, db, relu=relu, beta=beta, partials=p, slots=s)
        outs.append((dx, dg, db))
    for a, b, what in zip(outs[1], outs[0], ('dx', 'dgamma', 'dbeta')):
        print(what, rel(a, b))
        assert rel(a, b) < 2e-6, (what, rel(a, b))


@pytest.mark.parametrize('k', [3, 5] + MULTI)
def test_wino_dx_is_bitwise_reproducible(ops, k):
    """no atomics, one summation order per pixel: two runs on the same P agree bit for bit, in and out of deterministic mode"""
    n, co, ci, H, W, d = SHAPES[k]
    c = case(ops, k)
    t = ops.wino_tiles(H, W, d)
    dm, dm_amax = ops.wino_dy(c['dy'], d)
    p = torch.empty(36 * n * ci * t, device=DEV)
    ops.call('pfst_wino_gemm_f16x3', dm.data_ptr(), c['ut'].data_ptr(), c['at'].data_ptr(), dm_amax.data_ptr(), p.data_ptr(), n, co, ci, t, 4, 1,
             torch.cuda.current_stream().cuda_stream)
    was = ops.is_deterministic()
    runs = []
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            runs += [ops.wino_dx(p, ci, (H, W), d, n), ops.wino_dx(p, ci, (H, W), d, n)]
    finally:
        ops.set_deterministic(was)
    assert_close(runs[0], c['ref'], TOL, 'wino_dx')
    assert all(torch.equal(runs[0], r) for r in runs[1:])


@pytest.mark.parametrize('hw', [16, 10])
def test_conv_backward_shares_one_transform_of_dy(ops, hw):
    """Conv2dP(128, 128, 3) at 2 x 128 x 16 x 16 through layers.conv_backward with WINO_SHARE_DY on and off: the same dx and dw, and with the
    switch on one pfst_wino_dy, no pfst_wino_input on dy, one pfst_wino_dx.
    10 x 10: 9 tiles, no whole tile quads -- the weight gradient leaves the transform domain (wgrad_route), the layer's data gradient
    still takes the route its packed filter image was made for, with a dM of its own"""
    from pfst_amd import layers
    from pfst_amd.engine import Var
    n, c = 2, 128
    shared_wgrad = ops.wino_tiles(hw, hw, 1) % 4 == 0
    assert shared_wgrad == (hw == 16)
    x = torch.randn(n, c, hw, hw, generator=g(1)).to(DEV)
    dy = (torch.randn(n, c, hw, hw, generator=g(4)) * 1e-5).to(DEV)
    prev = layers.CONV_MATH, layers.WINO_SHARE_DY
    layers.CONV_MATH = 'f16x3'
    conv = layers.Conv2dP(c, c, 3, padding=1).to(DEV)
    inner, got = ops.call, {}
    try:
        for share in (True, False):
            layers.WINO_SHARE_DY = share
            conv.repack(True)
            assert conv.wino_f16 and conv.wino_dx == share and (conv.wgrad_route(hw, hw) == 'wino_f16x3') == shared_wgrad
            conv.weight.grad = torch.zeros_like(conv.weight)
            xv = Var(x, True)
            conv.fprop(x, keep=True)
            log = []

            def counting(name, *a):
                log.append((name, a[0]))
                return inner(name, *a)
            ops.call = counting
            try:
                layers.conv_backward(xv, conv, dy, conv.saved_v)
                layers.join_side_stream()
                torch.cuda.synchronize()
            finally:
                ops.call = inner
            names = [name for name, _ in log]
            on_dy = [name for name, first in log if name == 'pfst_wino_input' and first == dy.data_ptr()]
            assert names.count('pfst_wino_wgrad') == int(shared_wgrad), names
            if share:
                assert names.count('pfst_wino_dy') == 1 and names.count('pfst_wino_dx') == 1 and not on_dy, names
                assert 'pfst_wino_output' not in names
            else:
                assert names.count('pfst_wino_dy') == int(shared_wgrad) and names.count('pfst_wino_dx') == 0 and len(on_dy) == 1, names
            got[share] = (xv.grad.clone(), conv.weight.grad.clone())
    finally:
        layers.CONV_MATH, layers.WINO_SHARE_DY = prev
    dx_ref = torch.nn.grad.conv2d_input(x.shape, conv.weight.detach().double().cpu(), dy.double().cpu(), 1, 1, 1)
    assert_close(got[True][0], dx_ref, TOL, 'dx, switch on')
    assert_close(got[True][0], got[False][0], 2 * TOL, 'dx on vs off')
    assert_close(got[True][1], got[False][1], 2 * TOL, 'dw on vs off')


def test_batched_packing_writes_the_shared_image_and_drops_the_flipped_sets(ops):
    """WeightBatch on one layer with the switch off, then on: `ud` and its maxima equal the per-layer packing's under either setting, and a
    layer that moves onto the shared route gives up its resident flipped plain sets (`pd`)"""
    from pfst_amd import layers
    prev = layers.CONV_MATH, layers.WINO_SHARE_DY
    layers.CONV_MATH = 'f16x3'
    try:
        conv = layers.Conv2dP(128, 128, 3, padding=1).to(DEV)
        batch = layers.WeightBatch()
        for share in (False, True):
            layers.WINO_SHARE_DY = share
            batch.begin()
            conv.repack(True, batch)
            batch.flush()
            assert conv.wino_dx == share and (conv.pd is None) == share and conv.pf is not None
            uf, ud, af, ad = ops.wino_pack_weight_f16(conv.weight.data, True, True, shared_dy=share)
            assert torch.equal(conv.uf, uf) and torch.equal(conv.ud, ud)
            groups = lambda t: t.view(-1, ops.AMAX_SUB).max(dim=1).values
            assert torch.equal(groups(conv.uf_amax), groups(af)) and torch.equal(groups(conv.ud_amax), groups(ad))
            assert (conv.ud_amax.data_ptr() == conv.uf_amax.data_ptr()) == share
    finally:
        layers.CONV_MATH, layers.WINO_SHARE_DY = prev
