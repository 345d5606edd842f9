"""Deterministic mode (pfst_set_deterministic) kernel by kernel against fp64 torch.  In that mode every launcher whose sum is normally completed by
atomic adds of several workgroups writes one partial per workgroup (per grid slice) into a scratch and a second kernel adds the slots in index
order (csrc/det.h, bn.hip, dwconv.hip, pfgst_loss.hip; the scratch table in api.cpp).  tests/test_deterministic_gpu.py checks that a whole
step is reproducible; here each launcher's deterministic path is held to the mathematics it computes, at shapes where that path has several
slices and a ragged last one.  Every case checks, in deterministic mode:
  1. the result against plain fp64 torch, at the bound the default-mode test of that kernel uses (tests/test_hip_ops.py and
     tests/test_pfgst_kernel_size_gpu.py);
  2. accumulation: an output that starts out nonzero ends as prefill + gradient (every reduce kernel ends in `+=`);
  3. two launches bit-identical, and a launch on a second stream (run after the first, then synchronised) bit-identical to them;
  4. the default (atomic) mode within 1e-6 relative of it;
  5. that the slice structure it claims is really reached: the split-K plan is asked of the library's own planner (ops.wgrad_split_k, held to
     the recorded table by tests/test_wgrad_split_k_cpu.py) with the arguments the launcher passes, and must be the one the case states;
     split_for is restated below.  If a heuristic changes, this fails instead of quietly covering a single slice."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from test_hip_ops import WINO_TOL, assert_close, g, ops, rel_err  # noqa: F401  (ops: the module fixture)
from test_pfgst_kernel_size_gpu import W4, labels, unfold

pytestmark = pytest.mark.gpu

DEV = 'cuda'
DET_VS_DEFAULT = 1e-6          # the bound tests/test_hip_ops.py::test_f16x3_gemm_and_wgrad_normalise_on_load holds the two modes to


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the slice structure the launchers choose
def rows_tile(m):
    """BM of the fp32 / bf16x6 / K-quad weight-gradient kernels: 128 above 64 output channels, 64 above 32, else 32"""
    return 128 if m > 64 else 64 if m > 32 else 32


def bn_splits(hw, c, n):
    """bn.hip split_for: ~2048 workgroups, at least 1024 elements of a plane per split, chunks of whole float4s -> (splits, chunk)"""
    splits = min(2048 // (c * n), (hw + 1023) // 1024)
    splits = max(splits, 1)
    chunk = (cdiv(hw, splits) + 3) & ~3
    return cdiv(hw, chunk), chunk


def assert_slices(chunks, chunk_len, P, ragged=True, want=None):
    """want: the (chunks, chunk_len) the case states"""
    assert want is None or (chunks, chunk_len) == want, f'the planner gives {chunks} chunks of {chunk_len} over {P} pixels, the case states {want}'
    assert chunks > 1, f'a single pixel chunk ({P} pixels): the multi-slice path is not reached'
    if ragged:
        assert P % chunk_len != 0, f'{chunks} chunks of {chunk_len} cover {P} pixels exactly: no ragged last chunk'


# ------------------------------------------------------------------------------------------------------------------------ the common checks
@contextlib.contextmanager
def det_mode(ops):
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(False)


def on_side_stream(fn):
    """fn() on a second stream, after everything queued before it and before anything after it (sequential, not concurrent)"""
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return out


def check_det(ops, launch, outs, what):
    """launch(inits) -> list of output tensors; inits: one fresh tensor per output (the accumulating outputs add into it).
    outs: [(name, fp64 reference of what the launch adds / writes, bound, accumulates)] -- accumulates: True (the output ends as its old
    contents + the reference), False (written: the old contents must not matter) or f(old contents, reference) -> the expected output;
    an optional fifth element replaces DET_VS_DEFAULT for that output"""
    zeros = lambda: [torch.zeros(o[1].shape, device=DEV) for o in outs]
    prefill = [(torch.randn(o[1].shape, generator=g(90 + i)) * float(o[1].abs().max())).to(DEV) for i, o in enumerate(outs)]
    with det_mode(ops):
        a = launch(zeros())
        b = launch(zeros())
        acc = launch([t.clone() for t in prefill])
        side = on_side_stream(lambda: launch(zeros()))
    d = launch(zeros())
    assert not ops.is_deterministic()
    for i, (name, ref, tol, accumulates, *mode_tol) in enumerate(outs):
        tag, mode_tol = f'{what} {name}', (mode_tol or [DET_VS_DEFAULT])[0]
        e_det, e_def, e_mode = rel_err(a[i], ref), rel_err(d[i], ref), rel_err(a[i], d[i])
        print(f'{tag}: det vs fp64 {e_det:.2e}  default vs fp64 {e_def:.2e}  det vs default {e_mode:.2e}')
        assert e_det < tol, f'{tag}: deterministic rel err {e_det:.3e} >= {tol}'
        assert torch.equal(a[i], b[i]), f'{tag}: two deterministic launches differ'
        assert torch.equal(a[i], side[i]), f'{tag}: the launch on a second stream differs'
        if accumulates:
            p64 = prefill[i].double().cpu()
            assert_close(acc[i], accumulates(p64, ref) if callable(accumulates) else p64 + ref, tol, f'{tag} accumulate')
        else:
            assert torch.equal(acc[i], a[i]), f'{tag}: an output that is written, not added to, depends on its old contents'
        assert e_mode <= mode_tol, f'{tag}: deterministic vs default {e_mode:.3e} > {mode_tol}'
    return a


def conv_operands(n, ci, co, H, W, k, s, d, p, seed=1):
    x = torch.randn(n, ci, H, W, generator=g(seed))
    ho, wo = (H + 2 * p - (k - 1) * d - 1) // s + 1, (W + 2 * p - (k - 1) * d - 1) // s + 1
    dy = torch.randn(n, co, ho, wo, generator=g(seed + 3))
    ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dy.double(), s, p, d)
    return x.to(DEV), dy.to(DEV), ref, ho * wo


# ------------------------------------------------------------------------------------------------------------------- split-K weight gradients
# (n, cin, cout, H, W, k, stride, dil, pad): the split-K plan in the comment and, as (chunks, chunk_len), in WGRAD_PLANS
WGRAD_CASES = [
    (3, 16, 16, 64, 80, 3, 1, 1, 1),       # K-quad 3x3 (W % 16 == 0): 9 chunks of 576 over 5120 pixels
    (3, 16, 192, 70, 68, 1, 1, 1, 0),      # K-quad 1x1: 9 chunks of 544 over 4760, two row tiles
    (3, 16, 16, 141, 129, 3, 2, 1, 1),     # generic kernel, stride 2: 9 chunks of 528 over 71 x 65
    (4, 16, 16, 80, 45, 3, 1, 1, 1),       # generic kernel, odd width: 7 chunks of 528 over 3600
]
WGRAD_PLANS = dict(zip(WGRAD_CASES, [(9, 576), (9, 544), (9, 528), (7, 528)]))


@pytest.mark.parametrize('case', WGRAD_CASES)
def test_conv_wgrad(ops, case):
    n, ci, co, H, W, k, s, d, p = case
    x, dy, ref, P = conv_operands(*case)
    quad = s == 1 and ops.wgrad_q_operands_ok(x, dy) and ((k == 1 and P % 4 == 0) or (k == 3 and W % 16 == 0 and d <= 8))
    tiles = cdiv(ci * k * k, 128) * cdiv(co, rows_tile(co))
    if quad:        # conv_wgrad_q.hip launch_q: 16-deep K-steps, 4 workgroups per CU
        ch, cl = ops.wgrad_split_k(tiles * n, P, 256 * 4, 16)
    else:           # conv_mfma.hip launch_wgrad_k: 16-deep steps (4 per CU) for 3x3, 32 (2 per CU) for 1x1; N * chunks is gridDim.z
        ch, cl = ops.wgrad_split_k(tiles * n, P, 256 * (4 if k == 3 else 2), 16 if k == 3 else 32, chunk_cap=65535 // n)
    assert quad == (case in WGRAD_CASES[:2])
    assert_slices(ch, cl, P, want=WGRAD_PLANS[case])
    check_det(ops, lambda o: [ops.conv_wgrad_(o[0], x, dy, k, s, d, p)], [('dw', ref, 5e-5, True)], f'wgrad {"quad" if quad else "generic"}')


@pytest.mark.parametrize('case', [(3, 16, 192, 70, 52, 1, 1, 1, 0), (1, 16, 32, 50, 47, 3, 1, 1, 1)])
def test_conv_wgrad_split(ops, case):
    """bf16x6: 1x1 on the K-quad split kernel (launch_wgrad_split_q, 7 chunks of 528 over 3640), 3x3 on launch_wgrad_split (the doubling rule:
    4 chunks of 592 over 2350)"""
    n, ci, co, H, W, k, s, d, p = case
    x, dy, ref, P = conv_operands(*case)
    tiles = cdiv(ci * k * k, 128) * cdiv(co, rows_tile(co))
    ch, cl = ops.wgrad_split_k(tiles * n, P, 256 * 3, 16) if k == 1 else ops.wgrad_split_k(tiles * n, P, doubling=True)
    assert_slices(ch, cl, P, want=(7, 528) if k == 1 else (4, 592))
    check_det(ops, lambda o: [ops.conv_wgrad_split_(o[0], x, dy, k, s, d, p)], [('dw', ref, 3e-6, True)], f'split wgrad {k}x{k}')


@pytest.mark.parametrize('bnl', [False, True])
@pytest.mark.parametrize('case', [(2, 16, 256, 70, 52), (3, 16, 96, 70, 68)])
def test_conv_wgrad_f16x3(ops, case, bnl):
    """the whole-line f16x3 1x1 weight gradient: the 256-row tile (M % 256 == 0: 7 chunks of 528 over 3640) and the 128-row one (9 chunks of
    544 over 4760); bnl: x is the PRE-normalisation tensor, normalised on load"""
    n, ci, co, H, W = case
    P = H * W
    big = co % 256 == 0
    ch, cl = ops.wgrad_split_k(cdiv(ci, 128) * cdiv(co, 256 if big else 128) * n, P, 256 if big else 512, 16)
    assert_slices(ch, cl, P, want=(7, 528) if big else (9, 544))
    dy = torch.randn(n, co, H, W, generator=g(4)).to(DEV)
    if bnl:
        pre = (torch.randn(n, ci, H, W, generator=g(1)) * 1.5).to(DEV)
        gamma, beta = (torch.randn(ci, generator=g(3)) * 0.8).to(DEV), (torch.randn(ci, generator=g(5)) * 0.5).to(DEV)
        mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
        xa = ops.amax_slots(DEV)
        x = ops.bn_apply(pre, mean, invstd, gamma, beta, True, amax=xa)          # what the kernel normalises the rows of `pre` to
        src = pre
    else:
        x = torch.randn(n, ci, H, W, generator=g(1)).to(DEV)
        xa, coef, src = ops.absmax(x), None, x
    ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (co, ci, 1, 1), dy.double().cpu(), 1, 0, 1)
    da = ops.absmax(dy)
    check_det(ops, lambda o: [ops.conv_wgrad_f16x3_(o[0], src, dy, xa, da, bnl=coef)], [('dw', ref, 3e-6, True)],
              f'f16x3 wgrad M={co} bnl={bnl}')


@pytest.mark.parametrize('dil', [1, 2])
def test_conv_wgrad_f16q(ops, dil):
    """the f16x3 K-quad weight gradient of direct 3x3 layers (launch_q16): 9 chunks of 576 over 64 x 80"""
    case = (3, 16, 16, 64, 80, 3, 1, dil, dil)
    n, ci, co, H, W, k = case[:6]
    x, dy, ref, P = conv_operands(*case)
    ch, cl = ops.wgrad_split_k(cdiv(ci * 9, 128) * cdiv(co, rows_tile(co)) * n, P, 256 * 4, 16)
    assert_slices(ch, cl, P, want=(9, 576))
    xa, da = ops.absmax(x), ops.absmax(dy)
    check_det(ops, lambda o: [ops.conv_wgrad_f16q_(o[0], x, dy, xa, da, 3, dil)], [('dw', ref, 3e-6, True)], f'f16x3 quad wgrad dil={dil}')


@pytest.mark.parametrize('split', [0, 1, 2])
@pytest.mark.parametrize('m', [2, 4])
def test_wino_wgrad(ops, m, split):
    """the grouped transform-domain products of the Winograd weight gradient: (m+2)^2 groups of N * chunks slices each, dU of group xi at
    xi * Cout * Cin (dw_gs) -- fp32 K-quad (split 0), bf16x6 (1), f16x3 on pre-split operands (2).  2 x 16 -> 96 channels at 160 x 160:
    T = 6400 (m = 2) / 1600 (m = 4) tiles per image, 3 ... 12 chunks with a ragged last one: at m = 2, 11 chunks of 592 (split 0 and 1) and
    12 of 544 (split 2); at m = 4, 3 chunks of 544."""
    n, ci, co, H, W, d = 2, 16, 96, 160, 160, 1
    nx, T = (m + 2) ** 2, ops.wino_tiles(H, W, d, m)
    if split == 2:          # pfst_wgrad_f16x3_launch (packed operands); co % 256 != 0: the 128-row tile, 2 per CU
        ch, cl = ops.wgrad_split_k(cdiv(ci, 128) * cdiv(co, 128) * nx * n, T, 512, 16)
    else:                   # pfst_wgrad_q_launch (1x1 over the tile index) / pfst_wgrad_split_q_launch
        ch, cl = ops.wgrad_split_k(cdiv(ci, 128) * cdiv(co, rows_tile(co)) * nx * n, T, 1024 if split == 0 else 768, 16)
    assert_slices(ch, cl, T, want=(3, 544) if m == 4 else (12, 544) if split == 2 else (11, 592))
    x = torch.randn(n, ci, H, W, generator=g(1)).to(DEV)
    dy = torch.randn(n, co, H, W, generator=g(4)).to(DEV)
    ref = torch.nn.grad.conv2d_weight(x.double().cpu(), (co, ci, 3, 3), dy.double().cpu(), 1, d, d)

    def launch(o):
        ops.wino_wgrad_(o[0], x, dy, d, m=m, split=split)
        u = ops._wino_ws(x.device, 'U', nx * co * ci)[:nx * co * ci]       # the det reduce's output (the per-stream buffer may be larger)
        return [o[0], u.clone()]

    # dU (written, not added to: pfst_wino_wgrad zeroes it) has no fp64 reference of its own here: check_det holds it to itself (bit-identical
    # across launches and streams) and the default mode within 1e-6 of it -- dU is what the fixed-order reduce writes.  dw = G^T dU G (the
    # same element-wise kernel in both modes) amplifies dU's rounding as it amplifies everything else: F(4x4)'s fp64 bound is 10x F(2x2)'s
    # (WINO_TOL), and so is the bound on its mode difference (measured on dw: 2-3e-7 at m = 2, 1.8-2.3e-6 at m = 4; on dU: 2e-7)
    with det_mode(ops):
        u_det = launch([torch.zeros(co, ci, 3, 3, device=DEV)])[1].double().cpu()
    check_det(ops, launch, [('dw', ref, 2 * WINO_TOL[m], True, DET_VS_DEFAULT * WINO_TOL[m] / WINO_TOL[2]), ('dU', u_det, 1e-6, False)],
              f'wino wgrad m={m} split={split}')


# ------------------------------------------------------------------------------------------------------------------------------ bias gradient
def test_bias_grad(ops):
    """deterministic mode: one launch per image, one workgroup per channel -- N = 3 ordered writers per db[c], HW = 72 x 65 > 4096"""
    n, c, H, W = 3, 40, 72, 65
    dy = torch.randn(n, c, H, W, generator=g(4))
    dyd = dy.to(DEV)
    check_det(ops, lambda o: [ops.bias_grad_(o[0], dyd)], [('db', dy.double().sum((0, 2, 3)), 1e-5, True)], 'bias grad')


# ------------------------------------------------------------------------------------------------------------------------------ BatchNorm
BN_CASES = [((2, 8, 64, 64), True), ((2, 8, 63, 65), False)]      # 4 splits of 1024 per plane (vector path); 4 of 1024 over 4095 (scalar)


def bn_reference(x, r, gamma, beta, dy, relu, res):
    xr, gr, br = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    rr = r.double().requires_grad_() if res else None
    y = F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5)
    if res:
        y = y + rr
    if relu:
        y = F.relu(y)
    y.backward(dy.double())
    return y.detach(), xr.grad, gr.grad, br.grad, (rr.grad if res else None)


@pytest.mark.parametrize('shape,vec', BN_CASES)
def test_bn_stats(ops, shape, vec):
    n, c, h, w = shape
    sp, chunk = bn_splits(h * w, c, n)
    assert sp > 1 and (vec or (h * w) % chunk != 0)
    x = torch.randn(shape, generator=g(1)) * 2 + 0.5
    xd = x.to(DEV)
    xx = x.double()
    mean, var = xx.mean((0, 2, 3)), xx.var((0, 2, 3), unbiased=False)
    cnt = n * h * w

    def launch(o):
        rm, rv = o[2], o[3] + 1.0            # running statistics: updated in place with momentum 0.1 (rv starts at 1 + prefill)
        m, i = ops.bn_stats(xd, rm, rv, 0.1, 1e-5)
        return [m, i, rm, rv - 1.0]

    momentum = lambda old, new: 0.9 * old + new          # running <- 0.9 running + 0.1 batch statistic
    check_det(ops, launch, [('mean', mean, 1e-5, False), ('invstd', 1.0 / torch.sqrt(var + 1e-5), 1e-5, False),
                            ('running_mean', 0.1 * mean, 1e-5, momentum), ('running_var', 0.1 * (var * cnt / (cnt - 1) - 1.0), 1e-5, momentum)],
              f'bn_stats {shape}')


@pytest.mark.parametrize('shape,vec,mask', [BN_CASES[0] + (False,), BN_CASES[0] + (True,), BN_CASES[1] + (False,)])
def test_bn_backward(ops, shape, vec, mask):
    """vector path (HW % 4 == 0, with the ReLU gate from bn_apply's bitmask or from y) and scalar path (gate from y: the bitmask needs
    HW % 256 == 0); residual branch with dres accumulated; dgamma / dbeta / dres add into nonzero buffers"""
    n, c, h, w = shape
    sp, chunk = bn_splits(h * w, c, n)
    assert sp > 1 and (vec or (h * w) % chunk != 0)
    x = torch.randn(shape, generator=g(1)) * 2 + 0.5
    r = torch.randn(shape, generator=g(2))
    gamma, beta = torch.rand(c, generator=g(3)) + 0.5, torch.randn(c, generator=g(4))
    dy = torch.randn(shape, generator=g(5))
    _, dx_ref, dg_ref, db_ref, dr_ref = bn_reference(x, r, gamma, beta, dy, True, True)
    xd, rd, gd, bd, dyd = (t.to(DEV) for t in (x, r, gamma, beta, dy))
    with det_mode(ops):
        mean, invstd = ops.bn_stats(xd)
        y, bits = ops.bn_apply(xd, mean, invstd, gd, bd, True, rd, want_mask=True)
    assert (bits is not None) == vec

    def launch(o):
        dx = ops.bn_backward(dyd, None if mask else y, xd, mean, invstd, gd, o[1], o[2], True, o[3], dres_accumulate=True, beta=bd,
                             mask=bits if mask else None)
        return [dx, o[1], o[2], o[3]]

    check_det(ops, launch, [('dx', dx_ref, 1e-4, False), ('dgamma', dg_ref, 1e-4, True), ('dbeta', db_ref, 1e-4, True),
                            ('dres', dr_ref, 1e-6, True)], f'bn_backward {shape} mask={mask}')


@pytest.mark.parametrize('shape,vec', BN_CASES)
def test_bn_backward_sums(ops, shape, vec):
    """the reduction half alone (no fused partials): dgamma / dbeta += the sums, and the record's m1 = mean(dz), m2 = mean(dz * xhat)"""
    n, c, h, w = shape
    x = torch.randn(shape, generator=g(1)) * 2 + 0.5
    gamma, beta = torch.rand(c, generator=g(3)) + 0.5, torch.randn(c, generator=g(4))
    dy = torch.randn(shape, generator=g(5))
    y, _, dg_ref, db_ref, _ = bn_reference(x, x, gamma, beta, dy, True, False)
    dz = dy.double() * (y > 0)
    xhat = (x.double() - x.double().mean((0, 2, 3), keepdim=True)) / torch.sqrt(x.double().var((0, 2, 3), unbiased=False, keepdim=True) + 1e-5)
    m1, m2 = dz.mean((0, 2, 3)), (dz * xhat).mean((0, 2, 3))
    xd, gd, bd, dyd = (t.to(DEV) for t in (x, gamma, beta, dy))
    with det_mode(ops):
        mean, invstd = ops.bn_stats(xd)

    def launch(o):
        rec = ops.bn_backward_sums(dyd, xd, mean, invstd, gd, bd, o[0], o[1])
        d = rec.view(c, ops.BN_BWD_REC_BYTES)[:, :16].contiguous().view(torch.float64)      # (m1, m2) doubles at the front of each record
        return [o[0], o[1], d[:, 0].clone(), d[:, 1].clone()]

    check_det(ops, launch, [('dgamma', dg_ref, 1e-4, True), ('dbeta', db_ref, 1e-4, True), ('m1', m1, 1e-4, False), ('m2', m2, 1e-4, False)],
              f'bn_backward_sums {shape}')


def test_bn_backward_dual_refuses_deterministic_mode(ops):
    """the two-layer BatchNorm backward has no fixed-order reduction: in deterministic mode the wrapper returns None (the caller runs the layers
    one by one) and the entry point itself refuses"""
    from pfst_amd._lib import PfstHipError
    n, c, h, w = 2, 8, 16, 16
    dy = torch.randn(n, c, h, w, device=DEV)
    x = torch.randn(n, c, h, w, device=DEV)
    one, zero = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    mean, invstd = ops.bn_stats(x)
    _, bits = ops.bn_apply(x, mean, invstd, one, zero, True, torch.zeros_like(x), want_mask=True)
    side = lambda: dict(x=x, mean=mean, invstd=invstd, gamma=one, dgamma=torch.zeros(c, device=DEV), dbeta=torch.zeros(c, device=DEV), amax=None)
    assert ops.bn_backward_dual(dy, bits, side(), side()) is not None          # the default mode takes this case
    dxa, dxb = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(4 * c, dtype=torch.float64, device=DEV)
    with det_mode(ops):
        assert ops.bn_backward_dual(dy, bits, side(), side()) is None
        with pytest.raises(PfstHipError, match='default \\(atomic\\) reductions'):
            ops.call('pfst_bn_backward_dual', dy.data_ptr(), x.stride(0), bits.data_ptr(),
                     x.data_ptr(), x.stride(0), mean.data_ptr(), invstd.data_ptr(), one.data_ptr(), dxa.data_ptr(), x.stride(0), 0, 0,
                     ws.data_ptr(), 0, 0, 0,
                     x.data_ptr(), x.stride(0), mean.data_ptr(), invstd.data_ptr(), one.data_ptr(), dxb.data_ptr(), x.stride(0), 0, 0,
                     ws[2 * c:].data_ptr(), 0, n, c, h * w, torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------------------ depthwise
# (dil, H, W): the plane kernel (whole plane in LDS, W % 4 == 0: modes 3 / 1 / 2 = dilation 1 / % 4 / other; one slot per image) and the
# strip kernel (planes above 64 KiB: cdiv(H, rows) strips per image, one slot per strip and image; mode 0 = W % 4 != 0, scalar taps)
DW_CASES = [(1, 16, 20, 'plane'), (12, 32, 32, 'plane'), (2, 24, 32, 'plane'), (2, 7, 9, 'strip'),
            (1, 136, 128, 'strip'), (4, 130, 132, 'strip'), (2, 132, 128, 'strip'), (3, 131, 130, 'strip')]


def dw_strips(H, W, dil):
    """dwconv.hip strip_rows: the rows of a strip that fit 64 KiB of LDS with their halo -> strips per image"""
    if H * W * 4 <= 64 * 1024:
        return 1
    rows = max(64 * 1024 // (W * 4) - 2 * dil, 1)
    return cdiv(H, min(rows, H))


@pytest.mark.parametrize('dil,H,W,kernel', DW_CASES)
def test_dwconv_bwd_and_wgrad(ops, dil, H, W, kernel):
    n, c = 2, 24
    vec = W % 4 == 0
    plane = vec and H * W * 4 <= 64 * 1024
    assert plane == (kernel == 'plane')
    assert n * (1 if plane else dw_strips(H, W, dil)) > 1          # det_T: one slot per image (plane), per strip and image (strip kernel)
    if H * W * 4 > 64 * 1024:
        assert dw_strips(H, W, dil) > 1
    x = torch.randn(n, c, H, W, generator=g(1))
    w = torch.randn(c, 1, 3, 3, generator=g(2))
    dy = torch.randn(n, c, H, W, generator=g(3))
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), 1, dil, dil, c)
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), 1, dil, dil, c)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)

    def fused(o):
        ops.dwconv_bwd_(o[0], xd, dyd, wd, dil, o[1], accumulate=True)
        return [o[0], o[1]]

    check_det(ops, fused, [('dw', dw_ref, 1e-4, True), ('dx', dx_ref, 1e-5, True)], f'dwconv_bwd dil={dil} {H}x{W} {kernel}')
    check_det(ops, lambda o: [ops.dwconv_wgrad_(o[0], xd, dyd, dil)], [('dw', dw_ref, 1e-4, True)], f'dwconv_wgrad dil={dil} {H}x{W}')


@pytest.mark.parametrize('bnb', [False, True])
@pytest.mark.parametrize('H,W,dils', [(16, 16, (36,)), (24, 40, (4, 8)), (32, 32, (12, 24, 36))])
def test_dwconv_multi_bwd(ops, H, W, dils, bnb):
    """the ASPP branches' backward in one pass: every branch's weight gradient through [C][N][9] slots; bnb: each dy is the gradient of that
    branch's BatchNorm + ReLU output, the BatchNorm backward applied while staging (reference: fp64 autograd through batch_norm + relu)"""
    n, c, k = 2, 20, len(dils)
    x = torch.randn(n, c, H, W, generator=g(1))
    ws = [torch.randn(c, 1, 3, 3, generator=g(2 + i)) for i in range(k)]
    dys = [torch.randn(n, c, H, W, generator=g(7 + i)) for i in range(k)]
    xd, wd, dyd = x.to(DEV), [w.to(DEV) for w in ws], [t.to(DEV) for t in dys]
    assert ops.dwconv_multi_ok(xd, list(dils))
    grads, bn = dys, None
    if bnb:
        gam = [torch.rand(c, generator=g(30 + i)) + 0.5 for i in range(k)]
        bet = [torch.randn(c, generator=g(40 + i)) * 0.3 for i in range(k)]
        pres = [ops.dwconv(xd, wd[i], dils[i]) for i in range(k)]
        with det_mode(ops):
            recs = []
            for i in range(k):
                mean, invstd = ops.bn_stats(pres[i])
                recs.append(ops.bn_backward_sums(dyd[i], pres[i], mean, invstd, gam[i].to(DEV), bet[i].to(DEV), None, None))
        bn = [(pres[i], recs[i]) for i in range(k)]
        grads = [bn_reference(pres[i].cpu(), pres[i].cpu(), gam[i], bet[i], dys[i], True, False)[1] for i in range(k)]
    outs = [(f'dw[{i}]', torch.nn.grad.conv2d_weight(x.double(), ws[i].shape, grads[i].double(), 1, d, d, c), 1e-4, True)
            for i, d in enumerate(dils)]
    dx_ref = sum(torch.nn.grad.conv2d_input(x.shape, ws[i].double(), grads[i].double(), 1, d, d, c) for i, d in enumerate(dils))
    outs.append(('dx', dx_ref, 1e-5, False))

    def launch(o):
        dx = torch.empty_like(xd)
        ops.dwconv_multi_bwd_(o[:k], xd, dyd, wd, list(dils), dx, bnb=bn)
        return o[:k] + [dx]

    check_det(ops, launch, outs, f'dwconv_multi_bwd {dils} bnb={bnb}')


# ------------------------------------------------------------------------------------------------------------------ PFGSTLoss source statistics
@pytest.mark.parametrize('K,d', [(3, 1), (5, 2), (7, 3)])
def test_src_sim_losses(ops, K, d):
    """the six source sums as gxs * N fp64 slots (22 x 26 pixels: 3 pixel blocks x 2 images), for mean_std, margin2 and src_perc, at each
    kernel size of the one K x K kernel family; the inputs of tests/test_pfgst_kernel_size_gpu.py::test_source_target_and_cross_prob_k_against_torch"""
    gen = torch.Generator().manual_seed(100 + K * 10 + d)
    n, H, W = 2, 22, 26
    assert cdiv(H * W, 256) * n > 1
    gt, _ = labels(n, H, W, 7 * K + d)
    gt8 = ops.to_u8(gt.to(DEV))
    N = n * K * K * H * W
    sim = (torch.randperm(N, generator=gen).double() / N * 2 - 1).view(n, K * K, H, W)
    gl = F.interpolate(gt.float(), size=(H, W), mode='nearest')
    nb, ctr, vs = unfold(gl.double(), K, d).squeeze(1), gl.expand(n, K * K, H, W), (gl != 255).expand(n, K * K, H, W)
    simd = sim.float().to(DEV)
    for lt_name, perc in (('mean_std', None), ('margin2', None), ('mean_std', 0.4)):
        s = sim.clone().requires_grad_()
        pos, neg = s[(nb == ctr) & vs], s[(nb != ctr) & vs]
        if perc is not None:
            pos, neg = pos.sort()[0][:int(pos.numel() * perc)], neg.sort(descending=True)[0][:int(neg.numel() * perc)]
        if lt_name == 'mean_std':
            want = torch.stack([-pos.mean() * W4[0], neg.mean() * W4[1], pos.std() * W4[2], neg.std() * W4[3]])
        else:
            want = torch.stack([(F.relu(0.7 - pos) ** 2).mean() * W4[0], (F.relu(neg - 0.2) ** 2).mean() * W4[1]])
        want.sum().backward()
        nl = want.numel()

        def launch(o, lt_name=lt_name, perc=perc, nl=nl):
            losses, gsim = ops.src_sim_losses(simd, gt8, d, *W4, loss_type=lt_name, margin=(0.7, 0.2), src_perc=perc, ksize=K)
            return [losses[:nl], gsim]

        check_det(ops, launch, [('losses', want.detach(), 1e-5, False), ('gsim', s.grad, 1e-5, False)], f'src_sim K={K} {lt_name} perc={perc}')


# ------------------------------------------------------------------------------------------------------------- the scratch table (api.cpp)
def _small_wgrad():
    x = torch.randn(1, 16, 16, 16, generator=g(1)).to(DEV)
    dy = torch.randn(1, 32, 16, 16, generator=g(4)).to(DEV)
    return x, dy, torch.nn.grad.conv2d_weight(x.double().cpu(), (32, 16, 3, 3), dy.double().cpu(), 1, 1, 1)


def test_det_scratch_on_more_streams_than_table_slots(ops):
    """The scratch table has 8 slots keyed by (device, stream); a det launch on a stream beyond them takes the least recently used slot over.
    Ten fresh streams, one weight gradient on each, then a second pass over all ten (evictions on every launch): every result bit-identical to
    the current stream's.  (The device half of the key needs a second GPU to be told apart from the stream half: not covered here.)"""
    x, dy, ref = _small_wgrad()
    with det_mode(ops):
        base = ops.conv_wgrad_(torch.zeros(32, 16, 3, 3, device=DEV), x, dy, 3, 1, 1, 1)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(10)]
        assert len({s.cuda_stream for s in streams} | {torch.cuda.current_stream().cuda_stream}) == 11
        for rnd in range(2):
            for i, s in enumerate(streams):
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    out = ops.conv_wgrad_(torch.zeros(32, 16, 3, 3, device=DEV), x, dy, 3, 1, 1, 1)
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                assert torch.equal(out, base), f'pass {rnd}, stream {i}'
    assert_close(base, ref, 5e-5, 'wgrad')


def test_det_scratch_regrowth(ops):
    """On one stream: a small det launch, a large one (its scratch outgrows the 8 MiB first allocation: the regrowth path synchronises the
    device and frees the old buffer), a small one again -- all correct.  The stream's slot is first pushed out of the 8-slot table by launches
    on eight other streams, so that it starts empty whatever ran on it before."""
    xs, dys, ref_s = _small_wgrad()
    n, ci, co, H, W = 2, 128, 256, 48, 64
    xl, dyl, ref_l, P = conv_operands(n, ci, co, H, W, 3, 1, 1, 1)
    assert ops.wgrad_q_operands_ok(xl, dyl)
    ch, cl = ops.wgrad_split_k(cdiv(ci * 9, 128) * cdiv(co, 128) * n, P, 256 * 4, 16)
    assert 4 * co * ci * 9 * n * ch > 8 << 20, 'the large launch must outgrow the first scratch allocation'
    streams = [torch.cuda.Stream() for _ in range(9)]
    assert len({s.cuda_stream for s in streams}) == 9
    target = streams[0]
    with det_mode(ops):
        for s in streams[1:] + [target]:
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                if s is target:
                    a = ops.conv_wgrad_(torch.zeros(32, 16, 3, 3, device=DEV), xs, dys, 3, 1, 1, 1)
                    b = ops.conv_wgrad_(torch.zeros(co, ci, 3, 3, device=DEV), xl, dyl, 3, 1, 1, 1)
                    c = ops.conv_wgrad_(torch.zeros(32, 16, 3, 3, device=DEV), xs, dys, 3, 1, 1, 1)
                else:
                    ops.conv_wgrad_(torch.zeros(32, 16, 3, 3, device=DEV), xs, dys, 3, 1, 1, 1)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
    assert_close(a, ref_s, 5e-5, 'small before')
    assert_close(b, ref_l, 5e-5, 'large (regrown scratch)')
    assert torch.equal(a, c), 'small after the regrowth'
