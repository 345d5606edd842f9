"""The kernels of the adversarial (ADVENT) baseline -- csrc/adv_conv.hip (4x4 / stride-2 / padding-1 convolutions: forward with fused
LeakyReLU, data gradient with the gate of the layer below, weight + bias gradient; the mean / L1 tail) and the per-class entropy map of
csrc/entropy_loss.hip -- each against fp64 torch on the CPU (tests/advent_oracle.py).

Bounds (the project's): a loss within 1e-5 relative; per element |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref|.
The moved class walk (csrc/entropy_walk.h) must leave pfst_softmax_entropy_* unchanged: their results on the golden entropy_loss.npz inputs
are compared bit for bit with values recorded from the build before the move (tests/golden/advent_entropy_parent.json)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import advent_oracle as orc
from advent_oracle import per_link_excess

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -7777.0
SLOPE = 0.2
# (Cin, Cout, H, W, N): first layer with odd sizes; 19 classes; whole MFMA tiles; ragged pixels; channels that are no multiple of the tile;
# the last layer (one output channel: the direct forward kernel) with a 1x1 output, and with odd sizes and channels that are no multiple of
# 16; and the smallest layer whose weight gradient splits its output pixels over two chunks per image (SPLIT)
SPLIT = (64, 128, 66, 66, 3)
CONV_CASES = [(6, 8, 37, 45, 2), (19, 64, 33, 32, 1), (64, 128, 16, 16, 3), (128, 256, 7, 9, 2), (72, 136, 10, 6, 1), (512, 1, 2, 2, 2), (40, 1, 9, 7, 2), SPLIT]
IDS = ['x'.join(map(str, c)) for c in CONV_CASES]


def test_the_split_case_splits(ops):
    """the weight gradient's launcher plans with (tiles * N workgroups, Ho * Wo pixels, 512 slots, K-step 16, at most 65535 / N chunks): a
    split needs >= 512 pixels per chunk and enough workgroups for the planner's 2 % rule to prefer it.  SPLIT: 8 column tiles x 1 row tile x 3
    images over 33 x 33 = 1089 pixels -> two chunks of 560, the second ragged (529 pixels, no multiple of the K-step); every other case: one"""
    for cin, cout, h, w, n in CONV_CASES:
        tiles = -(-cin * 16 // 128) * -(-cout // (128 if cout > 64 else 64 if cout > 32 else 32))
        plan = ops.wgrad_split_k(tiles * n, (h // 2) * (w // 2), 512, 16, 65535 // n)
        assert plan == ((2, 560) if (cin, cout, h, w, n) == SPLIT else (1, plan[1])), (cin, cout, h, w, n, plan)


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


@pytest.fixture(scope='module')
def conv_data():
    """per case: fp64 inputs and the fp64 references, computed once and never modified"""
    out = {}
    for idx, (cin, cout, h, w, n) in enumerate(CONV_CASES):
        g = torch.Generator().manual_seed(100 + idx)
        x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
        x = torch.where(x > 0, x, SLOPE * x)                       # a LeakyReLU output, as the layers below produce it
        x.view(-1)[::7] = 0.0                                       # pre-activations of exactly 0 planted: the gate there is the slope
        wt = torch.randn(cout, cin, 4, 4, generator=g, dtype=torch.float64) / (cin * 16) ** 0.5
        b = torch.randn(cout, generator=g, dtype=torch.float64)
        if cout > 1:
            wt[cout // 2] = 0.0                                     # a channel whose pre-activation is exactly 0 everywhere
            b[cout // 2] = 0.0
        x, wt, b = x.float().double(), wt.float().double(), b.float().double()
        pre = F.conv2d(x, wt, b, stride=2, padding=1)
        dy = torch.randn(pre.shape, generator=g, dtype=torch.float64).float().double()
        xr = x.clone().requires_grad_(True)
        wr, br = wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
        (F.conv2d(xr, wr, br, stride=2, padding=1) * dy).sum().backward()
        gate = torch.where(x > 0, torch.ones_like(x), torch.full_like(x, SLOPE))
        out[cin, cout, h, w, n] = dict(x=x, w=wt, b=b, pre=pre, act=F.leaky_relu(pre, SLOPE), dy=dy, dx=xr.grad, dx_gated=xr.grad * gate,
                                       dw=wr.grad, db=br.grad)
    return out


def dev32(t):
    return t.float().to(DEV).contiguous()


def guarded(shape, fill=SENT):
    """a dense tensor of `shape` at the front of a flat buffer with 257 canary floats behind it"""
    n = int(np.prod(shape))
    flat = torch.full((n + 257,), fill, device=DEV)
    return flat, flat[:n].view(shape)


def canaries_intact(flat, n, what):
    sent = torch.full((1,), SENT, device=DEV).view(torch.int32)
    assert bool((flat[n:].view(torch.int32) == sent).all()), f'{what}: floats behind the output were written'


def check(got, ref, what):
    g = got.detach().cpu().numpy()
    ex = per_link_excess(g, ref.numpy())
    print(f'{what}: max |err| {np.abs(g - ref.numpy()).max():.3e} of max |ref| {float(ref.abs().max()):.3e}, excess over the per-link bound {ex:.3e}')
    assert np.isfinite(g).all()
    assert ex <= 0, what


@pytest.mark.parametrize('case', CONV_CASES, ids=IDS)
def test_conv_forward(ops, conv_data, case):
    d = conv_data[case]
    x, w, b = dev32(d['x']), dev32(d['w']), dev32(d['b'])
    for slope, ref in ((None, d['pre']), (SLOPE, d['act'])):
        flat, y = guarded(ref.shape)
        ops.adv_conv(x, w, b, slope=slope, out=y)
        torch.cuda.synchronize()
        check(y, ref, f'forward {case} slope {slope}')
        canaries_intact(flat, y.numel(), f'forward {case}')
        if case[1] > 1:
            assert bool((y[:, case[1] // 2] == 0).all())            # pre-activation exactly 0 -> exactly 0 either way
    nb = ops.adv_conv(x, w, None)
    check(nb, d['pre'] - d['b'].view(1, -1, 1, 1), f'forward {case} without bias')


@pytest.mark.parametrize('case', CONV_CASES, ids=IDS)
def test_conv_data_gradient(ops, conv_data, case):
    d = conv_data[case]
    x, w, dy = dev32(d['x']), dev32(d['w']), dev32(d['dy'])
    results = {}
    for gate, ref in ((None, d['dx']), (x, d['dx_gated'])):
        flat, dx = guarded(x.shape)
        ops.adv_conv_dgrad_(dx, dy, w, x_gate=gate, slope=SLOPE, accumulate=False)
        torch.cuda.synchronize()
        check(dx, ref, f'data gradient {case} gate {gate is not None}')        # every element written: a canary left inside would fail here
        canaries_intact(flat, dx.numel(), f'data gradient {case}')
        results[gate is not None] = dx.clone()
    # the gate at a planted 0 is the slope
    zero = x == 0
    assert int(zero.sum()) > 0
    assert torch.equal(results[True][zero], results[False][zero] * SLOPE)
    # accumulate adds exactly what a store writes, and two runs agree bit for bit
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    acc = ops.adv_conv_dgrad_(base.clone(), dy, w, x_gate=x, slope=SLOPE, accumulate=True)
    assert torch.equal(acc, base + results[True])
    again = ops.adv_conv_dgrad_(torch.empty_like(x), dy, w, x_gate=x, slope=SLOPE, accumulate=False)
    assert torch.equal(again, results[True])


@pytest.mark.parametrize('case', CONV_CASES, ids=IDS)
def test_conv_weight_and_bias_gradient(ops, conv_data, case):
    d = conv_data[case]
    x, dy = dev32(d['x']), dev32(d['dy'])
    fw, dw = guarded(d['dw'].shape, 0.0)
    fb, db = guarded(d['db'].shape, 0.0)
    fw[dw.numel():] = SENT
    fb[db.numel():] = SENT
    ops.adv_conv_wgrad_(dw, db, x, dy)
    torch.cuda.synchronize()
    check(dw, d['dw'], f'weight gradient {case}')
    check(db, d['db'], f'bias gradient {case}')
    canaries_intact(fw, dw.numel(), f'weight gradient {case}')
    canaries_intact(fb, db.numel(), f'bias gradient {case}')
    only_w = ops.adv_conv_wgrad_(torch.zeros_like(dw), None, x, dy)
    check(only_w, d['dw'], f'weight gradient {case} without bias gradient')


@pytest.mark.parametrize('case', CONV_CASES, ids=IDS)
def test_deterministic_mode_gradients_are_bit_identical_and_accumulate_exactly(ops, conv_data, case):
    d = conv_data[case]
    x, w, dy = dev32(d['x']), dev32(d['w']), dev32(d['dy'])
    assert not ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        runs = []
        for _ in range(2):
            dw, db = torch.zeros(d['dw'].shape, device=DEV), torch.zeros(d['db'].shape, device=DEV)
            ops.adv_conv_wgrad_(dw, db, x, dy)
            dx = ops.adv_conv_dgrad_(torch.empty_like(x), dy, w, x_gate=x, slope=SLOPE)
            runs.append((dw, db, dx))
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        check(runs[0][0], d['dw'], f'deterministic weight gradient {case}')
        check(runs[0][1], d['db'], f'deterministic bias gradient {case}')
        gen = torch.Generator().manual_seed(9)
        bw, bb = torch.randn(d['dw'].shape, generator=gen).to(DEV), torch.randn(d['db'].shape, generator=gen).to(DEV)
        aw, ab = bw.clone(), bb.clone()
        ops.adv_conv_wgrad_(aw, ab, x, dy)
        assert torch.equal(aw, bw + runs[0][0])                   # the ordered sum is added once: exactly what landed on zeros
    finally:
        ops.set_deterministic(False)


def test_conv_refusals(ops):
    x = torch.zeros(1, 6, 8, 8, device=DEV)
    w = torch.zeros(4, 6, 4, 4, device=DEV)
    with pytest.raises(ValueError, match='4, 4'):
        ops.adv_conv(x, torch.zeros(4, 6, 3, 3, device=DEV))
    with pytest.raises(ValueError, match='4, 4'):
        ops.adv_conv(torch.zeros(1, 6, 1, 8, device=DEV), w)
    with pytest.raises(ValueError, match='contiguous'):
        ops.adv_conv(torch.zeros(1, 6, 8, 16, device=DEV)[:, :, :, ::2], w)
    with pytest.raises(ValueError, match='bias'):
        ops.adv_conv(x, w, torch.zeros(5, device=DEV))
    with pytest.raises(ValueError, match='dy'):
        ops.adv_conv_dgrad_(torch.empty_like(x), torch.zeros(1, 4, 3, 4, device=DEV), w)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.adv_conv(x.cpu(), w)
    # more output channels than the bias gradient takes: refused before anything is added to dw
    from pfst_amd._lib import PfstHipError
    dw = torch.zeros(65536, 1, 4, 4, device=DEV)
    with pytest.raises(PfstHipError, match='pfst_adv_conv_wgrad failed'):
        ops.adv_conv_wgrad_(dw, torch.zeros(65536, device=DEV), torch.ones(1, 1, 2, 2, device=DEV), torch.ones(1, 65536, 1, 1, device=DEV))
    torch.cuda.synchronize()
    assert not bool(dw.any())


@pytest.mark.parametrize('n,hw,label', [(2, 1, 0.0), (3, 35, 1.0), (2, 1000, 0.0)])
def test_tail(ops, n, hw, label):
    g = torch.Generator().manual_seed(n * 1000 + hw)
    y = (torch.randn(n, 1, hw, 1, generator=g) + 0.3)
    if hw == 35:
        y[1] = 1.0                                                  # d_n == label exactly: sign(0) = 0
    y64 = y.double().requires_grad_(True)
    d64 = y64.mean(dim=(1, 2, 3))
    loss64 = 0.37 * (d64 - label).abs().mean()
    loss64.backward()
    d, loss, gy = ops.adv_tail(y.to(DEV), label, 0.37)
    torch.cuda.synchronize()
    rel = abs(float(loss) - float(loss64.detach())) / abs(float(loss64.detach()))
    print(f'tail n {n} hw {hw}: loss {float(loss):.8g} rel. error {rel:.2e}')
    assert rel <= 1e-5
    check(d, d64.detach(), 'tail d')
    check(gy, y64.grad, 'tail gradient')
    if hw == 35:
        assert bool((gy[1] == 0).all())
    half = ops.adv_tail(y.to(DEV), label, 0.37, grad_scale=0.5)[2]
    assert torch.equal(half, gy * 0.5)
    assert ops.adv_tail(y.to(DEV), label, 0.37, want_grad=False)[2] is None


# ---------------------------------------------------------------- the entropy map
ENT_C = (2, 6, 8, 9, 19)
ENT_HW = ((5, 7), (37, 41))


@pytest.fixture(scope='module')
def ent_data():
    out = {}
    for c in ENT_C:
        for h, w in ENT_HW:
            g = torch.Generator().manual_seed(c * 100 + h)
            z = (torch.randn(2, c, h, w, generator=g) * 2.0).double()
            ge = torch.randn(2, c, h, w, generator=g).double()
            zr = z.clone().requires_grad_(True)
            e = orc.entropy_map_graph(zr)
            (e * ge).sum().backward()
            out[c, h, w] = dict(z=z, ge=ge, e=e.detach(), dz=zr.grad)
    return out


@pytest.mark.parametrize('hw', ENT_HW, ids=['5x7', '37x41'])
@pytest.mark.parametrize('c', ENT_C)
def test_entropy_map_forward_and_backward(ops, ent_data, c, hw):
    d = ent_data[(c,) + hw]
    z, ge = dev32(d['z']), dev32(d['ge'])
    flat, e = guarded(z.shape)
    ops.entropy_map(z, out=e)
    torch.cuda.synchronize()
    check(e, d['e'], f'entropy map C {c} {hw}')
    canaries_intact(flat, e.numel(), 'entropy map')
    flat, dz = guarded(z.shape)
    ops.entropy_map_bwd_(dz, z, ge, accumulate=False)
    torch.cuda.synchronize()
    check(dz, d['dz'], f'entropy map backward C {c} {hw}')
    canaries_intact(flat, dz.numel(), 'entropy map backward')
    base = torch.randn(z.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    acc = ops.entropy_map_bwd_(base.clone(), z, ge, accumulate=True)
    assert torch.equal(acc, base + dz)
    if c <= 8:                                                      # the register form and the class loop: the same bits
        assert torch.equal(ops.entropy_map(z, generic=True), e)
        assert torch.equal(ops.entropy_map_bwd_(torch.empty_like(z), z, ge, accumulate=False, generic=True), dz)


def test_entropy_map_wide_logits_backward_is_finite_and_zero_where_the_reference_is():
    from pfst_amd import hip_ops as ops
    g = torch.Generator().manual_seed(11)
    z = torch.randn(2, 6, 37, 45, generator=g) * 40.0               # probabilities underflow to exactly 0 in fp32
    ge = torch.randn(2, 6, 37, 45, generator=g)
    zr = z.clone().requires_grad_(True)
    p = torch.softmax(zr, dim=1)
    e32 = -(p * torch.log2(p + 1e-30)) / np.log2(6)                 # the reference's expression in its own precision
    (e32 * ge).sum().backward()
    ref32 = zr.grad
    zeros = ref32 == 0
    assert int(zeros.sum()) > 100 and bool(torch.isfinite(ref32).all())
    zd = z.to(DEV)
    dz = ops.entropy_map_bwd_(torch.empty_like(zd), zd, ge.to(DEV), accumulate=False).cpu()
    e = ops.entropy_map(zd).cpu()
    assert bool(torch.isfinite(dz).all()) and bool(torch.isfinite(e).all())
    print(f'wide: {int(zeros.sum())} exact zeros in the reference gradient, max |kernel| there {float(dz[zeros].abs().max()):.2e}')
    assert bool((dz[zeros] == 0).all())
    zr64 = z.double().requires_grad_(True)
    (orc.entropy_map_graph(zr64) * ge.double()).sum().backward()
    check(dz, zr64.grad, 'wide entropy map backward')
    check(e, orc.entropy_map(z), 'wide entropy map')


def test_entropy_map_refusals(ops):
    from pfst_amd._lib import PfstHipError
    z = torch.zeros(2, 6, 9, 8, device=DEV)
    with pytest.raises(ValueError, match='dense'):
        ops.entropy_map(z[:, :, :, ::2])
    with pytest.raises(ValueError, match='dense'):
        ops.entropy_map_bwd_(torch.empty(2, 6, 9, 9, device=DEV), z, z)
    with pytest.raises(PfstHipError, match='pfst_entropy_map failed'):                 # one class: log2(1) = 0 would divide by zero
        ops.entropy_map(torch.zeros(2, 1, 4, 4, device=DEV))
    with pytest.raises(PfstHipError, match='pfst_entropy_map_bwd failed'):
        ops.entropy_map_bwd_(torch.zeros(2, 1, 4, 4, device=DEV), torch.zeros(2, 1, 4, 4, device=DEV), torch.zeros(2, 1, 4, 4, device=DEV))


# ---------------------------------------------------------------- the moved class walk leaves EntropyLoss's kernels as they were
def entropy_loss_record(ops, golden):
    """{case|kind: [loss bits, sha256 of the gradient's bytes, the same for the class-loop form]} of pfst_softmax_entropy_fwd / _bwd"""
    rec = {}
    for case in ('c6', 'c2', 'c11', 'c19', 'wide'):
        z = torch.from_numpy(golden[case + '|logits']).to(DEV)
        for kind in ('entropy', 'max_square'):
            row = []
            for generic in (False, True):
                loss = ops.softmax_entropy(z, kind, 0.7, generic=generic)
                grad = ops.softmax_entropy_bwd_(torch.empty_like(z), z, kind, 0.7, accumulate=False, generic=generic)
                row += [int(loss.view(torch.int32).item()), hashlib.sha256(grad.cpu().numpy().tobytes()).hexdigest()]
            rec[f'{case}|{kind}'] = row
    return rec


def test_entropy_loss_kernels_unchanged_by_the_shared_class_walk(ops, golden_dir):
    golden = np.load(os.path.join(golden_dir, 'entropy_loss.npz'))
    with open(os.path.join(golden_dir, 'advent_entropy_parent.json')) as f:
        want = json.load(f)
    got = entropy_loss_record(ops, golden)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], f'{k}: pfst_softmax_entropy_* no longer produce the bits they produced before entropy_walk.h'
