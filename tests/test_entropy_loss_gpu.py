"""EntropyLoss kernels (csrc/entropy_loss.hip: MinEnt and max-squares on low-resolution logits) against the fp64 oracle
(tests/entropy_oracle.py) and against the executed reference (tests/golden/entropy_loss.npz, written by tests/golden/make_golden_entropy.py).

Bounds: the loss within 1e-5 relative of fp64; gradients per element |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref| (the per-link bound, DESIGN
section 7) against fp64 and against the reference's fp32.  For scale: the reference's own fp32 sits at most 1.5e-7 (loss) from fp64 and its
gradient at most 4e-7 absolute inside the bound (tests/test_entropy_cpu.py prints both).
The register form (C <= 8) and the class-loop form perform the same fp32 operations on the same values in the same order (the file is
compiled with contraction off), and no sum depends on a launch order: route, accumulate and run-to-run comparisons are bit for bit."""
import os

import numpy as np
import pytest
import torch

from entropy_oracle import entropy_loss, per_link_excess

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -7777.0
TYPES = ('entropy', 'max_square')
CASES = ('c6', 'c2', 'c11', 'c19', 'wide')


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'entropy_loss.npz'))


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


@pytest.fixture(scope='module')
def ref64(golden):
    """the fp64 oracle of every (case, type), computed once"""
    return {(c, t): entropy_loss(golden[c + '|logits'], t, float(golden[t + '|weights'][0])) for c in CASES for t in TYPES}


def run(ops, logits, kind, weight, **kw):
    z = logits if torch.is_tensor(logits) else torch.from_numpy(logits).to(DEV)
    loss = ops.softmax_entropy(z, kind, weight, generic=kw.get('generic', False))
    grad = ops.softmax_entropy_bwd_(torch.empty_like(z), z, kind, weight, accumulate=False, **kw)
    torch.cuda.synchronize()
    return loss, grad


@pytest.mark.parametrize('kind', TYPES)
@pytest.mark.parametrize('case', CASES)
def test_kernels_against_fp64_and_the_reference(ops, golden, ref64, case, kind):
    logits, weight = golden[case + '|logits'], float(golden[kind + '|weights'][0])
    loss64, grad64 = ref64[case, kind]
    loss, grad = run(ops, logits, kind, weight)
    assert loss.shape == (1,) and loss.dtype == torch.float32
    g = grad.cpu().numpy()
    ref32 = golden[f'{case}|{kind}|grad']
    rel = abs(float(loss) - loss64) / abs(loss64)
    ex64, ex32 = per_link_excess(g, grad64), per_link_excess(g, ref32)
    print(f'{case} {kind}: loss {float(loss):.8g} rel. error {rel:.2e} (bound 1e-5), vs the reference fp32 '
          f'{abs(float(loss) - float(golden[f"{case}|{kind}|loss"])) / abs(loss64):.2e}; gradient max |err| '
          f'{np.abs(g - grad64).max():.2e} of max |ref| {np.abs(grad64).max():.2e}, excess over the per-link bound {ex64:.2e} (fp64) {ex32:.2e} (fp32)')
    assert np.isfinite(float(loss)) and np.isfinite(g).all()
    assert rel <= 1e-5
    assert ex64 <= 0 and ex32 <= 0
    if case == 'wide':
        # probabilities that underflow: the reference's gradient is exactly 0 at these elements (and finite everywhere: the + 1e-30)
        zeros = ref32 == 0
        assert int(zeros.sum()) > 100
        print(f'wide {kind}: {int(zeros.sum())} exact zeros in the reference gradient, {int((g == 0).sum())} in the kernel\'s; '
              f'max |kernel| there {np.abs(g[zeros]).max():.2e}')
        assert float(np.abs(g[zeros]).max()) <= 1e-4 * float(np.abs(grad64).max())


@pytest.mark.parametrize('kind', TYPES)
def test_register_and_class_loop_forms_agree(ops, golden, kind):
    logits = golden['c6|logits']
    la, ga = run(ops, logits, kind, 0.7)
    lb, gb = run(ops, logits, kind, 0.7, generic=True)
    assert torch.equal(la, lb) and torch.equal(ga, gb)


@pytest.mark.parametrize('kind', TYPES)
def test_gradient_plumbing(ops, golden, kind):
    z = torch.from_numpy(golden['c19|logits']).to(DEV)
    _, g = run(ops, z, kind, 0.7)
    assert float(g.abs().max()) > 0
    onto_zeros = ops.softmax_entropy_bwd_(torch.zeros_like(z), z, kind, 0.7, accumulate=True)
    assert torch.equal(onto_zeros, g)
    base = torch.randn(z.shape, generator=torch.Generator().manual_seed(5)).to(DEV) * float(g.abs().max())
    acc = ops.softmax_entropy_bwd_(base.clone(), z, kind, 0.7, accumulate=True)
    assert torch.equal(acc, base + g)
    half = ops.softmax_entropy_bwd_(torch.empty_like(z), z, kind, 0.7, grad_scale=0.5, accumulate=False)
    assert torch.equal(half, g * 0.5)


@pytest.mark.parametrize('kind', TYPES)
def test_two_runs_are_bit_identical_without_deterministic_mode(ops, golden, kind):
    assert not ops.is_deterministic()
    z = torch.from_numpy(golden['c19|logits']).to(DEV)
    la, ga = run(ops, z, kind, 0.7)
    lb, gb = run(ops, z.clone(), kind, 0.7)
    assert torch.equal(la, lb) and torch.equal(ga, gb)


def test_offset_dense_views_and_canaries(ops, golden):
    """logits and gradient as dense views at odd offsets of larger buffers (4-byte aligned only): the values of the dense copies, and
    not a float outside the gradient view is written"""
    z = torch.from_numpy(golden['c19|logits']).to(DEV)
    n = z.numel()
    zbuf = torch.full((n + 64,), float('nan'), device=DEV)
    zv = zbuf[3:3 + n].view(z.shape)
    zv.copy_(z)
    for kind in TYPES:
        loss, g = run(ops, z, kind, 0.7)
        for lead, accumulate in ((5, False), (1, True)):
            gbuf = torch.full((lead + n + 37,), SENT, device=DEV)
            gv = gbuf[lead:lead + n].view(z.shape)
            assert zv.is_contiguous() and gv.is_contiguous() and zv.data_ptr() % 8 != 0 and gv.data_ptr() % 8 != 0
            if accumulate:
                gv.zero_()
            assert torch.equal(ops.softmax_entropy(zv, kind, 0.7), loss)
            ops.softmax_entropy_bwd_(gv, zv, kind, 0.7, accumulate=accumulate)
            torch.cuda.synchronize()
            assert torch.equal(gv, g)
            sent = torch.full((1,), SENT, device=DEV).view(torch.int32)
            outside = torch.cat([gbuf[:lead], gbuf[lead + n:]]).view(torch.int32)
            assert bool((outside == sent).all()), f'{kind}: floats outside the gradient view were written'


def test_strided_views_and_bad_arguments_are_refused(ops, golden):
    from pfst_amd._lib import PfstHipError
    z = torch.from_numpy(golden['c6|logits']).to(DEV)
    wide = torch.zeros(2, 8, 19, 17, device=DEV)
    for bad in (wide[:, 1:7], z[:, :, :, ::2], z.permute(0, 1, 3, 2)):
        assert not bad.is_contiguous()
        with pytest.raises(ValueError, match='dense'):
            ops.softmax_entropy(bad, 'entropy', 1.0)
        with pytest.raises(ValueError, match='dense'):
            ops.softmax_entropy_bwd_(torch.empty(bad.shape, device=DEV), bad, 'entropy', 1.0)
    with pytest.raises(ValueError, match='dense'):
        ops.softmax_entropy_bwd_(wide[:, 1:7], z, 'entropy', 1.0)
    with pytest.raises(ValueError, match='dense'):
        ops.softmax_entropy_bwd_(torch.empty(2, 6, 19, 18, device=DEV), z, 'entropy', 1.0)
    with pytest.raises(ValueError, match='kind'):
        ops.softmax_entropy(z, 'renyi', 1.0)
    one = torch.zeros(2, 1, 4, 4, device=DEV)
    with pytest.raises(PfstHipError, match='C >= 2'):           # log2(1) = 0: the reference's division by zero
        ops.softmax_entropy(one, 'entropy', 1.0)
    with pytest.raises(PfstHipError, match='C >= 2'):
        ops.softmax_entropy_bwd_(torch.empty_like(one), one, 'entropy', 1.0)
    with pytest.raises(PfstHipError):                           # above what the class loop supports
        ops.softmax_entropy(torch.zeros(1, 256, 2, 2, device=DEV), 'entropy', 1.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.softmax_entropy(z.cpu(), 'entropy', 1.0)
