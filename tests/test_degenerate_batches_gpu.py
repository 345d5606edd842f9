"""Degenerate batches on the GPU: empty pair sets, all-ignored labels, zero operands.

Remote-sensing tiles produce batches that are all no-data, all one class, or without a pixel above the pseudo-label threshold.  The guards
that keep such a batch from putting NaN into the weights are exercised here, each against a plain fp64 restatement or the CPU oracle:

 1. whole PFGST / supervised train steps on degenerate label maps against the oracle, with the backward pass at amax == 0;
 2. the kernels behind them on the boundary inputs: target losses at valid counts 0 .. 3, source losses on empty / one-element /
    zero-variance sets, cosine similarity at zero-norm pixels, fused cross-entropy with nothing to average, the f16x3 arithmetic with zero
    and tiny operands.

The documented deviation from the reference: where the reference returns NaN -- the mean of
an empty source pair set, the unbiased std of a one-element set, the gradient of the std of a zero-variance set (pfgst_loss.py:107-131) --
this implementation returns exactly 0 and sends exactly 0 into the gradient."""
import functools
import math
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import to_dev
from test_pfgst_kernel_size_gpu import labels, ops, rel_err, t_sim, t_valid, unfold  # noqa: F401  (`ops` is the fixture)
from test_train_step_gpu import TOL, _build, conv_math  # noqa: F401  (`conv_math` is the fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
W4 = (0.1, 0.2, 0.3, 0.4)
SRC_NAN_ALL = {'loss_src_pos_mean', 'loss_src_neg_mean', 'loss_src_pos_std', 'loss_src_neg_std'}
ACC_TOL = 100.0 * 10 / (2 * 128 * 128)          # tests/test_train_step_gpu.py: ten arg-max flips of the 32768 pixels


def all_zero(t):
    return int((t != 0).sum()) == 0


def assert_close(a, b, tol, what):
    """max |a - b| / max |b|, printed before it is asserted: rel_err of tests/test_pfgst_kernel_size_gpu.py without the 1e-12 it adds to the
    denominator, which would swallow the references of order 1e-30 used here.  The reference must not be all zero."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert float(b.abs().max()) > 0
    e = float((a - b).abs().max() / b.abs().max())
    print(f'{what}: rel err {e:.3e} (bound {tol})')
    assert e < tol, f'{what} rel err {e:.3e} >= {tol}'


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------- 1. whole train steps
def _all_255(gt):
    gt[:] = 255


def _all_class_0(gt):
    gt[:] = 0


def _one_labelled_pixel(gt):
    gt[:] = 255
    gt[0, 0, 64, 64] = 3            # on the stride-8 nearest-neighbour lattice of the 16 x 16 loss grid: exactly one positive pair


def _one_image_255(gt):
    gt[0] = 255


def _unchanged(gt):
    pass


# name: (label edit, pseudo threshold, the oracle's NaN keys, the oracle's n_conf).  The NaN sets and counts were computed on the CPU with
# oracle.OraclePFGST.train_step (seeded_pfgst_state(O, 9), synth_batch(2, 128, 6, seed=55), Python / NumPy seed 4); the test asserts them.
# 'confident': the threshold is the 0.75 quantile of the teacher's maximum probability on this batch (0.170 .. 0.276), 'none_confident'
# the same batch at a threshold no probability reaches.
SCENARIOS = {
    'all_255': (_all_255, 0.30, SRC_NAN_ALL, 0),
    'all_class_0': (_all_class_0, 0.30, {'loss_src_neg_mean', 'loss_src_neg_std'}, 0),
    'one_labelled_pixel': (_one_labelled_pixel, 0.30, {'loss_src_pos_std'}, 0),
    'one_image_255': (_one_image_255, 0.30, set(), 0),
    'confident': (_unchanged, 0.211, set(), 7955),
    'none_confident': (_unchanged, 1.1, set(), 0),
}


@functools.lru_cache(maxsize=None)
def oracle_step(name):
    """the oracle's step on scenario `name`, computed once per session -> (batch, log values, extras, the student before the step)"""
    from oracle import pfst_oracle as O
    from helpers import seeded_pfgst_state
    from pfst_amd.synthetic import synth_batch
    edit, threshold, _, _ = SCENARIOS[name]
    _, student, teacher = seeded_pfgst_state(O, 9)
    batch = synth_batch(2, 128, 6, seed=55)
    edit(batch['gt_semantic_seg'])
    oracle = O.OraclePFGST(student, pseudo_threshold=threshold, teacher_sd=teacher)
    random.seed(4); np.random.seed(4)
    olog, ex = oracle.train_step(batch, return_extras=True)
    return batch, olog, ex, student


def run_scenario(name):
    """one PFGST.train_step on scenario `name` beside the oracle, with the assertions every scenario shares -> (model, log_vars, student)"""
    _, threshold, nan_keys, n_conf = SCENARIOS[name]
    batch, olog, ex, student = oracle_step(name)
    assert {k for k, v in olog.items() if math.isnan(v)} == nan_keys
    assert ex['n_conf'] == n_conf
    model, opt, _, _ = _build(threshold)
    random.seed(4); np.random.seed(4)
    model.debug = {}
    model.injected_pseudo = (ex['pseudo_label'].to(torch.uint8).cuda(), torch.tensor([ex['n_conf']], dtype=torch.int64).cuda())
    out = model.train_step(to_dev(batch, 'cuda'), opt)
    torch.cuda.synchronize()
    lv = out['log_vars']
    assert list(lv.keys()) == list(olog.keys())
    for k, v in olog.items():
        print(f'{name} {k}: {lv[k]!r} oracle {v!r}')
    for k, v in olog.items():
        if k in nan_keys:
            assert lv[k] == 0.0, (k, lv[k])                       # the documented deviation: 0 where the reference has NaN
        else:
            tol = ACC_TOL if k.endswith('acc_seg') else TOL * max(abs(v), 1e-2)
            assert abs(lv[k] - v) <= tol, (k, lv[k], v)
    assert bool(torch.isfinite(model.student_arena.data).all()), 'student weights'
    assert bool(torch.isfinite(model._teacher_arena.data).all()), 'teacher weights'
    stats = [(k, b) for k, b in model.named_buffers() if k.endswith('running_mean') or k.endswith('running_var')]
    assert len(stats) > 200                                       # student and teacher: 2 x 2 x 61 BatchNorm layers
    for k, b in stats:
        assert bool(torch.isfinite(b).all()), k
    return model, lv, student


def test_all_ignored_batch_steps_to_pure_weight_decay(conv_math):
    """Every gt_semantic_seg = 255.  The oracle's four source terms are NaN (empty pair sets, pfgst_loss.py:107-131); ours are exactly 0.0
    (the documented deviation).  Cross-entropy 0, acc_seg 100, target terms 0 as in the oracle.  Every gradient entering the backward
    pass is zero, so each f16x3 / Winograd / K-quad / depthwise / BatchNorm-backward launch runs with amax == 0 and must write exact
    zeros: the gradient arena is exactly zero and AdamW (m = v = 0) leaves p (1 - lr wd), to 1 ulp of the fp64 evaluation.  Under each
    convolution arithmetic."""
    model, lv, student = run_scenario('all_255')
    arena = model.student_arena
    assert all_zero(arena.grad), f'{int((arena.grad != 0).sum())} non-zero gradient elements'
    worst = 0
    for name in arena.names:
        got = arena.view(arena.data, name).detach().cpu()
        want = (student[name].detach().double() * (1.0 - 6e-5 * 0.01)).float()
        off = (got != want) & (got != torch.nextafter(want, want + 1)) & (got != torch.nextafter(want, want - 1))
        worst = max(worst, int(off.sum()))
        assert not bool(off.any()), (name, int(off.sum()))
    print(f'{conv_math}: parameters more than 1 ulp from p (1 - lr wd): {worst}')


def test_single_class_batch_has_no_negative_pairs():
    """Every label 0: the padding band of nn.Unfold carries label 0 too, so the negative set is empty (NaN in the oracle, 0.0 here)."""
    run_scenario('all_class_0')


def test_one_labelled_pixel_keeps_the_weights_finite():
    """One labelled pixel on the loss grid's lattice: the positive set has one element, whose unbiased std is NaN in the reference -- the
    reference's own student diverges in this step (192 tensors non-finite).  Ours reports 0.0 and stays finite."""
    _, _, ex, _ = oracle_step('one_labelled_pixel')
    assert not all(bool(torch.isfinite(g).all()) for g in ex['grads'].values()), 'the oracle was expected to diverge on this batch'
    run_scenario('one_labelled_pixel')


def test_one_image_without_labels_matches_the_oracle():
    run_scenario('one_image_255')


def test_confident_and_unconfident_pseudo_labels_match_the_oracle():
    """The same batch at a threshold that 7955 target pixels pass and at one none passes: the pixel weight of the mixed pass is q > 0 and
    exactly 0."""
    _, conf, _ = run_scenario('confident')
    _, none, _ = run_scenario('none_confident')
    assert abs(conf['mix.decode.loss_ce'] - none['mix.decode.loss_ce']) > 0.1       # the oracle: 0.7168 against 0.4195


def test_supervised_step_on_an_all_ignored_batch():
    """EncoderDecoder.train_step with SGD: loss 0 and acc_seg 100 as oracle.segmentor_forward_train gives, zero gradients, finite weights"""
    from test_supervised_gpu import build_model, oracle_step as sup_oracle_step, seeded_segmentor_state, sup_batch
    state = seeded_segmentor_state(9)
    batch = sup_batch()
    batch['gt_semantic_seg'][:] = 255
    olog, _ = sup_oracle_step(state, batch, torch.float32)
    assert olog['loss'] == 0.0 and olog['decode.loss_ce'] == 0.0 and olog['aux.loss_ce'] == 0.0
    assert abs(olog['decode.acc_seg'] - 100.0) < 1e-3 and abs(olog['aux.acc_seg'] - 100.0) < 1e-3
    model, opt = build_model(state)
    out = model.train_step(to_dev(batch, DEV), opt)
    torch.cuda.synchronize()
    lv = out['log_vars']
    assert list(lv.keys()) == list(olog.keys())
    for k, v in olog.items():
        assert abs(lv[k] - v) <= TOL * max(abs(v), 1e-2), (k, lv[k], v)
    assert lv['loss'] == 0.0 and lv['decode.loss_ce'] == 0.0 and lv['aux.loss_ce'] == 0.0
    arena = model.param_arena
    assert all_zero(arena.grad), f'{int((arena.grad != 0).sum())} non-zero gradient elements'
    assert bool(torch.isfinite(arena.data).all())
    for k, b in model.named_buffers():
        assert not b.is_floating_point() or bool(torch.isfinite(b).all()), k


# ----------------------------------------------------------------------------------------------------------------- 2a. target losses
# images that hold a run of valid pixels, per valid count; count 0: the windows of count 2 with the centre labels set to 255
BOUNDARY_RUNS = {0: (1, 1), 1: (1, 0), 2: (1, 1), 3: (2, 1)}


def boundary_maps(K, d, count, H=16, W=16):
    """full-resolution label / mix maps whose valid count (centre label != 255 AND all K^2 dilated taps inside the map and un-mixed) is
    exactly `count`: everything mixed except one window per image, just wide enough for a run of centres whose taps all lie inside it"""
    gt, _ = labels(2, H, W, 5)
    r = (K // 2) * d
    y0, x0 = 8, 6
    mix = torch.ones(2, 1, H, W, dtype=torch.long)
    for i, run in enumerate(BOUNDARY_RUNS[count]):
        if run:
            mix[i, 0, y0 - r:y0 + r + 1, x0 - r:x0 + run + r] = 0
            if count == 0:
                gt[i, 0, 2 * y0:2 * y0 + 2, 2 * x0:2 * (x0 + run)] = 255
    return gt, mix.repeat_interleave(2, 2).repeat_interleave(2, 3)


@pytest.mark.parametrize('count', [0, 1, 2, 3])
@pytest.mark.parametrize('K', [3, 5])
def test_target_losses_at_the_valid_count_boundary(ops, K, count):
    """trg_valid_mask + sim_topk_loss + cross_prob_bwd_ where `mask.sum() > 1` flips (pfgst_loss.py:227-234, oracle.pfgst_loss:411-421):
    at 0 and 1 valid pixels both losses and every gradient element are exactly 0, at 2 and 3 they equal the fp64 restatement.  The maps
    come from boundary_maps; their counts were checked on the CPU with t_valid, which the test repeats."""
    d, H, W, n, Cc, kk = 2, 16, 16, 2, 6, K * K
    gt, mix = boundary_maps(K, d, count)
    valid_ref, all_ref = t_valid(gt, mix, H, W, K, d)
    assert int(valid_ref.sum()) == count and int(all_ref.sum()) == sum(BOUNDARY_RUNS[count])
    gt8, mm8 = ops.to_u8(gt.to(DEV)), ops.to_u8(mix.to(DEV))
    valid, all_in, cnt = ops.trg_valid_mask(gt8, mm8, (H, W), d, ksize=K)
    assert torch.equal(valid.cpu().bool(), valid_ref) and torch.equal(all_in.cpu().bool(), all_ref)
    assert int(cnt) == count
    gen = torch.Generator().manual_seed(300 + 10 * K + count)
    logits = torch.randn(n, Cc, 2 * H, 2 * W, generator=gen, dtype=torch.float64) * 2
    ema = torch.rand(n, kk, H, W, generator=gen, dtype=torch.float64) * 2 - 1
    prob = torch.softmax(logits[:, :, ::2, ::2], 1)
    for top_k in (3, None):
        for unfold_grad in (False, True):
            lg = logits.clone().requires_grad_()
            pr = torch.softmax(lg[:, :, ::2, ::2], 1)
            q = unfold(pr, K, d)
            cp = (pr.unsqueeze(2) * (q if unfold_grad else q.detach())).sum(1)
            cp.retain_grad()
            es = ema.clone().requires_grad_()
            if top_k is None:
                lp, ln = es * -cp, (1 - es) * -(1 - cp)
            else:
                imax, imin = torch.topk(es, top_k + 1, dim=1)[1], torch.topk(es, top_k, dim=1, largest=False)[1]
                lp = torch.gather(es, 1, imax) * -torch.gather(cp, 1, imax)
                ln = (1 - torch.gather(es, 1, imin)) * -torch.gather(1 - cp, 1, imin)
            m = valid_ref
            out, gP, gS = ops.sim_topk_loss(ema.float().to(DEV), prob.float().to(DEV), valid, cnt, d, top_k, 0.3, 0.7, want_sim_grad=True,
                                            ksize=K)
            dl = torch.zeros(n, Cc, 2 * H, 2 * W, device=DEV)
            ops.cross_prob_bwd_(dl, prob.float().to(DEV), gP, d, 2, unfold_grad, ksize=K)
            if m.sum() > 1:
                want = torch.stack([lp[m.expand_as(lp)].mean() * 0.3, ln[m.expand_as(ln)].mean() * 0.7])
                want.sum().backward()
                e = dict(losses=rel_err(out, want), gP=rel_err(gP, cp.grad), gS=rel_err(gS, es.grad), dlogits=rel_err(dl, lg.grad))
                print(f'K={K} count={count} top_k={top_k} unfold_grad={unfold_grad}: ' + ' '.join(f'{k} {v:.3e}' for k, v in e.items()))
                assert float(want.abs().min()) > 0 and float(lg.grad.abs().max()) > 0
                assert max(e.values()) < 1e-5, e
            else:
                assert count <= 1
                assert float(out[0]) == 0.0 and float(out[1]) == 0.0, out
                assert all_zero(gP) and all_zero(gS) and all_zero(dl)


# ----------------------------------------------------------------------------------------------------------------- 2b. source losses
SRC_CASES = ['all_255', 'all_class_0', 'one_centre', 'constant_sim', 'src_perc_empties_the_negatives']
SRC_PERC = 0.01
# (positive, negative) pair counts of the label map of the src_perc case (2 x 16 x 16 grid, dilation 2), counted on the CPU with the
# restatement below: int(n_neg * 0.01) == 0 while int(n_pos * 0.01) >= 2
SRC_PERC_PAIRS = {3: (4592, 16), 5: (12752, 48)}


def src_case_inputs(case, K, d, H=16, W=16, n=2):
    """-> (full-resolution labels [n, 1, 2H, 2W], similarity map [n, K^2, H, W] fp64, src_perc)"""
    gen = torch.Generator().manual_seed(500 + K)
    N = n * K * K * H * W
    sim = (torch.randperm(N, generator=gen).double() / N * 2 - 1).view(n, K * K, H, W)       # distinct values, in fp32 too
    grid = torch.full((n, 1, H, W), 255, dtype=torch.long)
    perc = None
    if case == 'all_class_0':
        grid[:] = 0
    elif case == 'one_centre':
        grid[1, 0, 8, 8] = 3
    elif case == 'constant_sim':
        grid = F.interpolate(labels(n, H, W, 9)[0].float(), size=(H, W), mode='nearest').long()
        sim = torch.full_like(sim, float(np.float32(0.3)))
    elif case == 'src_perc_empties_the_negatives':
        grid[:] = 0
        grid[0, 0, 8, 8] = 1
        perc = SRC_PERC
    return grid.repeat_interleave(2, 2).repeat_interleave(2, 3), sim, perc


def src_reference(sim, gt, K, d, loss_type, perc):
    """oracle.pfgst_loss:402-408,425-433 in fp64, term by term -> (loss values, the gradient of the FINITE terms, mask of the elements
    that only terms with a NaN value or a NaN gradient feed, (n_pos, n_neg) before src_perc)"""
    n, kk, H, W = sim.shape
    s = sim.clone().requires_grad_()
    g = F.interpolate(gt.float(), size=(H, W), mode='nearest')
    nb = unfold(g.double(), K, d).squeeze(1)
    ctr = g.expand(n, kk, H, W)
    vs = (g != 255).expand(n, kk, H, W)
    pos, neg = s[(nb == ctr) & vs], s[(nb != ctr) & vs]
    pairs = (pos.numel(), neg.numel())
    if perc is not None:
        pos, neg = pos.sort()[0][:int(pos.shape[0] * perc)], neg.sort(descending=True)[0][:int(neg.shape[0] * perc)]
    if loss_type == 'mean_std':
        terms = [-pos.mean() * W4[0], neg.mean() * W4[1], pos.std() * W4[2], neg.std() * W4[3]]
    else:
        e = 1 if loss_type == 'margin' else 2
        terms = [(F.relu(0.7 - pos) ** e).mean() * W4[0], (F.relu(neg - 0.2) ** e).mean() * W4[1]]
    grad, fed = torch.zeros_like(sim), torch.zeros_like(sim, dtype=torch.bool)
    for t in terms:
        gt_, = torch.autograd.grad(t, s, retain_graph=True)
        if bool(torch.isfinite(t)) and bool(torch.isfinite(gt_).all()):
            grad += gt_
            fed |= gt_ != 0
    return torch.stack([t.detach() for t in terms]), grad, ~fed, pairs


@pytest.mark.parametrize('loss_type', ['mean_std', 'margin', 'margin2'])
@pytest.mark.parametrize('case', SRC_CASES)
@pytest.mark.parametrize('K', [3, 5])
def test_source_losses_on_empty_and_singular_sets(ops, K, case, loss_type):
    """src_sim_losses where the reference divides by zero (pfgst_loss.py:107-131): the mean of an empty set, the unbiased std of one
    element, the gradient of the std of a constant set.  Where the fp64 restatement is finite the kernel matches it; where it is NaN the
    loss is exactly 0.0 and the term sends nothing into gsim (the documented deviation).  Default and deterministic mode: each meets every
    assertion, the exact zeros included, and has the same zero pattern in gsim; the finite values of the two modes are compared with a
    tolerance (1e-6 of the largest value), not for equality -- their fp64 sums are taken in different orders."""
    import warnings
    d = 2
    gt, sim, perc = src_case_inputs(case, K, d)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                         # std(): degrees of freedom is <= 0
        want, want_g, unfed, pairs = src_reference(sim, gt, K, d, loss_type, perc)
    nan_terms = ~torch.isfinite(want)
    expect_nan = {'all_255': [0, 1, 2, 3], 'all_class_0': [1, 3], 'one_centre': [2], 'constant_sim': [],
                  'src_perc_empties_the_negatives': [1, 3]}[case]
    assert nan_terms.nonzero().flatten().tolist() == [i for i in expect_nan if i < want.numel()], want
    if case == 'constant_sim' and loss_type == 'mean_std':
        assert float(want[2]) == 0.0 and float(want[3]) == 0.0 and min(pairs) > 1       # std == 0 with n > 1: its gradient is 0 / 0
    if case == 'src_perc_empties_the_negatives':
        assert pairs == SRC_PERC_PAIRS[K] and int(pairs[1] * perc) == 0 and int(pairs[0] * perc) >= 2
    gt8 = ops.to_u8(gt.to(DEV))
    simd = sim.float().to(DEV)
    got = {}
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            losses, gsim = ops.src_sim_losses(simd, gt8, d, *W4, loss_type=loss_type, margin=(0.7, 0.2), src_perc=perc, ksize=K)
            torch.cuda.synchronize()
        finally:
            ops.set_deterministic(False)
        losses, gsim = losses.cpu()[:want.numel()], gsim.cpu()
        got[det] = (losses, gsim)
        print(f'K={K} {case} {loss_type} det={det}: losses {losses.tolist()} fp64 {want.tolist()}')
        assert bool(torch.isfinite(gsim).all()) and bool(torch.isfinite(losses).all())
        for i in range(want.numel()):
            if bool(nan_terms[i]):
                assert float(losses[i]) == 0.0, (i, float(losses[i]))
        if case == 'constant_sim' and loss_type == 'mean_std':
            assert float(losses[2]) == 0.0 and float(losses[3]) == 0.0, losses
        finite = torch.where(nan_terms, torch.zeros_like(want), want)
        if float(finite.abs().max()) > 0:
            assert_close(losses, finite, 1e-5, 'source losses')
        else:
            assert all_zero(losses)
        assert all_zero(gsim[unfed]), f'{int((gsim[unfed] != 0).sum())} elements that only NaN terms feed are not 0'
        if float(want_g.abs().max()) > 0:
            assert_close(gsim, want_g, 1e-5, 'source gradient')
        else:
            assert all_zero(gsim)
    assert rel_err(got[True][0], got[False][0]) < 1e-6 or all_zero(got[False][0])
    assert rel_err(got[True][1], got[False][1]) < 1e-6 or all_zero(got[False][1])
    assert torch.equal(got[True][1] == 0, got[False][1] == 0)


# ----------------------------------------------------------------------------------------------------------------- 2c. cosine similarity
ZERO_PATTERNS = ['isolated_pixel', 'block_5x5', 'border_row_and_column', 'image_1']


def zero_pattern(x, pattern):
    """zero feature vectors in x [n, C, H, W] in place -> bool [n, H, W] of the zeroed pixels"""
    z = torch.zeros(x.shape[0], *x.shape[2:], dtype=torch.bool)
    if pattern == 'isolated_pixel':
        z[0, 9, 11] = True
    elif pattern == 'block_5x5':
        z[0, 6:11, 8:13] = True                 # centre and taps both zero inside the block
    elif pattern == 'border_row_and_column':
        z[0, 0, :] = True                       # next to the zero padding
        z[0, :, -1] = True
    else:
        z[1] = True
    x.masked_fill_(z.unsqueeze(1), 0.0)
    return z


def simq_ok(C, H, W, d, *tensors):
    """pfgst_loss.hip:simq_ok and the alignment conditions of pfst_sim_map / pfst_sim_map_bwd restated (forward: feat, sim, norm; adjoint:
    feat, dfeat, coef): the 3 x 3 cosine entries take their strip kernels.  A restatement: it has to follow a change of the C++ condition"""
    return (d in (1, 2) and W % 4 == 0 and W // 4 in (16, 32, 64) and (H * W) % 256 == 0 and C % 4 == 0
            and all(t.data_ptr() % 16 == 0 for t in tensors))


FAST_SHAPES = [(2, 16, 16, 64), (2, 72, 16, 64)]      # 4 channel slices per strip; 8 (C % 8 == 0, C >= 64: the training shape's variant), two
#                                                       channel chunks in the adjoint, the second ragged
SIM_CASES = [(shape, 3, d, '3x3') for shape in FAST_SHAPES for d in (1, 2)]           # the strip kernels of the 3 x 3 entry
SIM_CASES += [
    ((2, 37, 21, 23), 3, 2, '3x3'),                                         # its generic kernels
    ((2, 37, 21, 23), 3, 2, 'k'), ((2, 37, 21, 23), 5, 2, 'k'), ((2, 37, 21, 23), 7, 1, 'k')]       # the K x K halo-tile family


def sim_inputs(shape, K, d, pattern):
    """-> (non-negative features fp64 with the pattern's pixels zeroed, their mask [n, H, W], a signed upstream gradient, a base tensor)"""
    n, C, H, W = shape
    gen = torch.Generator().manual_seed(700 + 10 * K + d)
    x = torch.randn(n, C, H, W, generator=gen, dtype=torch.float64).abs() * 0.5
    z = zero_pattern(x, pattern)
    gs = torch.randn(n, K * K, H, W, generator=gen, dtype=torch.float64)
    return x, z, gs, torch.randn(n, C, H, W, generator=gen)


def test_fp32_autograd_misses_the_per_element_bound_under_a_signed_gradient():
    """The reason the per-element comparison below runs under a non-negative upstream gradient: under a signed one the terms of a
    zero-pixel element cancel, and torch's own fp32 autograd of t_sim (the reference's arithmetic) is more than 1e-5 of the element's
    fp64 value away on some of them (1.7e-2 at worst on this input; 8e-6 .. 1.7e-2 over the inputs of the test below), while under the
    non-negative one it stays within 3e-7.  No GPU code runs here."""
    shape, K, d = (2, 37, 21, 23), 5, 2
    x, z, gs, _ = sim_inputs(shape, K, d, 'block_5x5')
    zc = z.unsqueeze(1).expand(*shape)
    worst = {}
    for signed in (True, False):
        g64 = gs if signed else gs.abs()
        xr, x32 = x.clone().requires_grad_(), x.float().requires_grad_()
        t_sim(xr, K, d, 'cosine', 1.0).backward(g64)
        t_sim(x32, K, d, 'cosine', 1.0).backward(g64.float())
        dz, wz = (x32.grad.double() - xr.grad)[zc].abs(), xr.grad[zc].abs()
        worst[signed] = float((dz[wz > 0] / wz[wz > 0]).max())
    print(f'fp32 autograd, worst zero-pixel element relative to its own fp64 value: signed {worst[True]:.3e}, non-negative {worst[False]:.3e}')
    assert worst[True] > 1e-5 and worst[False] < 1e-6


@pytest.mark.parametrize('pattern', ZERO_PATTERNS)
@pytest.mark.parametrize('shape,K,d,entry', SIM_CASES)
def test_cosine_similarity_at_zero_norm_pixels(ops, shape, K, d, entry, pattern):
    """sim_map + sim_map_bwd where a feature vector is exactly zero (the decoded features come after a ReLU): each norm is clamped at
    1e-8, so the map is 0 there and the gradient of order 1e8 x gs -- the reference's arithmetic (F.cosine_similarity) and t_sim's.
    (2, 16, 16, 64) and (2, 72, 16, 64) take the 3 x 3 strip kernels (4 and 8 channel slices per strip), (2, 37, 21, 23) the generic
    3 x 3 kernels and the K x K halo-tile family.  Forward and adjoint, accumulating and not.
    The features are non-negative, as after a ReLU.  The adjoint runs twice.  With a signed upstream gradient the pixels that hold a
    feature vector are compared against the largest gradient among them, and the zero pixels against the largest among those.  With a
    non-negative upstream gradient every zero-pixel element is compared with its OWN fp64 value, to 1e-5 of it: such an element is
    sum_k (gs_k + gs'_k) x_q / (1e-8 |x_q|), a sum of non-negative terms, so fp32 evaluates it to a few 2^-24 of its value.  (Under a
    signed gradient the terms cancel and no fp32 evaluation meets a per-element bound:
    test_fp32_autograd_misses_the_per_element_bound_under_a_signed_gradient.)"""
    n, C, H, W = shape
    x, z, gs, base = sim_inputs(shape, K, d, pattern)
    zc = z.unsqueeze(1).expand(n, C, H, W)
    xf = x.float().to(DEV)
    if entry == '3x3':
        sim, norm = ops.sim_map(xf, d, 'cosine')
        assert simq_ok(C, H, W, d, xf, sim, norm) == (shape in FAST_SHAPES)
    else:
        sim, norm = torch.empty(n, K * K, H, W, device=DEV), torch.empty(n, H, W, device=DEV)
        ops.call('pfst_sim_map_k', xf.data_ptr(), n, C, H, W, K, d, 0, 1.0, sim.data_ptr(), norm.data_ptr(), 0)
    assert bool(torch.isfinite(sim).all())
    assert_close(sim, t_sim(x, K, d, 'cosine', 1.0), 1e-5, 'sim')
    assert all_zero(norm.cpu()[z]), 'norm at the zero pixels'
    assert_close(norm, x.norm(dim=1), 1e-6, 'norm')
    for signed in (True, False):
        g64 = gs if signed else gs.abs()
        xr = x.clone().requires_grad_()
        t_sim(xr, K, d, 'cosine', 1.0).backward(g64)
        assert bool(torch.isfinite(xr.grad).all()), 'the fp64 gradient must be finite for this input'
        gsf = g64.float().to(DEV)
        for accumulate in (False, True):
            out = base.clone().to(DEV)
            coef = torch.empty(n * (K * K + 1) * H * W, device=DEV)
            if entry == '3x3':
                assert simq_ok(C, H, W, d, xf, out, coef) == (shape in FAST_SHAPES)        # the adjoint's own conditions
                ops.call('pfst_sim_map_bwd', xf.data_ptr(), sim.data_ptr(), norm.data_ptr(), gsf.data_ptr(), n, C, H, W, d, 0, 1.0,
                         out.data_ptr(), int(accumulate), coef.data_ptr(), 0)
            else:
                ops.call('pfst_sim_map_bwd_k', xf.data_ptr(), sim.data_ptr(), norm.data_ptr(), gsf.data_ptr(), n, C, H, W, K, d, 0, 1.0,
                         out.data_ptr(), int(accumulate), coef.data_ptr(), 0)
            want = xr.grad + (base.double() if accumulate else 0)
            got = out.double().cpu()
            assert bool(torch.isfinite(got).all())
            dz, wz = (got - want)[zc].abs(), want[zc].abs()
            e_live = float((got - want)[~zc].abs().max() / (want[~zc].abs().max() + 1e-12))
            e_zero_max = float(dz.max() / (wz.max() + 1e-12))
            e_zero = float((dz / wz.clamp_min(1e-300)).max())
            print(f'{shape} K={K} d={d} {entry} {pattern} signed={signed} accumulate={accumulate}: live pixels {e_live:.3e}, zero pixels '
                  f'{e_zero_max:.3e} of their maximum {float(wz.max()):.3e}, per element {e_zero:.3e}')
            assert e_live < 1e-5 and e_zero_max < 1e-5, (e_live, e_zero_max)
            if not signed:
                assert bool((dz <= 1e-5 * wz).all()), e_zero


# ----------------------------------------------------------------------------------------------------------------- 2d. fused cross-entropy
CE_SETS = [(2, C, h, h, H, H, use_w, use_cw) for C, h, H, use_w, use_cw in
           [(6, 16, 64, True, False), (6, 8, 64, False, False), (33, 12, 48, True, True), (2, 16, 64, True, False), (6, 64, 256, True, True),
            (8, 32, 128, False, False), (6, 7, 28, False, True), (5, 31, 124, True, True), (6, 2, 8, True, False)]]       # test_ce_upsample_fwd_bwd
CE_SETS += [(3, C, h, w, S * h, S * w, True, True) for S in (4, 8)
            for C, h, w in [(6, 33, 17), (8, 16, 46), (1, 15, 15), (6, 30, 31), (3, 1, 9)]]                              # the inter-cell-block kernels


@pytest.mark.parametrize('case', ['all_255', 'zero_pixel_weight', 'one_pixel'])
@pytest.mark.parametrize('n,C,h,w,H,W,use_w,use_cw', CE_SETS)
def test_fused_cross_entropy_with_nothing_to_average(ops, n, C, h, w, H, W, use_w, use_cw, case):
    """ce_upsample_fwd / _bwd / ce_finalize and CrossEntropyLoss.fused on label maps that are all ignore_index, under an all-zero pixel
    weight, and with a single labelled pixel, against F.cross_entropy(reduction='none').mean() in fp64 (oracle.ce_loss) and
    oracle.accuracy (100.0 for the empty set).  Both label-map alignments: the inter-cell-block kernels and the per-pixel kernels."""
    from oracle import pfst_oracle as O
    from pfst_amd.engine import Var
    from pfst_amd.models import CrossEntropyLoss
    gen = torch.Generator().manual_seed(900 + C + h)
    logits = (torch.randn(n, C, h, w, generator=gen, dtype=torch.float64) * 3).requires_grad_()
    label = torch.randint(0, C, (n, H, W), generator=gen)
    pw = torch.rand(n, H, W, generator=gen, dtype=torch.float64) if use_w else None
    cw = (torch.rand(C, generator=gen, dtype=torch.float64) + 0.5) if use_cw else None
    if case == 'all_255':
        label[:] = 255
    elif case == 'zero_pixel_weight':
        pw = torch.zeros(n, H, W, dtype=torch.float64)
    else:
        one = int(label[n - 1, H // 2, W // 3])
        label[:] = 255
        label[n - 1, H // 2, W // 3] = one
    lw = 0.4
    up = F.interpolate(logits, size=(H, W), mode='bilinear', align_corners=False)
    per = F.cross_entropy(up, label, weight=cw, reduction='none', ignore_index=255)
    if pw is not None:
        per = per * pw
    loss_ref = lw * per.mean()
    loss_ref.backward()
    acc_ref = float(O.accuracy(up.detach().float(), label))
    empty = case != 'one_pixel'
    zero_grad = empty or C == 1                   # one class: the softmax is 1 and the cross-entropy 0 everywhere
    if case == 'all_255':
        assert acc_ref == 100.0
    assert (float(loss_ref) == 0.0) == zero_grad and all_zero(logits.grad) == zero_grad
    ld = logits.detach().float().to(DEV)
    pwd = None if pw is None else pw.float().to(DEV)
    cwd = None if cw is None else cw.float().to(DEV)
    even = ops.to_u8(label.to(DEV))
    odd = torch.empty(even.numel() + 1, dtype=torch.uint8, device=DEV)[1:].view(n, H, W)
    odd.copy_(even)
    assert even.data_ptr() % 2 == 0 and odd.data_ptr() % 2 == 1
    base = torch.randn(n, C, h, w, generator=gen).to(DEV)
    for l8 in (even, odd):
        lse, acc = ops.ce_upsample_fwd(ld, l8, pwd, cwd)
        out = ops.ce_finalize(acc, n * H * W, lw).cpu()
        acc = acc.cpu()
        assert bool(torch.isfinite(out).all()) and float(out[2]) == 0.0
        assert abs(float(acc[0]) - float(per.sum())) <= 1e-5 * max(1.0, abs(float(per.sum())))
        assert abs(float(out[0]) - float(loss_ref)) < 1e-5 * max(1.0, abs(float(loss_ref)))
        assert abs(float(out[1]) - acc_ref) < 1e-3
        assert float(acc[2]) == float((label != 255).sum())
        dl = ops.ce_upsample_bwd(ld, l8, lse, lw / (n * H * W), pwd, cwd)
        dacc = ops.ce_upsample_bwd(ld, l8, lse, lw / (n * H * W), pwd, cwd, out=base.clone(), accumulate=True)
        assert bool(torch.isfinite(dl).all())
        if empty:
            assert float(out[0]) == 0.0
        if zero_grad:
            assert all_zero(dl), f'{int((dl != 0).sum())} non-zero gradient elements'
            assert same_bits(dacc, base), 'accumulating a zero gradient changed the destination'
        else:
            assert_close(dl, logits.grad, 1e-4, 'ce bwd')
            assert_close(dacc, base.double().cpu() + logits.grad, 1e-4, 'ce bwd accumulate')
        if case == 'all_255':
            assert float(out[1]) == 100.0 and float(acc[1]) == 0.0
    mod = CrossEntropyLoss(loss_weight=lw, class_weight=None if cw is None else cw.tolist())
    fused = mod.fused(Var(ld, True), even, pwd, None).cpu()
    assert abs(float(fused[1]) - acc_ref) < 1e-3 and abs(float(fused[0]) - float(loss_ref)) < 1e-5 * max(1.0, abs(float(loss_ref)))
    if case == 'all_255':
        assert float(fused[1]) == 100.0 and float(fused[0]) == 0.0


# ----------------------------------------------------------------------------------------------------------------- 2e. f16x3 arithmetic
TINY = 1e-30            # a normal float (2^-99.7); the scales clamp at biased exponent 16 (2^-111, csrc/amax.h), far below
CLAMPED = 2.0 ** -118   # maxima of biased exponent 9: inside the range amax_exponent clamps (below 16)
F16_TOL = 3e-6          # tests/test_hip_ops.py: test_conv_f16x3_is_fp32_faithful (wgrad), test_wgrad_f16x3_on_the_quad_kernel
F16_SHAPES = [(2, 64, 64, 32, 32, 3, 1), (2, 256, 64, 16, 16, 1, 1)]          # n, cin, cout, H, W, k, dil (stride 1, 'same' padding)


def g(seed):
    return torch.Generator().manual_seed(seed)


def amax_zero(slots):
    return all_zero(slots)


def clamped_operand(shape, seed):
    """normal floats of magnitude 0.5 .. 1.5 x 2^-118 with random signs: every element is a normal float (>= 2^-119) and the tensor's
    maximum has biased exponent 9, which amax_exponent raises to 16"""
    gen = g(seed)
    t = (0.5 + torch.rand(shape, generator=gen)) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1) * CLAMPED
    assert float(t.abs().min()) >= 2.0 ** -119 and 1 <= ((t.abs().max().view(torch.int32) >> 23) & 0xff) < 16
    return t


@pytest.mark.parametrize('case', F16_SHAPES)
def test_f16x3_gemm_with_zero_and_tiny_operands(ops, case):
    """conv_fprop_f16x3 / conv_dgrad_f16x3 / conv_wgrad_f16q_ with an operand that is all zero (amax_publish leaves the slot group
    untouched and the products must be exact zeros), with one scaled by 1e-30 (the error bound of the normal-range tests carries over), and
    with one whose maximum lies in the range amax_exponent clamps (biased exponent below 16).  The last is what pins that clamp: a zero
    maximum does not -- without the clamp its scale and inverse scale are the finite -2^-115 and -2^115, and 0 times either is still 0 --
    but for exponents 1 .. 15 the unclamped scale field 268 - e exceeds 8 bits, a float with the sign bit set and a wrong exponent.  With
    the clamp the scale is 2^125 and the two fp16 pieces hold x 2^125 (magnitudes 2^6 .. 2^8) to 22 bits, as in the normal range."""
    n, ci, co, H, W, k, d = case
    p = d if k == 3 else 0
    x = torch.randn(n, ci, H, W, generator=g(1))
    w = torch.randn(co, ci, k, k, generator=g(2)) * 0.1
    dy = torch.randn(n, co, H, W, generator=g(4))
    bias = torch.randn(co, generator=g(5))
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    assert ops.f16x3_eligible(ci, co, k) and ops.f16x3_eligible(co, ci, k)
    w4f, w4d, wa = ops.pack_weight_f16x2(wd, True, True)
    zx, zdy = torch.zeros_like(xd), torch.zeros_like(dyd)
    zxa, zda = ops.absmax(zx), ops.absmax(zdy)
    assert zxa.numel() == ops.AMAX_SUB and amax_zero(zxa) and amax_zero(zda) and float(zxa.max()) == 0.0
    # ---- forward, x == 0: the bias or 0, finite BatchNorm statistics, nothing published for the normalised output
    y = ops.conv_fprop_f16x3(zx, w4f, wa, zxa, co, k, 1, d, p)
    assert all_zero(y)
    yb = ops.conv_fprop_f16x3(zx, w4f, wa, zxa, co, k, 1, d, p, bias=bias.to(DEV))
    assert same_bits(yb, bias.to(DEV).view(1, co, 1, 1).expand(n, co, H, W))
    y_st, st, slots = ops.conv_fprop_f16x3(zx, w4f, wa, zxa, co, k, 1, d, p, want_stats=True)
    one, zero = torch.ones(co, device=DEV), torch.zeros(co, device=DEV)
    mean, invstd, coef = ops.bn_finalize_partials(st, slots, co, n * H * W, gamma=one, beta=zero)
    assert all_zero(y_st) and all_zero(mean) and bool(torch.isfinite(invstd).all()) and bool(torch.isfinite(coef).all())
    assert_close(invstd, torch.full((co,), 1e-5, dtype=torch.float64).rsqrt(), 1e-6, 'invstd of a zero tensor')
    out_amax = ops.amax_slots(torch.device(DEV, torch.cuda.current_device()))
    yn = ops.bn_apply(y_st, mean, invstd, one, zero, relu=True, amax=out_amax)
    assert all_zero(yn) and amax_zero(out_amax), 'a zero tensor published a maximum'
    # ---- data gradient, dy == 0: exact zeros; accumulating leaves the destination bit-unchanged
    dx = ops.conv_dgrad_f16x3(zdy, w4d, wa, zda, ci, (H, W), k, 1, d, p)
    assert all_zero(dx)
    base = torch.randn(n, ci, H, W, generator=g(6)).to(DEV)
    dxa = ops.conv_dgrad_f16x3(zdy, w4d, wa, zda, ci, (H, W), k, 1, d, p, out=base.clone(), accumulate=True)
    assert same_bits(dxa, base)
    # ---- K-quad weight gradient, dy == 0 into a random dw
    dw0 = torch.randn(co, ci, k, k, generator=g(7)).to(DEV)
    dw = ops.conv_wgrad_f16q_(dw0.clone(), xd, zdy, ops.absmax(xd), zda, k, d)
    assert same_bits(dw, dw0)
    # ---- one operand scaled by 1e-30
    xt, dyt = x * TINY, dy * TINY
    assert float(xt.abs()[xt != 0].min()) > 1.2e-38 and float(dyt.abs()[dyt != 0].min()) > 1.2e-38, 'operands must be normal floats'
    xtd, dytd = xt.to(DEV), dyt.to(DEV)
    xta, dyta = ops.absmax(xtd), ops.absmax(dytd)
    assert float(xta.max()) == float(xt.abs().max())
    ref = F.conv2d(xt.double(), w.double(), None, 1, p, d)
    assert_close(ops.conv_fprop_f16x3(xtd, w4f, wa, xta, co, k, 1, d, p), ref, F16_TOL, 'f16x3 fprop, x * 1e-30')
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), dyt.double(), 1, p, d)
    assert_close(ops.conv_dgrad_f16x3(dytd, w4d, wa, dyta, ci, (H, W), k, 1, d, p), dx_ref, F16_TOL, 'f16x3 dgrad, dy * 1e-30')
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dyt.double(), 1, p, d)
    dw = ops.conv_wgrad_f16q_(torch.zeros(co, ci, k, k, device=DEV), xd, dytd, ops.absmax(xd), dyta, k, d)
    assert_close(dw, dw_ref, F16_TOL, 'f16x3 quad wgrad, dy * 1e-30')
    # ---- one operand with its maximum inside the clamped range
    xc, dyc = clamped_operand(x.shape, 11), clamped_operand(dy.shape, 12)
    xcd, dycd = xc.to(DEV), dyc.to(DEV)
    xca, dyca = ops.absmax(xcd), ops.absmax(dycd)
    assert float(xca.max()) == float(xc.abs().max()) and float(dyca.max()) == float(dyc.abs().max())
    ref = F.conv2d(xc.double(), w.double(), None, 1, p, d)
    assert_close(ops.conv_fprop_f16x3(xcd, w4f, wa, xca, co, k, 1, d, p), ref, F16_TOL, 'f16x3 fprop, max |x| = 1.5 * 2^-118')
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), dyc.double(), 1, p, d)
    assert_close(ops.conv_dgrad_f16x3(dycd, w4d, wa, dyca, ci, (H, W), k, 1, d, p), dx_ref, F16_TOL, 'f16x3 dgrad, max |dy| = 1.5 * 2^-118')
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, k, k), dyc.double(), 1, p, d)
    dw = ops.conv_wgrad_f16q_(torch.zeros(co, ci, k, k, device=DEV), xd, dycd, ops.absmax(xd), dyca, k, d)
    assert_close(dw, dw_ref, F16_TOL, 'f16x3 quad wgrad, max |dy| = 1.5 * 2^-118')


def test_f16x3_whole_line_weight_gradient_with_zero_and_tiny_dy(ops):
    """conv_wgrad_f16x3_ (1 x 1, more than 64 output rows: (2, 64, 256, 16, 16), the mirror of the suite's (2, 256, 64, 16, 16) shape, which
    this kernel refuses): dy == 0 leaves a random dw bit-unchanged; dy * 1e-30, and a dy whose maximum lies in the range amax_exponent
    clamps, within 3e-6 of fp64"""
    n, ci, co, H, W = 2, 64, 256, 16, 16
    x = torch.randn(n, ci, H, W, generator=g(1))
    dy = torch.randn(n, co, H, W, generator=g(4))
    xd = x.to(DEV)
    xa = ops.absmax(xd)
    zdy = torch.zeros(n, co, H, W, device=DEV)
    dw0 = torch.randn(co, ci, 1, 1, generator=g(7)).to(DEV)
    assert same_bits(ops.conv_wgrad_f16x3_(dw0.clone(), xd, zdy, xa, ops.absmax(zdy)), dw0)
    dyt = dy * TINY
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 1, 1), dyt.double(), 1, 0, 1)
    dw = ops.conv_wgrad_f16x3_(torch.zeros(co, ci, 1, 1, device=DEV), xd, dyt.to(DEV), xa, ops.absmax(dyt.to(DEV)))
    assert_close(dw, dw_ref, F16_TOL, 'f16x3 wgrad, dy * 1e-30')
    dyc = clamped_operand(dy.shape, 12)
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 1, 1), dyc.double(), 1, 0, 1)
    dw = ops.conv_wgrad_f16x3_(torch.zeros(co, ci, 1, 1, device=DEV), xd, dyc.to(DEV), xa, ops.absmax(dyc.to(DEV)))
    assert_close(dw, dw_ref, F16_TOL, 'f16x3 wgrad, max |dy| = 1.5 * 2^-118')


def test_winograd_f16x3_with_zero_and_tiny_operands(ops):
    """the Winograd pipeline on the f16x3 GEMM (F(2x2, 3x3); (1, 96, 128, 16, 16), a shape of test_winograd_on_the_f16x3_gemm with more
    than 64 output rows, which the f16 weight-gradient variant needs): zero weights give exact zeros, dy == 0 leaves dw bit-unchanged,
    operands scaled by 1e-30 stay within 3e-6 of fp64"""
    n, ci, co, H, W, d, m = 1, 96, 128, 16, 16, 1, 2
    x = torch.randn(n, ci, H, W, generator=g(1))
    w = torch.randn(co, ci, 3, 3, generator=g(2)) * 0.1
    dy = torch.randn(n, co, H, W, generator=g(4))
    xd = x.to(DEV)
    uf0, _, af0, _ = ops.wino_pack_weight_f16(torch.zeros(co, ci, 3, 3, device=DEV), True, False, m=m)
    assert amax_zero(af0)
    y0 = ops.wino_conv(xd, uf0, co, d, m=m, u_amax=af0)
    assert all_zero(y0)
    uf, ud, af, ad = ops.wino_pack_weight_f16(w.to(DEV), m=m)
    assert all_zero(ops.wino_conv(torch.zeros_like(xd), uf, co, d, m=m, u_amax=af))
    assert ops.wino_tiles(H, W, d, m) % 4 == 0
    dw0 = torch.randn(co, ci, 3, 3, generator=g(7)).to(DEV)
    zdy = torch.zeros(n, co, H, W, device=DEV)
    assert same_bits(ops.wino_wgrad_(dw0.clone(), xd, zdy, d, m=m, split=2), dw0)
    y, (v, v_amax) = ops.wino_conv(xd, uf, co, d, m=m, u_amax=af, keep_v=True)
    assert same_bits(ops.wino_wgrad_(dw0.clone(), xd, zdy, d, v=v, m=m, split=2, v_amax=v_amax), dw0)
    xt, dyt = x * TINY, dy * TINY
    ref = F.conv2d(xt.double(), w.double(), None, 1, d, d)
    assert_close(ops.wino_conv(xt.to(DEV), uf, co, d, m=m, u_amax=af), ref, F16_TOL, 'winograd/f16x3 fprop, x * 1e-30')
    dx_ref = torch.nn.grad.conv2d_input(x.shape, w.double(), dyt.double(), 1, d, d)
    assert_close(ops.wino_conv(dyt.to(DEV), ud, ci, d, m=m, u_amax=ad), dx_ref, F16_TOL, 'winograd/f16x3 dgrad, dy * 1e-30')
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (co, ci, 3, 3), dyt.double(), 1, d, d)
    dw = ops.wino_wgrad_(torch.zeros(co, ci, 3, 3, device=DEV), xd, dyt.to(DEV), d, m=m, split=2)
    assert_close(dw, dw_ref, F16_TOL, 'winograd/f16x3 wgrad, dy * 1e-30')


def test_absmax_of_a_zero_tensor(ops):
    a = ops.absmax(torch.zeros(3, 40, 9, 11, device=DEV))
    assert a.numel() == ops.AMAX_SUB and float(a.max()) == 0.0 and all_zero(a)
    planes = ops.absmax(torch.zeros(3, 40, 9, 11, device=DEV), planes=3)
    assert planes.numel() == 3 * ops.AMAX_SUB and float(planes.max()) == 0.0
