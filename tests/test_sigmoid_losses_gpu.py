"""FocalLoss and CrossEntropyLoss(use_sigmoid=True) fused with the decode head's bilinear up-sampling (csrc/sigmoid_loss.hip) against the fp64
closed form (tests/sigmoid_loss_oracle.py) and against the executed reference (tests/golden/sigmoid_losses.npz, written by
tests/golden/make_golden_focal.py); the two terms inside BaseDecodeHead's loss lists.

Bounds: the loss and every per-(image, class) sum within 1e-5 relative of fp64; every gradient element |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref|
(the per-link bound) against fp64 and against the reference's fp32; counts exact.  For scale, the reference's own fp32 path
sits <= 1.2e-7 (loss) and <= 1.7e-3 of the bound (gradients) from fp64 on the same inputs (tests/test_sigmoid_losses_cpu.py).
Measured on an MI355X (worst over the 17 cases): loss 4.1e-8 relative, per-class sums 1.1e-7, gradients 1.9e-3 of the per-link bound against
fp64 and 1.0e-3 against the reference's fp32; block against generic form: sums 1.6e-16, gradients 6.5e-4 of the bound; the head case 4.6e-4."""
import os

import numpy as np
import pytest
import torch

import sigmoid_loss_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
ALPHA6 = [0.25, 0.5, 0.75, 0.1, 0.9, 0.4]
CW33 = [0.5 + 0.05 * i for i in range(33)]
SIZES = {'x4': (76, 68), 'x8': (136, 144), 'x8c33': (136, 144), 'x8bad': (136, 144), 'g11': (30, 37), 'g2': (30, 37), 'x4sat': (76, 68)}
FORMS = {'x4': 4, 'x8': 8, 'x8bad': 8, 'x4sat': 4}
# name: (inputs, (k_pos, k_neg) rows, gamma, reduction, loss_weight, pixel weights?, accumulate?, the fixture's case or None)
CASES = {
    'x4_focal': ('x4', O.focal_coef(6), 2.0, 'mean', 1.0, True, False, 'x4_focal'),
    'x4_bce': ('x4', O.bce_coef(6), 0.0, 'mean', 1.0, True, True, 'x4_bce'),
    'x4_bce_pos': ('x4', O.bce_coef(6, CW6), 0.0, 'mean', 0.4, False, False, None),
    'x4_g05': ('x4', O.focal_coef(6, ALPHA6), 0.5, 'sum', 1.0, True, True, None),
    'x8_focal': ('x8', O.focal_coef(6, ALPHA6, CW6), 3.0, 'mean', 1.0, True, True, 'x8_focal'),
    'x8_g0': ('x8', O.focal_coef(6, 0.25), 0.0, 'none', 1.0, False, False, None),
    'x8_bad': ('x8bad', O.focal_coef(6), 2.0, 'mean', 1.0, True, False, None),
    'x8c33_focal': ('x8c33', O.focal_coef(33, 0.25, CW33), 2.0, 'sum', 1.0, True, False, None),
    'x8c33_g05': ('x8c33', O.focal_coef(33), 0.5, 'mean', 3.0, False, True, None),
    'x8c33_bce': ('x8c33', O.bce_coef(33, CW33), 0.0, 'mean', 1.0, True, False, None),
    'g11_focal': ('g11', O.focal_coef(11, 0.25), 0.5, 'none', 1.0, True, False, 'g11_focal'),
    'g11_g3': ('g11', O.focal_coef(11, [0.1 + 0.08 * i for i in range(11)]), 3.0, 'mean', 1.0, True, True, None),
    'g2_focal': ('g2', O.focal_coef(2, [0.3, 0.6]), 0.0, 'sum', 1.0, False, False, 'g2_focal'),
    'g2_bce': ('g2', O.bce_coef(2), 0.0, 'mean', 0.5, False, True, 'g2_bce'),
    'g2_g2': ('g2', O.focal_coef(2, 0.5, [0.6, 1.4]), 2.0, 'mean', 1.0, True, False, None),
    # saturated logits (the x4 ones times 40): the literal formula's autograd is NaN at gamma = 0.5; the closed form is finite
    'sat_g05': ('x4sat', O.focal_coef(6), 0.5, 'mean', 1.0, True, False, None),
    'sat_g2': ('x4sat', O.focal_coef(6, ALPHA6, CW6), 2.0, 'mean', 1.0, True, True, None),
}


def make_c33(base):
    return torch.stack([base[:, c % 6] * (1.0 + (c // 6) / 8.0) + (c // 6) / 4.0 for c in range(33)], 1).contiguous()


@pytest.fixture(scope='module')
def golden(golden_dir):
    return O.load_fixture(os.path.join(golden_dir, 'sigmoid_losses.npz'))


@pytest.fixture(scope='module')
def inputs(golden):
    """{inputs name: (logits, label uint8, weight [N, H, W])} on the CPU"""
    out = {}
    for src in ('x4', 'x8', 'g11', 'g2'):
        out[src] = (torch.from_numpy(golden[src + '|logits']), torch.from_numpy(golden[src + '|label']),
                    O.expand_blocks(torch.from_numpy(golden[src + '|weight_blocks']), SIZES[src]))
    z8, l8, w8 = out['x8']
    out['x8c33'] = (make_c33(z8), l8, w8)
    bad = l8.clone()
    bad[1, 16:20, 4:8] = 7                              # outside [0, 6), not the ignore index: the reference raises on it
    out['x8bad'] = (z8, bad, w8)
    out['x4sat'] = (out['x4'][0] * 40, out['x4'][1], out['x4'][2])
    return out


@pytest.fixture(scope='module')
def ref64(inputs):
    """the fp64 closed form of every case, computed once"""
    out = {}
    for name, (src, coef, gamma, red, lw, weighted, _, _) in CASES.items():
        z, lab, w = inputs[src]
        out[name] = O.sigmoid_loss(z, lab, SIZES[src], coef, gamma, w if weighted else None, 255, red, lw)
    return out


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


def run_sig(ops, z, lab, w, coef, gamma, reduction, loss_weight, accumulate=False, base=None, generic=False):
    ld, l8 = z.to(DEV), lab.to(DEV)
    wd = None if w is None else w.to(DEV)
    cf = torch.tensor(coef, dtype=torch.float32, device=DEV)
    n, c = z.shape[:2]
    D = O.divisor(reduction, n, c, *lab.shape[-2:])
    slab, counts, form = ops.sigloss_upsample_fwd(ld, l8, cf, gamma, wd, 255, generic=generic)
    out, sums = ops.sigloss_finalize(slab, counts, D, loss_weight)
    if accumulate:
        grad = ops.sigloss_upsample_bwd(ld, l8, cf, loss_weight / D, gamma, wd, 255, out=base.clone(), accumulate=True, generic=generic)
    else:
        grad = ops.sigloss_upsample_bwd(ld, l8, cf, loss_weight / D, gamma, wd, 255, generic=generic)
    _, acc_ce = ops.ce_upsample_fwd(ld, l8)
    torch.cuda.synchronize()
    return dict(out=out, sums=sums, slab=slab, counts=counts, grad=grad, form=form, acc_ce=acc_ce)


def case_args(inputs, name):
    src, coef, gamma, red, lw, weighted, accumulate, fix = CASES[name]
    z, lab, w = inputs[src]
    return src, (z, lab, w if weighted else None, coef, gamma, red, lw), accumulate, fix


@pytest.mark.parametrize('name', list(CASES))
def test_kernels_against_fp64_and_the_reference(ops, golden, inputs, ref64, name):
    src, args, accumulate, fix = case_args(inputs, name)
    z, lab = args[0], args[1]
    n, C = z.shape[:2]
    r = ref64[name]
    assert ops.sigloss_form(z.to(DEV), lab.to(DEV), None if args[2] is None else args[2].to(DEV))[0] == FORMS.get(src, 0)
    base = torch.randn(z.shape, generator=torch.Generator().manual_seed(5)).to(DEV) * float(np.abs(r['grad']).max())
    got = run_sig(ops, *args, accumulate=accumulate, base=base)
    assert got['form'] == FORMS.get(src, 0)
    sums = got['sums'].cpu()
    # counts: exact, and the CE kernels' on the same inputs
    acc_ce = got['acc_ce'].cpu()
    assert sums[n * C:].tolist() == [float(v) for v in r['counts']], (sums[n * C:], r['counts'])
    assert sums[n * C:].tolist() == acc_ce[1:].tolist(), (sums[n * C:], acc_ce)
    assert (r['counts'][2] > 0) == (src == 'x8bad') and float(got['out'][2]) == r['counts'][2]
    acc = (r['counts'][0] + 1.1920928955078125e-07) * (100.0 / (r['counts'][1] + 1.1920928955078125e-07))
    assert float(got['out'][1]) == float(np.float32(acc))
    assert np.isfinite(sums.numpy()).all() and bool(torch.isfinite(got['out']).all()) and bool(torch.isfinite(got['grad']).all())
    # the loss and the per-(image, class) sums against fp64
    s = sums[:n * C].view(n, C).numpy()
    e_sum = float(np.max(np.where(r['sums'] == s, 0.0, np.abs(s - r['sums']) / np.maximum(np.abs(r['sums']), 1e-300))))
    e_loss = abs(float(got['out'][0]) - r['loss']) / abs(r['loss'])
    grad = (got['grad'] - base if accumulate else got['grad']).cpu().numpy()
    ratio64 = O.worst_ratio(grad, r['grad'])
    print(f'{name}: form {got["form"]} loss {float(got["out"][0])!r} fp64 {r["loss"]!r} rel err {e_loss:.2e}, per-class sums {e_sum:.2e} (bounds 1e-5)  '
          f'gradient: worst ratio to the per-link bound vs fp64 {ratio64:.2e}')
    assert e_loss <= 1e-5
    assert e_sum <= 1e-5
    # (accumulate: base + g rounds at the size of base, a few max|g|: some 1e-7 max|g|, 1e-3 of the bound's floor)
    assert ratio64 <= 1.0
    if src == 'g11':
        # image 1 is entirely 255: nothing in the loss, exactly nothing in the gradient
        assert not s[1].any()
        assert torch.equal(got['grad'][1], base[1]) if accumulate else not got['grad'][1].any()
    if fix is not None:
        gref = golden[fix + '|grad']
        ratio32 = O.worst_ratio(grad, gref)
        want = float(golden[fix + '|loss'])
        e_ref = abs(float(got['out'][0]) - want) / abs(want)
        print(f'{name}: vs the executed reference (fp32): loss rel err {e_ref:.2e}, gradient ratio to the bound {ratio32:.2e}; '
              f'the reference itself vs fp64: {O.worst_ratio(gref, r["grad"]):.2e}')
        assert e_ref <= 1e-5 and ratio32 <= 1.0


def test_zero_weights_give_exactly_zero(ops, inputs):
    """a low-resolution cell whose whole footprint has weight 0 receives exactly 0; all weights 0: loss 0, gradient exactly 0"""
    for src, gamma in (('x4', 2.0), ('g11', 0.5), ('x8c33', 0.0)):
        z, lab, w = inputs[src]
        got = run_sig(ops, z, lab, torch.zeros_like(w), O.focal_coef(z.shape[1]), gamma, 'mean', 1.0)
        assert float(got['out'][0]) == 0.0 and not got['grad'].any() and not got['sums'][:-3].any(), src
    z, lab, w = inputs['x4']
    w = w.clone()
    w[:, 20:44, 16:40] = 0.0                      # full-resolution rows 20..43, columns 16..39: cells (6..9, 5..8) see nothing else
    got = run_sig(ops, z, lab, w, O.focal_coef(6), 2.0, 'mean', 1.0)
    assert not got['grad'][:, :, 6:10, 5:9].any() and got['grad'][:, :, 3:5, 5:9].any()


def test_block_and_generic_forms_agree(ops, inputs):
    for name in ('x4_focal', 'x4_g05', 'x8_focal'):
        src, args, _, _ = case_args(inputs, name)
        blk = run_sig(ops, *args)
        gen = run_sig(ops, *args, generic=True)
        assert blk['form'] == FORMS[src] and gen['form'] == 0 and blk['slab'].shape != gen['slab'].shape
        n, C = args[0].shape[:2]
        a, b = blk['sums'].cpu(), gen['sums'].cpu()
        err = float(((a - b).abs() / a.abs().clamp_min(1e-300))[:n * C].max())
        ratio = O.worst_ratio(blk['grad'].cpu().numpy(), gen['grad'].cpu().numpy())
        print(f'{name}: sums, block form vs generic form: rel err {err:.2e} (bound 1e-12); gradient ratio to the bound {ratio:.2e}')
        assert err <= 1e-12 and torch.equal(a[n * C:], b[n * C:])
        assert ratio <= 1.0


@pytest.mark.parametrize('name', ['x4_focal', 'x8_focal', 'x8c33_g05', 'g2_bce'])
def test_two_runs_are_bit_identical_without_deterministic_mode(ops, inputs, name):
    assert not ops.is_deterministic()
    _, args, _, _ = case_args(inputs, name)
    a, b = run_sig(ops, *args), run_sig(ops, *args)
    for k in ('slab', 'counts', 'sums', 'out', 'grad'):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ the head
def build_head(loss_decode, **over):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    return build(dict(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                           c1_in_channels=8, c1_channels=4, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True),
                           align_corners=False, loss_decode=loss_decode), **over))


def head_losses(loss_decode, logits, label, weight, grad_scale=1.0, **over):
    from pfst_amd.engine import Tape, Var
    head = build_head(loss_decode, **over)
    z, tape = Var(logits.to(DEV), True), Tape()
    res = head.losses(z, label.to(DEV).unsqueeze(1).contiguous(), None if weight is None else weight.to(DEV), tape, grad_scale)
    tape.backward()
    torch.cuda.synchronize()
    return res, z.grad


CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
FOCAL = dict(type='FocalLoss', loss_weight=2.0, gamma=2.0, alpha=0.25, class_weight=CW6)


def test_head_with_a_loss_list_matches_the_reference(golden, inputs):
    logits, label, weight = inputs['x4']
    for key, w in (('head', None), ('head_w', weight)):
        res, grad = head_losses([CE, FOCAL], logits, label, w)
        assert list(res) == ['loss_ce', 'loss_focal', 'acc_seg', '_bad_labels']
        names = ['loss_ce', 'loss_focal'] + (['acc_seg'] if key == 'head' else [])
        for k, want in zip(names, golden[key + '|values']):
            got = float(res[k])
            print(f'{key} {k}: {got!r} reference {float(want)!r} rel err {abs(got - want) / abs(want):.2e}')
            assert abs(got - want) <= 1e-5 * abs(want)
        assert float(res['_bad_labels']) == 0.0
        ratio = O.worst_ratio(grad.cpu().numpy(), golden[key + '|grad'])
        print(f'{key} d logits: worst ratio to the per-link bound {ratio:.2e}')
        assert ratio <= 1.0
    # unlike Dice, the sigmoid terms honour the pixel weights
    res2, _ = head_losses([CE, FOCAL], logits, label, weight * 0.5)
    assert not torch.equal(res2['loss_focal'], res['loss_focal']) and not torch.equal(res2['loss_ce'], res['loss_ce'])
    assert abs(float(res2['loss_focal']) - 0.5 * float(res['loss_focal'])) <= 1e-6 * float(res['loss_focal'])


def test_acc_seg_is_bit_equal_whichever_losses_are_listed(inputs):
    bce = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)
    for src in ('x4', 'x8bad'):
        logits, label, weight = inputs[src]
        ce, g_ce = head_losses(CE, logits, label, weight)
        focal, g_f = head_losses(FOCAL, logits, label, weight)
        both, g_both = head_losses([CE, FOCAL], logits, label, weight)
        rev, _ = head_losses([FOCAL, CE], logits, label, weight)
        sig, _ = head_losses(bce, logits, label, weight)
        three, _ = head_losses([FOCAL, dict(type='DiceLoss'), bce], logits, label, weight)
        for other in (focal, both, rev, sig, three):
            assert torch.equal(ce['acc_seg'], other['acc_seg'])
        assert 0.0 < float(ce['acc_seg']) < 100.0
        assert list(three) == ['loss_focal', 'loss_dice', 'loss_ce', 'acc_seg', '_bad_labels']
        # the label of 7 at C = 6 surfaces in every head's bad-label count
        assert all((float(r['_bad_labels']) > 0) == (src == 'x8bad') for r in (ce, focal, both, sig))
        assert torch.equal(both['loss_focal'], rev['loss_focal']) and torch.equal(both['loss_ce'], rev['loss_ce'])
        assert torch.equal(both['loss_focal'], focal['loss_focal']) and torch.equal(both['loss_ce'], ce['loss_ce'])
        # a Dice term after the sigmoid terms forms its own log-sum-exp: the value of a Dice-only head
        dice, _ = head_losses(dict(type='DiceLoss'), logits, label, weight)
        assert torch.equal(three['loss_dice'], dice['loss_dice'])
        assert O.worst_ratio(g_both.cpu().numpy(), g_ce.double().cpu().numpy() + g_f.double().cpu().numpy()) <= 1.0


def test_the_sampler_feeds_a_sigmoid_ce_term(inputs):
    """OHEMPixelSampler(thresh) + CrossEntropyLoss(use_sigmoid=True): the map comes from the softmax of the logits, as for a softmax CE head,
    and multiplies the term as pixel weights"""
    logits, label, weight = inputs['x4']
    sampler = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=200)
    bce = dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)
    head = build_head(bce, sampler=sampler)
    smap = head.sampler.sample(logits.to(DEV), label.to(DEV).unsqueeze(1).contiguous())
    ce_head = build_head(CE, sampler=sampler)
    assert torch.equal(smap, ce_head.sampler.sample(logits.to(DEV), label.to(DEV).unsqueeze(1).contiguous()))
    assert 0 < int(smap.sum()) < smap.numel()
    res, grad = head_losses(bce, logits, label, weight, sampler=sampler)         # the sampler's map replaces `weight`
    want = O.sigmoid_loss(logits, label, SIZES['x4'], O.bce_coef(6), 0.0, smap.cpu())
    assert abs(float(res['loss_ce']) - want['loss']) <= 1e-5 * want['loss']
    assert O.worst_ratio(grad.cpu().numpy(), want['grad']) <= 1.0
