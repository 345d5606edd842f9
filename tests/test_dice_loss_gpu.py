"""DiceLoss fused with the decode head's bilinear up-sampling (csrc/dice_loss.hip) against fp64 autograd of the literal formula and against
the executed reference (tests/golden/dice_loss.npz, written by tests/golden/make_golden_dice.py); the loss lists of BaseDecodeHead.

Bounds: gradients per element |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref| (the per-link bound) against fp64 and against the
reference's fp32; the loss within 1e-5 relative of fp64, on inputs whose every term 1 - num/den is >= 0.1 (the cancellation then amplifies
soft-max rounding by at most 10).  For scale: the reference's own fp32 path sits 3e-8 (loss) and 2e-7 of the maximum (gradients) from fp64.
Measured on an MI355X (worst case over the six cases): loss 5.2e-8 relative, gradient 1.4e-3 of the bound and 4.2e-7 of the maximum --
beside the executed reference's own fp32 gradient, which sits at 4e-4 .. 1.5e-3 of the bound from fp64 on the same inputs."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
# name: (C, (H, W), DiceLoss options, shared lse, accumulate)         -- the options of tests/golden/make_golden_dice.py's CASES
CASES = {
    'x4': (6, (76, 68), dict(), True, False),
    'x8': (6, (136, 144), dict(exponent=3, smooth=0.5, class_weight=CW6), False, True),
    'x8c33': (33, (136, 144), dict(ignore_index=2, class_weight=[0.5 + 0.05 * i for i in range(33)]), True, False),
    'g11': (11, (30, 37), dict(exponent=3), False, True),
    'g2': (2, (30, 37), dict(smooth=0.5, class_weight=[0.6, 1.4]), True, False),
    # not in the fixture: the block form with a class index as ignore_index (the x4 inputs), against fp64 only
    'x4_ign2': (6, (76, 68), dict(ignore_index=2, class_weight=CW6), False, True),
}


def make_c33(base):
    return torch.stack([base[:, c % 6] * (1.0 + (c // 6) / 8.0) + (c // 6) / 4.0 for c in range(33)], 1).contiguous()


def dice_ref64(logits, label, C, size, smooth=1, exponent=2, class_weight=None, ignore_index=255, loss_weight=1.0):
    """the formula of DESIGN.md section 8h, literally, in fp64 with autograd"""
    z = logits.double().clone().requires_grad_()
    p = F.softmax(F.interpolate(z, size=size, mode='bilinear', align_corners=False), dim=1)
    lab = label.long()
    t = F.one_hot(lab.clamp(0, C - 1), C).permute(0, 3, 1, 2).double()
    valid = (lab != ignore_index).double().unsqueeze(1)
    I = (valid * t * p).flatten(2).sum(2)
    P = p.pow(exponent).flatten(2).sum(2)
    T = t.flatten(2).sum(2)
    num, den = 2 * I + smooth, P + T + smooth
    term = 1 - num / den
    cw = torch.ones(C, dtype=torch.float64) if class_weight is None else torch.tensor(class_weight, dtype=torch.float64)
    loss = loss_weight / C * sum(cw[c] * term[:, c].mean() for c in range(C) if c != ignore_index)
    loss.backward()
    return dict(loss=float(loss.detach()), grad=z.grad, I=I.detach(), P=P.detach(), T=T.detach(), term=term.detach())


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'dice_loss.npz'))


@pytest.fixture(scope='module')
def inputs(golden):
    """{case: (logits, label uint8)} on the CPU, and the fp64 reference of every case, computed once"""
    out = {}
    for name in CASES:
        src = 'x4' if name == 'x4_ign2' else name
        logits = make_c33(torch.from_numpy(golden['x8|logits'])) if name == 'x8c33' else torch.from_numpy(golden[src + '|logits'])
        out[name] = (logits, torch.from_numpy(golden[src + '|label']))
    return out


@pytest.fixture(scope='module')
def ref64(inputs):
    return {name: dice_ref64(*inputs[name], C, size, **opts) for name, (C, size, opts, _, _) in CASES.items()}


def link_ratio(got, ref):
    """max over the elements of |got - ref| / (1e-4 max|ref| + 1e-3 |ref|): within the per-link bound iff <= 1"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (1e-4 * ref.abs().max() + 1e-3 * ref.abs())).max())


def run_dice(ops, logits, label, C, opts, shared, accumulate=False, generic=False, base=None, loss_weight=1.0):
    ld, l8 = logits.to(DEV), label.to(DEV)
    ign, e = opts.get('ignore_index', 255), float(opts.get('exponent', 2))
    cw = None if opts.get('class_weight') is None else torch.tensor(opts['class_weight'], dtype=torch.float32, device=DEV)
    lse_ce, acc_ce = ops.ce_upsample_fwd(ld, l8)
    slab, counts, lse, form = ops.dice_upsample_fwd(ld, l8, ign, 255, e, lse=lse_ce if shared else None, generic=generic)
    out, coef, sums = ops.dice_finalize(slab, counts, cw, ign, opts.get('smooth', 1), e, loss_weight)
    if accumulate:
        grad = ops.dice_upsample_bwd(ld, l8, lse, coef, loss_weight, ign, e, out=base.clone(), accumulate=True, generic=generic)
    else:
        grad = ops.dice_upsample_bwd(ld, l8, lse, coef, loss_weight, ign, e, generic=generic)
    torch.cuda.synchronize()
    return dict(out=out, coef=coef, sums=sums, slab=slab, counts=counts, lse=lse, lse_ce=lse_ce, acc_ce=acc_ce, grad=grad, form=form)


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


@pytest.mark.parametrize('name', list(CASES))
def test_dice_kernels_against_fp64_and_the_reference(ops, golden, inputs, ref64, name):
    C, size, opts, shared, accumulate = CASES[name]
    logits, label = inputs[name]
    r = ref64[name]
    # the inputs keep the cancellation in 1 - num/den below a factor of 10
    assert float(r['term'].min()) >= 0.1, float(r['term'].min())
    assert ops.dice_form(logits.to(DEV), label.to(DEV))[0] == {'x4': 4, 'x4_ign2': 4, 'x8': 8}.get(name, 0)
    base = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).to(DEV) * float(r['grad'].abs().max())
    got = run_dice(ops, logits, label, C, opts, shared, accumulate, base=base)
    n = logits.shape[0]
    sums = got['sums'].cpu()
    I, P, T = (sums[:n * C * 3].view(n, C, 3)[..., i] for i in range(3))
    # exact: T; the accuracy counts as the CE kernels count them; the bad labels as the label map holds them
    assert torch.equal(T, r['T']), 'T'
    if name == 'x4':
        assert float(T[0, 3]) == 0.0 and float(I[0, 3]) == 0.0, 'class 3 is absent from image 0'
    if name == 'g11':
        assert float(I[1].abs().max()) == 0.0 and float(T[1, C - 1]) == size[0] * size[1], 'image 1 is entirely 255'
    lab = label.long()
    ign = opts.get('ignore_index', 255)
    want_bad = int(((lab >= C) & (lab != 255) & (lab != ign)).sum())
    assert (want_bad > 0) == (name == 'x8')
    acc_ce = got['acc_ce'].cpu()
    assert sums[n * C * 3:].tolist() == [float(acc_ce[1]), float(acc_ce[2]), float(want_bad)], (sums[n * C * 3:], acc_ce)
    assert float(got['out'][2]) == want_bad
    assert float(acc_ce[3]) == int(((lab >= C) & (lab != 255)).sum())
    # own and shared log-sum-exp: the same bits
    other = run_dice(ops, logits, label, C, opts, not shared, accumulate, base=base)
    assert torch.equal(got['lse'], other['lse']) and torch.equal(got['slab'], other['slab']) and torch.equal(got['grad'], other['grad'])
    assert torch.equal(got['out'], other['out'])
    # I, P and the loss against fp64
    e_sum = max(float(((I - r['I']).abs() / r['I'].abs().clamp_min(1.0)).max()), float(((P - r['P']).abs() / r['P'].abs()).max()))
    e_loss = abs(float(got['out'][0]) - r['loss']) / abs(r['loss'])
    grad = got['grad'] - base if accumulate else got['grad']
    ratio64 = link_ratio(grad, r['grad'])
    e_max = float((grad.double().cpu() - r['grad']).abs().max() / r['grad'].abs().max())
    print(f'{name}: form {got["form"]} I/P rel err {e_sum:.2e}  loss {float(got["out"][0])!r} fp64 {r["loss"]!r} rel err {e_loss:.2e} (bound 1e-5)  '
          f'gradient: worst ratio to the per-link bound vs fp64 {ratio64:.2e}, max err / max {e_max:.2e}')
    assert e_loss <= 1e-5
    assert ratio64 <= 1.0
    if name + '|grad' in golden.files:
        gref = torch.from_numpy(golden[name + '|grad'])
        ratio32 = link_ratio(grad, gref)
        e_ref = abs(float(got['out'][0]) - float(golden[name + '|loss'])) / abs(float(golden[name + '|loss']))
        print(f'{name}: vs the executed reference (fp32): loss rel err {e_ref:.2e}, gradient ratio to the bound {ratio32:.2e}; '
              f'the reference itself vs fp64: {link_ratio(gref, r["grad"]):.2e}')
        assert ratio32 <= 1.0 and e_ref <= 1e-5


def test_block_and_generic_forms_agree(ops, inputs):
    """the x4 shape through the generic kernels (the wrapper's test-only switch): lse bit for bit, the slab sums to 1e-12"""
    C, size, opts, _, _ = CASES['x4_ign2']
    logits, label = inputs['x4_ign2']
    blk = run_dice(ops, logits, label, C, opts, shared=False)
    gen = run_dice(ops, logits, label, C, opts, shared=False, generic=True)
    assert blk['form'] == 4 and gen['form'] == 0 and blk['slab'].shape != gen['slab'].shape
    assert torch.equal(blk['lse'], gen['lse']) and torch.equal(blk['lse'], blk['lse_ce'])
    n = logits.shape[0]
    a, b = blk['sums'].cpu(), gen['sums'].cpu()
    err = float(((a - b).abs() / a.abs().clamp_min(1e-300))[:n * C * 3].max())
    print(f'slab sums, block form vs generic form: rel err {err:.2e} (bound 1e-12)')
    assert err <= 1e-12 and torch.equal(a[n * C * 3:], b[n * C * 3:])
    assert torch.equal(a.view(-1)[2:n * C * 3:3], b.view(-1)[2:n * C * 3:3]), 'T'
    assert link_ratio(blk['grad'], gen['grad']) <= 1.0


@pytest.mark.parametrize('name', ['x4', 'x8c33'])
def test_two_runs_are_bit_identical_without_deterministic_mode(ops, inputs, name):
    assert not ops.is_deterministic()
    C, size, opts, shared, _ = CASES[name]
    a = run_dice(ops, *inputs[name], C, opts, shared)
    b = run_dice(ops, *inputs[name], C, opts, shared)
    for k in ('slab', 'counts', 'sums', 'coef', 'out', 'grad', 'lse'):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------------------------ the head
def build_head(loss_decode):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    return build(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                      c1_in_channels=8, c1_channels=4, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True),
                      align_corners=False, loss_decode=loss_decode))


def head_losses(loss_decode, logits, label, weight, grad_scale=1.0):
    from pfst_amd.engine import Tape, Var
    head = build_head(loss_decode)
    z, tape = Var(logits.to(DEV), True), Tape()
    res = head.losses(z, label.to(DEV).unsqueeze(1).contiguous(), None if weight is None else weight.to(DEV), tape, grad_scale)
    tape.backward()
    torch.cuda.synchronize()
    return res, z.grad


CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)


def test_head_with_a_loss_list_matches_the_reference(golden, inputs):
    logits, label = inputs['x4']
    weight = torch.from_numpy(golden['head_weight_blocks']).repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    res, grad = head_losses([CE, dict(type='DiceLoss', loss_weight=3.0, class_weight=CW6)], logits, label, weight)
    assert list(res) == list(golden['head|names']) + ['_bad_labels'] == ['loss_ce', 'loss_dice', 'acc_seg', '_bad_labels']
    for k, want in zip(golden['head|names'], golden['head|values']):
        got = float(res[k])
        print(f'head {k}: {got!r} reference {float(want)!r} rel err {abs(got - want) / abs(want):.2e}')
        assert abs(got - want) <= 1e-5 * abs(want)
    assert float(res['_bad_labels']) == 0.0
    ratio = link_ratio(grad, torch.from_numpy(golden['head|grad']))
    print(f'head d logits: worst ratio to the per-link bound {ratio:.2e}')
    assert ratio <= 1.0
    # the Dice term ignores the pixel weights: loss_dice is the unweighted fixture's value x 3 x class weights -- and scaling them changes CE only
    res2, _ = head_losses([CE, dict(type='DiceLoss', loss_weight=3.0, class_weight=CW6)], logits, label, weight * 0.5)
    assert torch.equal(res2['loss_dice'], res['loss_dice']) and not torch.equal(res2['loss_ce'], res['loss_ce'])


def test_two_dice_terms_with_one_loss_name_are_added(inputs):
    logits, label = inputs['x4']
    one, g1 = head_losses([dict(type='DiceLoss', loss_weight=1.0)], logits, label, None)
    two, g2 = head_losses([dict(type='DiceLoss', loss_weight=2.0)], logits, label, None)
    both, g12 = head_losses([dict(type='DiceLoss', loss_weight=1.0), dict(type='DiceLoss', loss_weight=2.0)], logits, label, None)
    assert list(both) == ['loss_dice', 'acc_seg', '_bad_labels']
    assert abs(float(both['loss_dice']) - (float(one['loss_dice']) + float(two['loss_dice']))) <= 1e-6 * float(both['loss_dice'])
    assert link_ratio(g12, g1.double() + g2.double()) <= 1.0
    named, _ = head_losses([dict(type='DiceLoss', loss_weight=1.0), dict(type='DiceLoss', loss_weight=2.0, loss_name='loss_dice2')], logits, label, None)
    assert list(named) == ['loss_dice', 'loss_dice2', 'acc_seg', '_bad_labels'] and torch.equal(named['loss_dice2'], two['loss_dice'])


def test_acc_seg_is_bit_equal_whichever_losses_are_listed(inputs):
    for name in ('x4', 'x8'):
        logits, label = inputs[name]
        ce, _ = head_losses(CE, logits, label, None)
        dice, _ = head_losses(dict(type='DiceLoss'), logits, label, None)
        both, _ = head_losses([CE, dict(type='DiceLoss')], logits, label, None)
        rev, _ = head_losses([dict(type='DiceLoss'), CE], logits, label, None)
        assert torch.equal(ce['acc_seg'], dice['acc_seg']) and torch.equal(ce['acc_seg'], both['acc_seg']) and torch.equal(ce['acc_seg'], rev['acc_seg'])
        assert 0.0 < float(ce['acc_seg']) < 100.0
        # the label of 7 at C = 6 (x8) surfaces in every head's bad-label count
        assert (float(ce['_bad_labels']) > 0) == (float(dice['_bad_labels']) > 0) == (float(both['_bad_labels']) > 0) == (name == 'x8')
        # a Dice term behind a CE term reads its log-sum-exp; in front of it, it forms its own: the same bits either way
        assert torch.equal(both['loss_dice'], rev['loss_dice']) and torch.equal(both['loss_ce'], rev['loss_ce'])
