"""LovaszLoss fused with the decode head's bilinear up-sampling (csrc/lovasz_loss.hip): the segmented radix sort on its own against
numpy.argsort(kind='stable'), and the loss, acc_seg and gradient against tests/lovasz_oracle.py (fp64, the kernels' tie rule) at the cases of
tests/golden/lovasz_loss.npz.

Bounds (the form of tests/test_dice_loss_gpu.py): the loss within 1e-5 relative of fp64; the gradient per element |hip - oracle| <= 1e-4
max|oracle| + 1e-3 |oracle| outside the oracle's mask of cells whose gradient fp32 does not determine (at most 5 % of the cells: asserted;
masked cells must be finite and below twice the largest oracle gradient).  For scale, the executed reference's own fp32 run sits at 7e-9 ..
5e-8 (loss) and 0.005 .. 0.17 of the gradient bound from the oracle on these inputs (tests/test_lovasz_cpu.py prints them).  acc_seg within
1e-5 relative of the oracle's (an fp32 rounding of the ratio; no arg-max of these inputs is tied to fp32 resolution)."""
import os

import numpy as np
import pytest
import torch

import lovasz_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
# name: (inputs, options, generic route forced, shared lse, accumulate)
CASES = {
    'x4': ('x4', dict(), False, True, False),
    'x4_generic': ('x4', dict(), True, False, True),
    'x4_all': ('x4', dict(classes='all', class_weight=CW6), False, False, True),
    'x4_img': ('x4', dict(per_image=True, reduction='mean'), False, True, False),
    'x4_img_sum': ('x4', dict(per_image=True, reduction='sum'), False, False, False),
    'x8': ('x8', dict(classes=[1, 4]), False, True, True),
    'g11': ('g11', dict(), False, False, False),
}
FORMS = {'x4': 4, 'x4_all': 4, 'x4_img': 4, 'x4_img_sum': 4, 'x8': 8}
POISON = 0x5A5A5A5A


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'lovasz_loss.npz'))


@pytest.fixture(scope='module')
def inputs(golden):
    return {src: (torch.from_numpy(golden[src + '|logits']), torch.from_numpy(golden[src + '|label'])) for src in ('x4', 'x8', 'g11')}


@pytest.fixture(scope='module')
def oracle(inputs):
    """the fp64 oracle of every distinct (inputs, options), computed once"""
    out = {}
    for name, (src, opts, _, _, _) in CASES.items():
        if name != 'x4_generic':
            logits, label = inputs[src]
            out[name] = O.lovasz_oracle(logits, label, tuple(label.shape[-2:]), **opts)
    out['x4_generic'] = out['x4']
    return out


# ------------------------------------------------------------------------------------------------------------------ the sort alone
def sort_case(ops, keys, lens):
    """keys uint32 [S, stride], lens per segment -> checks keys_out / the permutation of every segment and the untouched rest"""
    s, stride = keys.shape
    kd = torch.from_numpy(keys.view(np.int32)).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    canary = 64
    ko = torch.full((s * stride + canary,), POISON, dtype=torch.int32, device=DEV)
    vo = torch.full((s * stride + canary,), POISON, dtype=torch.int32, device=DEV)
    ops.lovasz_sort(kd, ld, out=(ko, vo))
    torch.cuda.synchronize()
    ko, vo = ko.cpu().numpy().view(np.uint32), vo.cpu().numpy().view(np.uint32)
    assert (ko[s * stride:] == POISON).all() and (vo[s * stride:] == POISON).all(), 'canary after the output buffers'
    for i, n in enumerate(lens):
        seg_k, seg_v = ko[i * stride:(i + 1) * stride], vo[i * stride:(i + 1) * stride]
        want = np.argsort(keys[i, :n], kind='stable')
        assert np.array_equal(seg_v[:n], want.astype(np.uint32)), f'segment {i} (length {n}): permutation'
        assert np.array_equal(seg_k[:n], keys[i, :n][want]), f'segment {i} (length {n}): keys'
        assert (seg_k[n:] == POISON).all() and (seg_v[n:] == POISON).all(), f'segment {i}: nothing is written at or beyond its length'
    return vo


@pytest.mark.parametrize('pattern', ['random', 'equal', 'top_digit', 'bottom_digit', 'errors'])
def test_sort_against_numpy_stable_argsort(ops, pattern):
    """one launch, six segments: lengths 0, 1, 255, 256, 257 and three workgroups (4096 elements each) plus a ragged tail"""
    stride = 3 * 4096 + 123
    lens = [0, 1, 255, 256, 257, stride]
    rng = np.random.default_rng(7)
    raw = rng.integers(0, 2 ** 32, size=(len(lens), stride), dtype=np.uint64).astype(np.uint32)
    if pattern == 'equal':
        keys = np.full_like(raw, 0x3F000000)
    elif pattern == 'top_digit':
        keys = (raw & np.uint32(0xFF000000)) | np.uint32(0x00123456)
    elif pattern == 'bottom_digit':
        keys = (raw & np.uint32(0x000000FF)) | np.uint32(0x3E123400)
    elif pattern == 'errors':          # the loss's keys: 0x3F800000 - bits(e), e in [0, 1] with many exact ties, and the invalid key
        e = (rng.integers(0, 64, size=raw.shape) / 63.0).astype(np.float32)
        keys = np.uint32(0x3F800000) - e.view(np.uint32)
        keys[raw % 5 == 0] = 0x3F800001
    else:
        keys = raw
    perm = sort_case(ops, keys, lens)
    if pattern == 'equal':
        assert np.array_equal(perm[5 * stride:6 * stride], np.arange(stride, dtype=np.uint32)), 'all keys equal: the identity'


def test_sort_full_segments_carry_values_and_work_in_place(ops):
    rng = np.random.default_rng(11)
    s, stride = 2, 4096 + 77
    keys = rng.integers(0, 1 << 30, size=(s, stride), dtype=np.int64).astype(np.int32)
    vals = rng.integers(0, 1 << 31, size=(s, stride), dtype=np.int64).astype(np.int32)
    kd, vd = torch.from_numpy(keys).to(DEV), torch.from_numpy(vals).to(DEV)
    ko, vo = ops.lovasz_sort(kd, None, vals=vd)
    ops.lovasz_sort(kd, None, vals=vd, out=(kd, vd))          # in place
    torch.cuda.synchronize()
    for i in range(s):
        want = np.argsort(keys[i], kind='stable')
        assert np.array_equal(ko[i].cpu().numpy(), keys[i][want]) and np.array_equal(vo[i].cpu().numpy(), vals[i][want])
    assert torch.equal(kd, ko) and torch.equal(vd, vo)


# ------------------------------------------------------------------------------------------------------------------ the loss
def run_lovasz(ops, logits, label, opts, generic=False, shared=False, accumulate=False, base=None, loss_weight=1.0, want_sorted=False):
    ld, l8 = logits.to(DEV), label.to(DEV)
    C = ld.shape[1]
    classes = opts.get('classes', 'present')
    slot, cls = ops.lovasz_class_tables(classes, C, DEV)
    cw = opts.get('class_weight')
    sw = None if cw is None else torch.tensor([cw[c] for c in cls.tolist()], dtype=torch.float32, device=DEV)
    lse_ce, acc_ce = ops.ce_upsample_fwd(ld, l8)
    r = ops.lovasz_upsample_fwd(ld, l8, slot, cls, sw, 255, opts.get('per_image', False), classes == 'present',
                                'sum' if opts.get('reduction') == 'sum' else 'mean', loss_weight, lse=lse_ce if shared else None,
                                generic=generic, want_sorted=want_sorted)
    args = (ld, l8, slot, cls, r['lse'], r['map'], r['scale'], loss_weight, 255)
    if accumulate:
        grad = ops.lovasz_upsample_bwd(*args, out=base.clone(), accumulate=True, generic=generic)
    else:
        grad = ops.lovasz_upsample_bwd(*args, generic=generic)
    torch.cuda.synchronize()
    r.update(grad=grad, lse_ce=lse_ce, acc_ce=ops.ce_finalize(acc_ce, label.numel(), 1.0))
    return r


def check_against(name, got_out, grad, ref):
    mask = ref['mask']
    frac = float(mask.float().mean())
    e_loss = abs(float(got_out[0]) - ref['loss']) / abs(ref['loss'])
    e_acc = abs(float(got_out[1]) - ref['acc_seg']) / ref['acc_seg']
    ratio = O.link_ratio(grad, ref['grad'], ~mask.unsqueeze(1))
    gmax = float(ref['grad'].abs().max())
    print(f'{name}: loss {float(got_out[0])!r} fp64 {ref["loss"]!r} rel err {e_loss:.2e} (bound 1e-5); acc_seg rel err {e_acc:.2e}; masked cells '
          f'{int(mask.sum())} of {mask.numel()}; gradient: worst ratio to the per-link bound {ratio:.2e}, max |grad| {float(grad.abs().max()):.3e} '
          f'oracle {gmax:.3e}')
    assert frac <= O.MASK_CAP, 'the cap on masked cells is a condition of the test'
    assert e_loss <= 1e-5 and e_acc <= 1e-5
    assert float(got_out[2]) == ref['bad']
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) <= 2.0 * gmax
    assert ratio <= 1.0


@pytest.mark.parametrize('name', list(CASES))
def test_loss_and_gradient_against_the_oracle(ops, golden, inputs, oracle, name):
    src, opts, generic, shared, accumulate = CASES[name]
    logits, label = inputs[src]
    ref = oracle[name]
    assert ops.lovasz_form(logits.to(DEV), label.to(DEV), None, generic) == FORMS.get(name, 0)
    base = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5)).to(DEV) * float(ref['grad'].abs().max())
    got = run_lovasz(ops, logits, label, opts, generic, shared, accumulate, base=base)
    grad = got['grad'] - base if accumulate else got['grad']
    check_against(name, got['out'].cpu(), grad.cpu(), ref)
    # own and shared log-sum-exp: the same bits, and the same result
    other = run_lovasz(ops, logits, label, opts, generic, not shared, accumulate, base=base)
    assert torch.equal(got['lse'], other['lse']) and torch.equal(got['lse'], got['lse_ce'])
    assert torch.equal(got['out'], other['out']) and torch.equal(got['grad'], other['grad'])
    # acc_seg: the CE term's bits
    assert torch.equal(got['out'][1], got['acc_ce'][1])
    if name == 'x4':
        n, k = 2, 6
        G = got['counters'][3:].view(n, k).cpu()
        lab = label.long()
        assert G.tolist() == [[int((lab[i] == c).sum()) for c in range(k)] for i in range(n)] and int(G[0, 3]) == 0, 'class 3 is absent from image 0'
    gname = 'x4' if name == 'x4_generic' else name
    e_ref = abs(float(got['out'][0]) - float(golden[gname + '|loss'])) / abs(float(golden[gname + '|loss']))
    r32 = O.link_ratio(grad, torch.from_numpy(golden[gname + '|grad']), ~ref['mask'].unsqueeze(1))
    print(f'{name}: vs the executed reference (fp32): loss rel err {e_ref:.2e}, gradient ratio to the bound {r32:.2e}')
    assert e_ref <= 1e-5 and r32 <= 1.0


def test_block_and_generic_routes_agree(ops, inputs):
    logits, label = inputs['x4']
    blk = run_lovasz(ops, logits, label, dict(), want_sorted=True)
    gen = run_lovasz(ops, logits, label, dict(), generic=True, want_sorted=True)
    assert blk['form'] == 4 and gen['form'] == 0
    # the same interpolation and class order: the same keys, hence the same order and the same sums
    assert torch.equal(blk['lse'], gen['lse']) and torch.equal(blk['keys'], gen['keys']) and torch.equal(blk['vals'], gen['vals'])
    assert torch.equal(blk['sums'], gen['sums']) and torch.equal(blk['out'], gen['out']) and torch.equal(blk['counters'], gen['counters'])
    assert O.link_ratio(blk['grad'], gen['grad']) <= 1.0


def test_exactly_tied_errors_follow_the_raster_rule(ops, inputs):
    """all logits zero: every error is 1/6 or 5/6, in fp32 and in fp64 alike; the loss has a closed form and the gradient is the oracle's under
    the tie rule (ascending pixel index), with no mask"""
    _, label = inputs['x4']
    logits = torch.zeros(2, 6, 19, 17)
    ref = O.lovasz_oracle(logits, label, (76, 68))
    assert int(ref['mask'].sum()) == 0 and abs(ref['loss'] - O.closed_form_uniform(label, 6)) <= 1e-12
    for generic in (False, True):
        got = run_lovasz(ops, logits, label, dict(), generic=generic, want_sorted=True)
        e = abs(float(got['out'][0]) - 5.0 / 6.0) / (5.0 / 6.0)
        ratio = O.link_ratio(got['grad'], ref['grad'])
        print(f'tied, generic={generic}: loss {float(got["out"][0])!r} closed form {5 / 6!r} rel err {e:.2e}; gradient ratio {ratio:.2e}')
        assert e <= 1e-6 and ratio <= 1.0
        # within a class: foreground (5/6) first, then background (1/6), each run in ascending pixel index; then the pixels under 255
        keys, vals = got['keys'].cpu().numpy().view(np.uint32), got['vals'].cpu().numpy().view(np.uint32)
        lab = label.reshape(-1).numpy()
        for c in range(6):
            idx = np.arange(lab.size)
            want = np.concatenate([idx[lab == c], idx[(lab != c) & (lab != 255)], idx[lab == 255]])
            assert np.array_equal(vals[c] & 0x7FFFFFFF, want.astype(np.uint32)), c
            assert np.array_equal(vals[c] >> 31, (lab[want] == c).astype(np.uint32)), c


def test_degenerate_inputs(ops, inputs):
    logits, label = inputs['x4']
    # no valid pixel at all: loss 0, gradient exactly 0, under 'present' and under 'all'
    none = torch.full_like(label, 255)
    for opts in (dict(), dict(classes='all'), dict(per_image=True, reduction='sum')):
        got = run_lovasz(ops, logits, none, opts)
        assert float(got['out'][0]) == 0.0 and float(got['out'][2]) == 0.0 and bool(torch.isfinite(got['out']).all())
        assert float(got['grad'].abs().max()) == 0.0
    # per_image with image 1 all 255: it adds 0 and still counts in the divisor N
    half = label.clone()
    half[1] = 255
    for red in ('mean', 'sum'):
        opts = dict(per_image=True, reduction=red)
        ref = O.lovasz_oracle(logits, half, (76, 68), **opts)
        got = run_lovasz(ops, logits, half, opts)
        check_against(f'image 1 all 255, {red}', got['out'].cpu(), got['grad'].cpu(), ref)
        assert float(got['grad'][1].abs().max()) == 0.0
    one = run_lovasz(ops, logits, half, dict(per_image=True, reduction='mean'))
    img0 = run_lovasz(ops, logits[:1], label[:1], dict(per_image=True, reduction='mean'))
    assert abs(float(one['out'][0]) - 0.5 * float(img0['out'][0])) <= 1e-6 * float(one['out'][0])
    # 'present' with one class present
    single = torch.where(label == 255, label, torch.full_like(label, 2))
    ref = O.lovasz_oracle(logits, single, (76, 68))
    got = run_lovasz(ops, logits, single, dict())
    check_against('one class present', got['out'].cpu(), got['grad'].cpu(), ref)
    assert got['scale'].cpu().tolist() == [[0.0, 0.0, 1.0, 0.0, 0.0, 0.0]] * 2
    # a bad label (7 at C = 6): counted once, a valid pixel that is foreground for no class
    bad = label.clone()
    bad[0, 40:44, 40:44] = 7
    ref = O.lovasz_oracle(logits, bad, (76, 68))
    got = run_lovasz(ops, logits, bad, dict())
    assert ref['bad'] == 16
    check_against('bad label', got['out'].cpu(), got['grad'].cpu(), ref)


@pytest.mark.parametrize('name', ['x4', 'x4_img', 'g11'])
def test_two_runs_are_bit_identical_without_deterministic_mode(ops, inputs, name):
    assert not ops.is_deterministic()
    src, opts, generic, shared, _ = CASES[name]
    a = run_lovasz(ops, *inputs[src], opts, generic, shared, want_sorted=True)
    b = run_lovasz(ops, *inputs[src], opts, generic, shared, want_sorted=True)
    for k in ('keys', 'vals', 'sums', 'counters', 'scale', 'out', 'grad', 'lse'):
        assert torch.equal(a[k], b[k]), k


def test_an_offset_view_is_its_dense_copy_and_a_strided_view_is_refused(ops, inputs):
    """the loss family reads dense logits (as ce_upsample_fwd): a contiguous view at an offset into a larger buffer -- odd, so neither 8- nor
    16-byte aligned -- gives the bits of its dense copy; a view with strides is refused before any launch"""
    logits, label = inputs['x4']
    dense = run_lovasz(ops, logits, label, dict())
    big = torch.zeros(logits.numel() + 5, device=DEV)
    view = big[3:3 + logits.numel()].view(logits.shape)
    view.copy_(logits)
    slot, cls = ops.lovasz_class_tables('present', 6, DEV)
    l8 = label.to(DEV)
    r = ops.lovasz_upsample_fwd(view, l8, slot, cls)
    grad = ops.lovasz_upsample_bwd(view, l8, slot, cls, r['lse'], r['map'], r['scale'], 1.0)
    assert torch.equal(r['out'], dense['out']) and torch.equal(grad, dense['grad'])
    wide = torch.zeros(2, 8, 19, 17, device=DEV)
    with pytest.raises(ValueError, match='contiguous'):
        ops.lovasz_upsample_fwd(wide[:, :6], l8, slot, cls)
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.lovasz_upsample_fwd(logits, l8, slot, cls)


# ------------------------------------------------------------------------------------------------------------------ the head
def head_losses(loss_decode, logits, label, weight, grad_scale=1.0):
    import pfst_amd  # noqa: F401
    from pfst_amd.engine import Tape, Var
    from pfst_amd.registry import build_head
    head = build_head(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                           c1_in_channels=8, c1_channels=4, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True),
                           align_corners=False, loss_decode=loss_decode))
    z, tape = Var(logits.to(DEV), True), Tape()
    res = head.losses(z, label.to(DEV).unsqueeze(1).contiguous(), None if weight is None else weight.to(DEV), tape, grad_scale)
    ops_on_tape = [tag['op'] for _, tag in tape.fns]
    tape.backward()
    torch.cuda.synchronize()
    return res, z.grad, ops_on_tape


CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
LV = dict(type='LovaszLoss', loss_weight=2.0, reduction='none')


def test_head_with_a_loss_list_matches_the_reference(golden, inputs):
    logits, label = inputs['x4']
    weight = torch.from_numpy(golden['x4|weight_blocks']).repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    res, grad, tags = head_losses([CE, LV], logits, label, weight)
    assert list(res) == list(golden['head|names']) + ['_bad_labels'] == ['loss_ce', 'loss_lovasz', 'acc_seg', '_bad_labels']
    assert tags == ['ce', 'lovasz']
    for k, want in zip(golden['head|names'], golden['head|values']):
        got = float(res[k])
        print(f'head {k}: {got!r} reference {float(want)!r} rel err {abs(got - want) / abs(want):.2e}')
        assert abs(got - want) <= 1e-5 * abs(want)
    assert float(res['_bad_labels']) == 0.0
    ratio = O.link_ratio(grad, torch.from_numpy(golden['head|grad']))
    print(f'head d logits: worst ratio to the per-link bound {ratio:.2e}')
    assert ratio <= 1.0
    # pixel weights and their absence: bit-equal Lovasz results, a different CE
    res2, _, _ = head_losses([CE, LV], logits, label, weight * 0.5)
    assert torch.equal(res2['loss_lovasz'], res['loss_lovasz']) and not torch.equal(res2['loss_ce'], res['loss_ce'])
    a, ga, _ = head_losses(LV, logits, label, weight)
    b, gb, _ = head_losses(LV, logits, label, None)
    assert torch.equal(a['loss_lovasz'], b['loss_lovasz']) and torch.equal(a['loss_lovasz'], res['loss_lovasz']) and torch.equal(ga, gb)
    # acc_seg: the same bits whichever terms are listed, in either order
    ce, _, _ = head_losses(CE, logits, label, None)
    rev, _, _ = head_losses([LV, CE], logits, label, weight)
    assert torch.equal(ce['acc_seg'], a['acc_seg']) and torch.equal(ce['acc_seg'], res['acc_seg']) and torch.equal(ce['acc_seg'], rev['acc_seg'])
    assert torch.equal(rev['loss_lovasz'], res['loss_lovasz']) and torch.equal(rev['loss_ce'], res['loss_ce'])
    # grad_scale scales the gradient and nothing else
    c, gc, _ = head_losses(LV, logits, label, None, grad_scale=0.25)
    assert torch.equal(c['loss_lovasz'], b['loss_lovasz']) and float((gc - 0.25 * gb).abs().max()) <= 1e-6 * float(gb.abs().max())
