"""OHEMPixelSampler on the device (csrc/ohem.hip) against things that are not the code under test: the key map against the fp64 oracle
(tests/ohem_oracle.py), the select EXACTLY against torch.sort of that same key map on the device, the weight map against the fp64 oracle
outside a band around the cut, the head's loss and gradient against fp64 CE under the oracle's weights.

Bounds.  Keys: p within 2e-5 relative for |logit| <= 32 (three interpolation fmas: 3 * 2^-24 * 32 = 6e-6 in the exponent's argument = the
relative error of p; the sum, the division and expf add (C + 4) * 2^-24; 2e-5 is twice the total), nll within 2e-5 absolute.  The select has
no tolerance.  Weight map: a pixel may differ from the fp64 oracle only where its fp64 key lies within that key error of the fp64 cut (the
error of the pixel's key plus that of the cut, an order statistic of keys with the same error); the inputs keep that band below 0.25 % of the
valid pixels.  Head: loss 1e-5 relative, gradients by the per-link bound of tests/test_dice_loss_gpu.py.
Measured on an MI355X (worst case over all cases): p 5.6e-6 relative, nll 7.7e-6 absolute; at most 4 valid pixels in a band and no pixel,
inside or outside it, that differs from the fp64 oracle; head losses 5e-8 relative, gradients 5e-4 of the per-link bound."""
import numpy as np
import pytest
import torch

import ohem_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = 2
# name: (C, (h, w), (H, W))
SHAPES = {
    'x4': (6, (16, 16), (64, 64)),
    'x4r': (6, (19, 17), (76, 68)),          # crosses a tile edge, ends ragged (N H W = 10336: a float4 body, chunks that end inside a tile)
    'x8': (6, (8, 8), (64, 64)),             # clamped borders: runs of identical p, the cut lands inside a tie
    'g19': (19, (13, 9), (50, 37)),          # non-integer ratio, generic class walk; H W = 1850 is no multiple of 4
}
THRESH_CASES = ['thresh_wins', 'sk_wins', 'k_last', 'one_image_ignored', 'all_ignored', 'bad_label', 'saturated']
TOPK_CASES = ['random', 'constant', 'all_ignored', 'bad_label', 'keep_all']


def gen(seed):
    return torch.Generator().manual_seed(seed)


def make_case(shape, case, topk=False):
    """-> (logits [N, C, h, w], label uint8 [N, H, W], thresh | None, min_kept); every label map has a 255 region"""
    C, lo, hi = SHAPES[shape]
    g = gen(1000 + 17 * list(SHAPES).index(shape) + (100 if topk else 0))
    logits = torch.randn(N, C, *lo, generator=g) * 2
    label = torch.randint(0, C, (N, *hi), generator=g)
    thresh, min_kept = (None, 700) if topk else (0.7, 100)
    if case in ('sk_wins', 'k_last'):
        arg = O.upsample(logits, hi, torch.float64).argmax(1)
        label = torch.where(torch.rand(N, *hi, generator=g) < 0.9, arg, label)          # mostly the arg-max: few p below the threshold
        thresh, min_kept = 0.3, (1500 if case == 'sk_wins' else 5000)
    if case == 'saturated':
        logits = logits * 40                                                          # p reaches exactly 0 and exactly 1
    if case == 'constant':
        logits = torch.full_like(logits, 0.25)                                        # every valid key is equal: the tie fill decides everything
    if case == 'keep_all':
        min_kept = 5000                                                               # batch_kept > n_valid
    label[:, 5:14, 9:23] = 255
    if case == 'k_last':
        label[:, 40:48, :] = 255                                                      # n_valid <= batch_kept on every shape
    if case == 'one_image_ignored':
        label[1] = 255
    if case == 'all_ignored':
        label[:] = 255
    if case == 'bad_label':
        label[0, 20:24, 3:11] = 7 if C == 6 else 200
    return logits, label.to(torch.uint8), thresh, min_kept


@pytest.fixture(scope='module')
def ops():
    from pfst_amd import hip_ops
    return hip_ops


def run(ops, logits, label, thresh, min_kept, coef=None):
    C = logits.shape[1]
    cf = None
    if thresh is None:
        cf = torch.tensor([1.0] * C if coef is None else coef, dtype=torch.float32, device=DEV)
    w, info, keys = ops.ohem_sample(logits.to(DEV), label.to(DEV), 255, thresh, min_kept * N, cf, want_keys=True)
    torch.cuda.synchronize()
    return w, info, keys


def info_value(info):
    return info[0:1].to(torch.int32).view(torch.float32)


def check_keys(case, keys, k64, valid, topk):
    kc = keys.double().cpu()
    assert torch.equal(kc < 0, ~valid) and bool((kc[~valid] == -1).all()), 'the sentinel sits exactly at the pixels that are not valid'
    if not valid.any():
        return
    if topk:
        err = float((kc - k64)[valid].abs().max())
        print(f'{case}: max |nll - fp64| {err:.2e} (bound {O.NLL_ABS})')
        assert err <= O.NLL_ABS
    else:
        err = float(((kc - k64).abs() / k64)[valid].max())
        print(f'{case}: max rel err of p {err:.2e} (bound {O.P_REL})')
        assert err <= O.P_REL


def check_band(case, w, w64, band, valid):
    nb, nv = int(band.sum()), int(valid.sum())
    diff = (w.cpu() != w64) & ~band
    print(f'{case}: {nb} of {nv} valid pixels in the band, {int((w.cpu() != w64).sum())} differ from the fp64 oracle')
    assert nb <= O.BAND_SHARE * nv, 'the inputs must keep the band thin'
    assert not diff.any(), f'{int(diff.sum())} pixels outside the band differ from the fp64 oracle'


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('case', THRESH_CASES)
def test_threshold_mode(ops, shape, case):
    logits, label, thresh, min_kept = make_case(shape, case)
    w, info, keys = run(ops, logits, label, thresh, min_kept)
    k64, valid = O.keys(logits, label, 255, True, dtype=torch.float64)
    if case != 'saturated':
        assert float(logits.abs().max()) <= 32
        check_keys(f'{shape}/{case}', keys, k64, valid, False)
    else:
        kv = keys[keys >= 0]
        assert float(kv.min()) == 0.0 and float(kv.max()) == 1.0
    # the select, exactly: torch.sort of the same key map on the device
    vd = keys >= 0
    nv = int(vd.sum())
    assert nv == int(valid.sum()) == int(info[1])
    t32 = torch.tensor(thresh, dtype=torch.float32, device=DEV)
    if nv:
        k = min(min_kept * N, nv - 1)
        sk = keys[vd].sort()[0][k]
        want = torch.maximum(sk, t32)
        wins = 'thresh' if float(sk) <= float(t32) else 's[k]'
    else:
        k, want, wins = 0, t32, 'thresh'
    got = info_value(info)
    print(f'{shape}/{case}: n_valid {nv} k {k} threshold {float(got)!r} ({wins} wins) kept {int(info[2])}')
    assert int(info[3]) == k
    assert torch.equal(got.view(torch.int32), want.reshape(1).view(torch.int32)), (float(got), float(want))
    assert torch.equal(w, (vd & (keys < want)).float())
    assert int(info[2]) == int(w.sum())
    assert wins == {'thresh_wins': 'thresh', 'sk_wins': 's[k]', 'k_last': 's[k]'}.get(case, wins)
    if case == 'k_last':
        assert k == nv - 1
    if case in ('all_ignored',):
        assert nv == 0 and not w.any()
    if case == 'one_image_ignored':
        assert not w[1].any() and w[0].any()
    if case == 'bad_label':
        assert not valid[0, 20:24, 3:11].any() and not w[0, 20:24, 3:11].any()
    # the map against the fp64 oracle, outside the band
    if case != 'saturated':
        w64, thr64, _ = O.select_thresh(k64, valid, thresh, min_kept * N)
        check_band(f'{shape}/{case}', w, w64, O.band_thresh(k64, valid, thr64), valid)


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('case', TOPK_CASES)
def test_topk_mode(ops, shape, case):
    logits, label, _, min_kept = make_case(shape, case, topk=True)
    C = logits.shape[1]
    coef = [0.5 + 0.25 * (c % 5) for c in range(C)] if case == 'bad_label' else None
    w, info, keys = run(ops, logits, label, None, min_kept, coef)
    k64, valid = O.keys(logits, label, 255, False, coef, dtype=torch.float64)
    if coef is None:
        check_keys(f'{shape}/{case}', keys, k64, valid, True)
    else:                                            # the key is coef[y] * nll: the bound on nll scales with the coefficient
        err = float((keys.double().cpu() - k64)[valid].abs().max())
        print(f'{shape}/{case}: max |coef nll - fp64| {err:.2e} (bound {O.NLL_ABS * max(coef):.1e})')
        assert err <= O.NLL_ABS * max(coef)
    vd = keys >= 0
    nv = int(vd.sum())
    m = min(min_kept * N, nv)
    assert nv == int(valid.sum()) == int(info[1]) and int(info[3]) == m
    assert int(info[2]) == int(w.sum()) == m, 'exactly min(batch_kept, n_valid) pixels are kept'
    assert bool(((w == 0) | (w == 1)).all()) and not w[~vd].any()
    if m:
        cut = keys[vd].sort(descending=True)[0][m - 1]
        assert torch.equal(info_value(info).view(torch.int32), cut.reshape(1).view(torch.int32))
        assert bool((w[vd & (keys > cut)] == 1).all()) and not w[vd & (keys < cut)].any()
        ties = (vd & (keys == cut)).flatten().nonzero().flatten()
        take = m - int((vd & (keys > cut)).sum())
        kept = w.flatten()[ties]
        print(f'{shape}/{case}: n_valid {nv} kept {m} cut {float(cut)!r}, {ties.numel()} pixels equal to the cut, {take} of them kept')
        assert 1 <= take <= ties.numel()
        assert bool((kept[:take] == 1).all()) and not kept[take:].any(), 'ties are filled in raster order'
        if case == 'constant':
            assert ties.numel() == nv and take == m < nv
    else:
        assert not w.any()
    if case in ('random', 'bad_label'):
        w64, cut64, _ = O.select_topk(k64, valid, min_kept * N)
        check_band(f'{shape}/{case}', w, w64, O.band_topk(k64, valid, cut64, 1.0 if coef is None else max(coef)), valid)
    if case == 'constant':
        w64, _, _ = O.select_topk(k64, valid, min_kept * N)
        assert torch.equal(w.cpu(), w64), 'the first batch_kept valid pixels in raster order'


def test_the_cut_lands_inside_a_tie_on_clamped_borders(ops):
    """x8: the border pixels repeat their cell's logits, so p comes in runs of equal values; labels constant on the border make them ties"""
    C, lo, hi = SHAPES['x8']
    logits = torch.randn(N, C, *lo, generator=gen(5)) * 2
    logits[:, 0, 0, :] += 6                          # class 0 confident along the top row of cells
    label = torch.randint(0, C, (N, *hi), generator=gen(6))
    label[:, 0:4, :] = 3                             # a hard label there: large equal losses, four rows x 4-pixel runs
    label[:, 30:40, 30:40] = 255
    lab8 = label.to(torch.uint8)
    w, info, keys = run(ops, logits, lab8, None, 50)
    vd = keys >= 0
    m = 50 * N
    cut = keys[vd].sort(descending=True)[0][m - 1]
    ties = (vd & (keys == cut)).flatten().nonzero().flatten()
    take = m - int((keys > cut).sum())
    print(f'top-k: {ties.numel()} pixels equal to the cut {float(cut)!r}, {take} kept')
    assert ties.numel() > take >= 1, 'the inputs must put the cut inside a tie'
    kept = w.flatten()[ties]
    assert int(w.sum()) == m and bool((kept[:take] == 1).all()) and not kept[take:].any()
    # threshold mode: min_kept chosen from the key map (which does not depend on it) so that s[k] lies inside a run of equal p, above thresh
    thresh = 1e-6
    _, _, keys = run(ops, logits, lab8, thresh, 40)
    s = keys[keys >= 0].sort()[0]
    k = next(k for k in range(60, 400, 2) if float(s[k - 1]) == float(s[k]) == float(s[k + 1]) > thresh)
    w, info, keys2 = run(ops, logits, lab8, thresh, k // N)
    assert torch.equal(keys2, keys) and int(info[3]) == k
    print(f'threshold mode: k {k}, s[k] {float(s[k])!r} inside a run of {int((s == s[k]).sum())} equal p')
    assert torch.equal(info_value(info).view(torch.int32), s[k].reshape(1).view(torch.int32))
    assert torch.equal(w, ((keys >= 0) & (keys < s[k])).float()) and int(w.sum()) < k, 'strict: the whole run stays out'


def test_a_view_of_the_logits_is_refused_as_ce_upsample_fwd_refuses_it(ops):
    logits, label, thresh, min_kept = make_case('x4', 'thresh_wins')
    big = torch.randn(N, 8, 16, 16, device=DEV)
    view = big[:, 1:7]
    assert not view.is_contiguous()
    with pytest.raises(ValueError, match='contiguous'):
        ops.ce_upsample_fwd(view, label.to(DEV))
    with pytest.raises(ValueError, match='contiguous'):
        ops.ohem_sample(view, label.to(DEV), 255, thresh, min_kept * N)
    w, info = ops.ohem_sample(view.contiguous(), label.to(DEV), 255, thresh, min_kept * N)
    assert int(info[2]) == int(w.sum())


@pytest.mark.parametrize('det', [0, 1])
def test_two_calls_are_bit_identical(ops, det):
    ops.set_deterministic(det)
    try:
        for shape, case, topk in (('x4r', 'sk_wins', False), ('g19', 'thresh_wins', False), ('x8', 'random', True), ('x4r', 'constant', True)):
            logits, label, thresh, min_kept = make_case(shape, case, topk)
            a = run(ops, logits, label, thresh, min_kept)
            b = run(ops, logits, label, thresh, min_kept)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (shape, case)
    finally:
        ops.set_deterministic(0)


# ------------------------------------------------------------------------------------------------------------------ the head
def build_head(loss_decode, sampler, kind='DepthwiseSeparableASPPHead'):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head as build
    if kind == 'FCNHead':
        return build(dict(type='FCNHead', in_channels=32, in_index=2, channels=16, num_convs=1, concat_input=False, dropout_ratio=0.0,
                          num_classes=6, norm_cfg=dict(type='BN', requires_grad=True), align_corners=False, loss_decode=loss_decode,
                          sampler=sampler))
    return build(dict(type='DepthwiseSeparableASPPHead', in_channels=32, in_index=3, channels=16, dilations=(1, 12, 24, 36),
                      c1_in_channels=8, c1_channels=4, dropout_ratio=0.0, num_classes=6, norm_cfg=dict(type='BN', requires_grad=True),
                      align_corners=False, loss_decode=loss_decode, sampler=sampler))


def head_losses(head, logits, label, weight):
    from pfst_amd.engine import Tape, Var
    z, tape = Var(logits.to(DEV), True), Tape()
    res = head.losses(z, label.to(DEV).unsqueeze(1).contiguous(), None if weight is None else weight.to(DEV), tape)
    tape.backward()
    torch.cuda.synchronize()
    return res, z.grad


def link_ratio(got, ref):
    """tests/test_dice_loss_gpu.py: max |got - ref| / (1e-4 max|ref| + 1e-3 |ref|), within the per-link bound iff <= 1"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (1e-4 * ref.abs().max() + 1e-3 * ref.abs())).max())


CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
HEAD_CASES = {
    # name: (head type, shape, loss_decode, sampler)
    'decode_thresh': ('DepthwiseSeparableASPPHead', 'x4r', dict(type='CrossEntropyLoss', loss_weight=1.0), dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100)),
    'aux_topk': ('FCNHead', 'x8', [dict(type='CrossEntropyLoss', loss_weight=0.4, class_weight=CW6), dict(type='CrossEntropyLoss', loss_weight=0.2, loss_name='loss_ce2')],
                 dict(type='OHEMPixelSampler', min_kept=800)),
}


@pytest.mark.parametrize('name', list(HEAD_CASES))
def test_head_losses_with_a_sampler(name):
    kind, shape, loss_decode, sampler = HEAD_CASES[name]
    logits, label, _, _ = make_case(shape, 'thresh_wins')
    head = build_head(loss_decode, sampler, kind)
    terms = loss_decode if isinstance(loss_decode, list) else [loss_decode]
    # the fp64 oracle's map, on inputs whose band is empty
    thresh_mode = 'thresh' in sampler
    coef = None if thresh_mode else [sum(t['loss_weight'] * (t.get('class_weight') or [1.0] * 6)[c] for t in terms) for c in range(6)]
    k64, valid = O.keys(logits, label, 255, thresh_mode, coef, dtype=torch.float64)
    if thresh_mode:
        w64, cut64, _ = O.select_thresh(k64, valid, sampler['thresh'], sampler['min_kept'] * N)
        band = O.band_thresh(k64, valid, cut64)
    else:
        w64, cut64, _ = O.select_topk(k64, valid, sampler['min_kept'] * N)
        band = O.band_topk(k64, valid, cut64, max(coef))
    # (in top-k mode the pixel AT the cut is the band's one member: nothing else can change places with it)
    assert int(band.sum()) == (0 if thresh_mode else 1), 'the head case needs inputs with an empty band'
    assert 0 < int(w64.sum()) < int(valid.sum())
    passed = torch.rand(label.shape, generator=gen(3))
    res, grad = head_losses(head, logits, label, passed)
    assert torch.equal(head.sampler.last_info.cpu()[1:3], torch.tensor([int(valid.sum()), int(w64.sum())]))
    want_loss, want_grad = {}, 0
    for t in terms:
        l, gr = O.ce_under_weights(logits, label, w64, 255, t.get('class_weight'), t['loss_weight'])
        want_loss[t.get('loss_name', 'loss_ce')] = l
        want_grad = want_grad + gr
    assert list(res) == list(want_loss) + ['acc_seg', '_bad_labels']
    for k, want in want_loss.items():
        got = float(res[k])
        print(f'{name} {k}: {got!r} fp64 {want!r} rel err {abs(got - want) / abs(want):.2e} (bound 1e-5)')
        assert abs(got - want) <= 1e-5 * abs(want)
    ratio = link_ratio(grad, want_grad)
    print(f'{name} d logits: worst ratio to the per-link bound {ratio:.2e}')
    assert ratio <= 1.0
    # a seg_weight passed in is ignored; acc_seg is the head's value without a sampler
    res2, grad2 = head_losses(head, logits, label, None)
    assert all(torch.equal(res[k], res2[k]) for k in res) and torch.equal(grad, grad2)
    plain, _ = head_losses(build_head(loss_decode, None, kind), logits, label, None)
    assert torch.equal(plain['acc_seg'], res['acc_seg']) and 0.0 < float(res['acc_seg']) < 100.0
    assert not any(torch.equal(plain[k], res[k]) for k in want_loss)


def test_supervised_train_step_with_samplers_on_both_heads():
    import math
    import pfst_amd  # noqa: F401
    from helpers import model_cfg, to_dev
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import synth_batch
    cfg = model_cfg(dropout=0.1)
    cfg['decode_head']['sampler'] = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=500)
    cfg['auxiliary_head']['sampler'] = dict(type='OHEMPixelSampler', min_kept=500)
    torch.manual_seed(0)
    model = build_segmentor(cfg)
    model.cuda()
    opt = build_optimizer(model, dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005))
    batch = {k: v for k, v in synth_batch(2, 64, 6, seed=7).items() if not k.startswith('target_')}
    assert tuple(batch['img'].shape) == (2, 3, 64, 64)
    out = model.train_step(to_dev(batch, DEV), opt)
    torch.cuda.synchronize()
    lv = out['log_vars']
    print(lv)
    assert list(lv) == ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss']
    assert all(math.isfinite(v) for v in lv.values()) and lv['decode.loss_ce'] > 0 and lv['aux.loss_ce'] > 0
    for head in (model.decode_head, model.auxiliary_head):
        nv, kept = (int(v) for v in head.sampler.last_info[1:3])
        assert 0 < kept <= nv <= 2 * 64 * 64
    assert int(model.auxiliary_head.sampler.last_info[2]) == min(1000, int(model.auxiliary_head.sampler.last_info[1]))


# ------------------------------------------------------------------------------------------------------------------ the executed reference
GOLDEN_HEADS = {
    # name: (head type, logits and labels of, loss_decode, sampler)            -- tests/golden/make_golden_ohem.py's HEADS
    'head_thresh': ('DepthwiseSeparableASPPHead', 'x4r_thresh', dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                    dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100)),
    'head_topk': ('FCNHead', 'x8_topk', [dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.4, class_weight=CW6),
                                         dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.2, loss_name='loss_ce2')],
                  dict(type='OHEMPixelSampler', min_kept=800)),
}


@pytest.mark.parametrize('name', list(GOLDEN_HEADS))
def test_head_matches_the_executed_reference(golden_dir, name):
    """the reference's own BaseDecodeHead.losses with its OHEMPixelSampler (fp32, CPU) on inputs whose band around the cut holds no pixel that
    could fall either way (asserted by the generator): the same map bit for bit, losses within 1e-5, gradients within the per-link bound"""
    import os
    golden = np.load(os.path.join(golden_dir, 'ohem_sampler.npz'))
    kind, src, loss_decode, sampler = GOLDEN_HEADS[name]
    logits, label = torch.from_numpy(golden[src + '|logits']), torch.from_numpy(golden[src + '|label'])
    want_w = torch.from_numpy(np.unpackbits(golden[name + '|weight_bits'])[:label.numel()].astype(np.float32)).view(label.shape)
    head = build_head(loss_decode, sampler, kind)
    res, grad = head_losses(head, logits, label, torch.rand(label.shape, generator=gen(4)))
    w = head.sampler.sample(logits.to(DEV), label.to(DEV))
    assert torch.equal(w.cpu(), want_w), f'{int((w.cpu() != want_w).sum())} pixels differ from the reference map'
    assert list(res) == list(golden[name + '|names']) + ['_bad_labels']
    for k, want in zip(golden[name + '|names'], golden[name + '|values']):
        got = float(res[k])
        print(f'{name} {k}: {got!r} reference {float(want)!r} rel err {abs(got - want) / abs(want):.2e}')
        assert abs(got - want) <= 1e-5 * abs(want)
    ratio = link_ratio(grad, torch.from_numpy(golden[name + '|grad']))
    print(f'{name} d logits: worst ratio to the per-link bound {ratio:.2e}')
    assert ratio <= 1.0
