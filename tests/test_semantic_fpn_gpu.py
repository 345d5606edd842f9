"""The FPN neck under FPNHead on the GPU against what the reference's own modules returned (tests/golden/semantic_fpn.npz, made by
tests/golden/make_golden_semantic_fpn.py), under each of the three convolution arithmetics and on the golden's three geometries: A (every
level in the fused sum, every merge exact x2), C (levels 1 and 2 fused, level 3 through the addend, non-integer nearest merges) and B (nothing
fused).  Neck outputs, logits, level-sum features, input gradients and parameter gradients are held to the project's per-link bound
|hip - ref| <= 1e-4 max|ref| + 1e-3 |ref|, the losses to 1e-4 max(|v|, 1e-3) (both: tests/test_baseline_heads_gpu.py).  Further: the deferred
normalisations are bit-identical to the written tensors; the head's launches are counted (one level sum, the resizes of the levels outside
it, one adjoint resize for the sum, no pfst_absmax under f16x3); the evaluation-mode head equals the same modules through bn_apply and the
existing ops."""
import os

import numpy as np
import pytest
import torch

from test_upernet_gpu import link_ratio, load_golden_params, prepare

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NORM = dict(type='BN', requires_grad=True)
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
NECK = dict(type='FPN', in_channels=[8, 16, 24, 32], out_channels=16, num_outs=4)
HEAD = dict(type='FPNHead', in_channels=[16] * 4, in_index=[0, 1, 2, 3], feature_strides=[4, 8, 16, 32], channels=8, dropout_ratio=0.0,
            num_classes=6, norm_cfg=NORM, align_corners=False, loss_decode=CE)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'semantic_fpn.npz'))


@pytest.fixture(params=['f32', 'bf16x6', 'f16x3'])
def conv_math(request):
    from pfst_amd import layers
    prev, layers.CONV_MATH = layers.CONV_MATH, request.param
    yield request.param
    layers.CONV_MATH = prev


def build(golden):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_head, build_neck
    return load_golden_params(build_neck(dict(NECK)), golden, 'neck'), load_golden_params(build_head(dict(HEAD)), golden, 'head')


def run(neck, head, golden, geo, count=None, bwd_count=None):
    """neck, head, losses, backward on geometry `geo`.  count / bwd_count: lists that receive the name of every library call made during the HEAD's
    forward pass / during the backward sweep up to and including the level sum's closure"""
    from pfst_amd import _lib, hip_ops, layers
    from pfst_amd.engine import Tape, Var
    prepare(neck), prepare(head)
    xs = [Var(torch.from_numpy(golden[f'{geo}|x{i}'].astype(np.float32)).to(DEV), True) for i in range(4)]
    label = torch.from_numpy(golden[f'{geo}|label']).to(DEV)
    tape = Tape()
    outs = neck(xs, tape)
    if layers.CONV_MATH == 'f16x3':
        for o in outs:                       # the maxima of the head's inputs are the producer's side of the hand-over (as tests/test_upernet_gpu.py)
            layers.amax_of(o)
    real = _lib.call

    def counting(into):
        def call(name, *args):
            into.append(name)
            return real(name, *args)
        return call
    if count is not None:
        _lib.call = hip_ops.call = counting(count)
    try:
        logits, feats = head.forward(outs, return_features=True, tape=tape, training=True)
    finally:
        _lib.call = hip_ops.call = real
    res = head.losses(logits, label, None, tape)
    if bwd_count is not None:
        # run the sweep down to the level sum's closure under the counter, the rest plainly
        _lib.call = hip_ops.call = counting(bwd_count)
        try:
            while tape.fns:
                fn, tag = tape.fns.pop()
                fn()
                if tag is not None and tag.get('op') == 'fpn_level_sum':
                    break
        finally:
            _lib.call = hip_ops.call = real
    tape.backward()
    torch.cuda.synchronize()
    return dict(outs=outs, logits=logits, feats=feats, res=res, dxs=[x.grad for x in xs])


def named_grads(neck, head):
    return {**{'neck.' + k: p.grad for k, p in neck.named_parameters()}, **{'head.' + k: p.grad for k, p in head.named_parameters()}}


@pytest.mark.parametrize('geo', ['A', 'B', 'C'])
def test_neck_and_head_match_the_reference(golden, conv_math, geo):
    neck, head = build(golden)
    r = run(neck, head, golden, geo)
    ref = lambda k: torch.from_numpy(golden[f'{geo}|{k}'])
    worst = {f'out{i}': link_ratio(o.data, ref(f'out{i}')) for i, o in enumerate(r['outs'])}
    worst['logits'] = link_ratio(r['logits'].data, ref('logits'))
    worst['feats'] = link_ratio(r['feats'].data, ref('feats'))
    for i, dx in enumerate(r['dxs']):
        worst[f'dx{i}'] = link_ratio(dx, ref(f'dx{i}'))
    checked = 0
    for k, gr in named_grads(neck, head).items():
        if f'{geo}|grad|{k}' in golden.files:
            worst['grad ' + k] = link_ratio(gr, ref('grad|' + k))
            checked += 1
    assert checked == 16 + 2 + 3 * 7 or (geo == 'B' and checked == 0), checked          # neck: 8 convs with a bias; head: conv_seg + 7 ConvModules
    for k, v in worst.items():
        print(f'semantic fpn {geo} {conv_math} {k}: {v:.3f} of the per-link bound')
    for k, want in zip(golden[f'{geo}|loss_names'], golden[f'{geo}|loss_values']):
        got = float(r['res'][str(k)])
        print(f'semantic fpn {geo} {conv_math} {k}: {got!r} reference {float(want)!r}')
        assert abs(got - want) <= 1e-4 * max(abs(want), 1e-3), (k, got, want)
    assert float(r['res']['_bad_labels']) == 0.0
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_the_deferred_normalisation_is_bit_identical_to_the_written_tensors(golden, conv_math):
    from pfst_amd import layers
    neck, head = build(golden)
    on = run(neck, head, golden, 'A')
    on_grads = {k: v.clone() for k, v in named_grads(neck, head).items()}
    prev, layers.DEFER_BN_APPLY = layers.DEFER_BN_APPLY, False
    try:
        neck, head = build(golden)
        off = run(neck, head, golden, 'A')
    finally:
        layers.DEFER_BN_APPLY = prev
    assert torch.equal(on['logits'].data, off['logits'].data) and torch.equal(on['feats'].data, off['feats'].data)
    for a, b in zip(on['dxs'], off['dxs']):
        assert torch.equal(a, b)
    for k, v in named_grads(neck, head).items():
        assert torch.equal(on_grads[k], v), k


def test_the_heads_launches_are_counted(golden):
    from pfst_amd import layers
    prev = layers.CONV_MATH
    try:
        for math in ('f32', 'f16x3'):
            layers.CONV_MATH = math
            fwd, bwd = [], []
            neck, head = build(golden)
            r = run(neck, head, golden, 'A', count=fwd, bwd_count=bwd)
            assert fwd.count('pfst_fpn_level_sum') == 1 and fwd.count('pfst_resize_bilinear') == 0, fwd
            assert fwd.count('pfst_upsample2x_norm') == 0 + 1 + 2 and fwd.count('pfst_bn_apply') == 0, fwd       # every normalisation rides in a consumer
            assert bwd.count('pfst_resize_bilinear_bwd') == 1, bwd                                                # one adjoint resize serves levels 1 .. 3
            if math == 'f16x3':
                assert fwd.count('pfst_absmax') == 0, fwd
                assert r['feats'].amax is not None and float(r['feats'].amax.max()) == float(r['feats'].data.abs().max())
            fwd = []
            neck, head = build(golden)
            run(neck, head, golden, 'C', count=fwd)
            assert fwd.count('pfst_fpn_level_sum') == 1 and fwd.count('pfst_resize_bilinear') == 2, fwd            # level 3: x2, then down to level 0's grid
            if math == 'f16x3':
                assert fwd.count('pfst_absmax') == 0, fwd
            fwd = []
            neck, head = build(golden)
            run(neck, head, golden, 'B', count=fwd)
            assert fwd.count('pfst_fpn_level_sum') == 1 and fwd.count('pfst_resize_bilinear') == 6 and fwd.count('pfst_axpy_f32') == 2, fwd
    finally:
        layers.CONV_MATH = prev


def test_every_merged_map_gets_its_maximum_from_the_merge(golden):
    from pfst_amd import _lib, hip_ops, layers
    from pfst_amd.engine import Var
    prev, layers.CONV_MATH = layers.CONV_MATH, 'f16x3'
    try:
        neck, _ = build(golden)
        prepare(neck)
        for geo in ('A', 'B'):
            xs = [Var(torch.from_numpy(golden[f'{geo}|x{i}'].astype(np.float32)).to(DEV), False) for i in range(4)]
            seen = []
            real = hip_ops.topdown_merge_nearest

            def merge(lat, coarse, out=None, amax=None):
                y = real(lat, coarse, out=out, amax=amax)
                seen.append((y, amax))
                return y
            hip_ops.topdown_merge_nearest = merge
            try:
                neck(xs, None)
            finally:
                hip_ops.topdown_merge_nearest = real
            assert len(seen) == 3
            for y, amax in seen:
                assert amax is not None and float(amax.max()) == float(y.abs().max())
    finally:
        layers.CONV_MATH = prev


def test_evaluation_mode_head_equals_bn_apply_and_the_existing_ops(golden, conv_math):
    """under bn_eval nothing is deferred: the head's kernels read written tensors (null tables).  The same modules through conv_bn_act, resize_bilinear
    and adds, in the kernel's order"""
    from pfst_amd import hip_ops, layers
    from pfst_amd.engine import Var
    from pfst_amd.layers import ConvModule, bn_eval
    neck, head = build(golden)
    prepare(neck), prepare(head)
    with torch.no_grad():
        for m in head.modules():          # running statistics that are not the identity
            if hasattr(m, 'running_mean'):
                m.running_mean.copy_(torch.linspace(-0.2, 0.3, m.running_mean.numel(), device=DEV))
                m.running_var.copy_(torch.linspace(0.5, 1.5, m.running_var.numel(), device=DEV))
    for geo in ('A', 'C'):
        xs = [Var(torch.from_numpy(golden[f'{geo}|x{i}'].astype(np.float32)).to(DEV), False) for i in range(4)]
        with bn_eval():
            outs = neck(xs, None)
            logits, feats = head.forward(outs, return_features=True, tape=None, training=False)
            finals = []
            for i, o in enumerate(outs):
                convs = [m for m in head.scale_heads[i] if isinstance(m, ConvModule)]
                t = o
                for k, cm in enumerate(convs):
                    t = cm(t, None)
                    if i > 0 and k < len(convs) - 1:
                        t = Var(hip_ops.resize_bilinear(t.data, (2 * t.data.shape[2], 2 * t.data.shape[3])))
                finals.append(t.data)
        h0 = tuple(finals[0].shape[-2:])
        half = [f for f in finals[1:] if (2 * f.shape[2], 2 * f.shape[3]) == h0]
        rest = [f for f in finals[1:] if (2 * f.shape[2], 2 * f.shape[3]) != h0]
        want = finals[0]
        if half:
            s = half[0]
            for f in half[1:]:
                s = s + f
            want = want + hip_ops.resize_bilinear(s, h0)
        if rest:
            add = None
            for f in rest:
                f = hip_ops.resize_bilinear(hip_ops.resize_bilinear(f, (2 * f.shape[2], 2 * f.shape[3])), h0)
                add = f if add is None else add + f
            want = want + add
        assert len(half) == (3 if geo == 'A' else 2)
        assert torch.equal(feats.data, want), geo
        assert bool(torch.isfinite(logits.data).all())
