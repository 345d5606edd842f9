"""HRNet under a multi-level FCNHead against the reference's own run (tests/golden/hrnet.npz, make_golden_hrnet.py), under each arithmetic of
the dense convolutions, on geometry A (3 x 64 x 64: every exchange is an exact power of two, the fused route) and B (3 x 72 x 56: the
reference interpolates twice, the composed route).  Bounds: the project's per-link bound |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref| on every
stored tensor and 1e-4 max(|v|, 1e-3) on the loss, both as in tests/test_baseline_heads_gpu.py.  Large tensors are stored as strided samples
(tests/hrnet_oracle.py `sample`); the same sample of the project's tensor is compared.

Launch counts, through the counting wrapper of _lib.call: the narrow model has 2 + 3 + 2 x 4 = 13 exchange outputs and 2 + 6 + 2 x 12 = 32
fuse paths.  On A every output is fused.  On B the rule is applied per output (a coarser member's grid times 2^(j-i) must be the output grid):
the 8 outputs with a member that fails it -- stage3 i = 0, 1 and stage4 i = 0, 1, 2 of both modules, 22 fuse paths -- take the composed
route with 27 resize_bilinear launches (two where the reference interpolates twice); the 5 others -- stage2's 18 x 14 over 9 x 7 and its last
branch, the last branch of stage3 and of both stage4 modules, which have no coarser member -- are exact and stay fused."""
import os

import numpy as np
import pytest
import torch

from hrnet_oracle import KEEP_GRAD, KEEP_MAP, sample
from test_hrnet_cpu import HEAD, NARROW, NORM
from test_upernet_gpu import conv_math, link_ratio, load_golden_params, prepare  # noqa: F401  (conv_math: a fixture)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
OUTPUTS, PATHS = 13, 32
B_FUSED, B_COMPOSED, B_COMPOSED_PATHS, B_RESIZES = 5, 8, 22, 27
GRIDS = dict(A=[(16, 16), (8, 8), (4, 4), (2, 2)], B=[(18, 14), (9, 7), (5, 4), (3, 2)])


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'hrnet.npz'))


def build(golden):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import build_backbone, build_head
    net = load_golden_params(build_backbone(dict(type='HRNet', extra=NARROW, norm_cfg=NORM)), golden, 'backbone')
    head = load_golden_params(build_head(dict(HEAD)), golden, 'head')
    prepare(net), prepare(head)
    return net, head


def run(golden, geo, count=None):
    """forward, loss, backward.  count: a dict that receives the names of the library calls, by phase ('backbone', 'head', 'backward')"""
    from pfst_amd import _lib, hip_ops
    from pfst_amd.engine import Tape, Var
    net, head = build(golden)
    img = Var(torch.from_numpy(golden[geo + '|img'].astype(np.float32)).to(DEV), True)
    label = torch.from_numpy(golden[geo + '|label']).to(DEV)
    tape = Tape()
    real = _lib.call
    phase = ['backbone']
    if count is not None:
        def counting(name, *args):
            count.setdefault(phase[0], []).append(name)
            return real(name, *args)
        _lib.call = hip_ops.call = counting
    try:
        outs = net(img, tape)
        phase[0] = 'head'
        logits, feats = head.forward(list(outs), return_features=True, tape=tape, training=True)
        res = head.losses(logits, label, None, tape)
        phase[0] = 'backward'
        tape.backward()
    finally:
        _lib.call = hip_ops.call = real
    torch.cuda.synchronize()
    return net, head, outs, logits, feats, res, img.grad


@pytest.mark.parametrize('geo', ['A', 'B'])
def test_matches_the_reference(golden, conv_math, geo):  # noqa: F811
    calls = {}
    net, head, outs, logits, feats, res, dimg = run(golden, geo, calls)
    assert [tuple(o.data.shape[2:]) for o in outs] == GRIDS[geo]
    ref = lambda k: torch.from_numpy(golden[f'{geo}|{k}'])
    worst = {f'out{i}': link_ratio(o.data, ref(f'out{i}')) for i, o in enumerate(outs)}
    worst['logits'] = link_ratio(logits.data, ref('logits'))
    worst['feats'] = link_ratio(sample(feats.data, KEEP_MAP), ref('feats'))
    worst['dimg'] = link_ratio(sample(dimg, KEEP_MAP), ref('dimg'))
    for part, m in (('backbone', net), ('head', head)):
        for k, p in m.named_parameters():
            worst[f'grad {part}.{k}'] = link_ratio(sample(p.grad, KEEP_GRAD), ref(f'grad|{part}.{k}'))
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:6]
    print(f'hrnet {geo} {conv_math}: the largest shares of the per-link bound:', [(k, round(v, 3)) for k, v in top])
    for k, want in zip(golden[geo + '|loss_names'], golden[geo + '|loss_values']):
        if not str(k).startswith('loss'):
            continue
        got = float(res[str(k)])
        print(f'hrnet {geo} {conv_math} {k}: {got!r} reference {float(want)!r}')
        assert abs(got - want) <= 1e-4 * max(abs(want), 1e-3), (k, got, want)
    assert float(res['_bad_labels']) == 0.0
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad
    # the route: one fused launch per exchange output on A; on B none for an output with a member off the exact grid
    fwd, bwd = calls['backbone'], calls['backward']
    assert fwd.count('pfst_hr_fuse') == (OUTPUTS if geo == 'A' else B_FUSED), fwd.count('pfst_hr_fuse')
    assert fwd.count('pfst_resize_bilinear') == (0 if geo == 'A' else B_RESIZES), fwd.count('pfst_resize_bilinear')
    assert bwd.count('pfst_hr_fuse_bwd') == OUTPUTS


def test_launch_counts_on_the_fused_route(golden):
    from pfst_amd import layers
    prev, layers.CONV_MATH = layers.CONV_MATH, 'f16x3'
    try:
        a, b = {}, {}
        run(golden, 'A', a)
        run(golden, 'B', b)
    finally:
        layers.CONV_MATH = prev
    # per exchange output: one forward launch; in backward one call (the gate pass and the multi-level gather), and nothing else -- dL/dx_i
    # takes the gated buffer itself, so the only plane copies of the whole step are the head's level 0 and its adjoint
    assert a['backbone'].count('pfst_hr_fuse') == OUTPUTS and a['backward'].count('pfst_hr_fuse_bwd') == OUTPUTS
    assert a['backbone'].count('pfst_copy_planes') == 0 and a['head'].count('pfst_copy_planes') == 1 and a['backward'].count('pfst_copy_planes') == 1
    assert a['backbone'].count('pfst_resize_bilinear') == 0 and a['backward'].count('pfst_resize_bilinear_bwd') == 0
    assert a['head'].count('pfst_fpn_resize_concat') == 3 and a['backward'].count('pfst_fpn_resize_concat_bwd') == 3
    # no maximum is taken by a pass of its own inside the backbone
    assert a['backbone'].count('pfst_absmax') == 0 and a['head'].count('pfst_absmax') == 0
    # no normalisation pass for a fuse layer: every conv -> BN layer of the backbone but the 32 fuse paths' last ones (and layer1.0's
    # downsample, which its block's bn3 pass normalises on load) runs exactly one; the composed route one per fuse path and output more
    from pfst_amd.layers import BatchNorm2dP, folds_into_residual
    net, _ = build(golden)
    norms = sum(isinstance(m, BatchNorm2dP) for m in net.modules())
    assert a['backbone'].count('pfst_bn_apply') == norms - PATHS - int(bool(folds_into_residual())), (a['backbone'].count('pfst_bn_apply'), norms)
    assert b['backbone'].count('pfst_bn_apply') - a['backbone'].count('pfst_bn_apply') == B_COMPOSED_PATHS + B_COMPOSED
    assert b['backbone'].count('pfst_hr_fuse') == B_FUSED and b['backward'].count('pfst_hr_fuse_bwd') == OUTPUTS


def test_evaluation_mode_equals_the_composition(golden, monkeypatch):
    """running statistics: every fuse layer is written by bn_apply; the fused launch over those final values gives the bits of the composed route"""
    from pfst_amd import hip_ops
    from pfst_amd.engine import Var
    from pfst_amd.layers import bn_eval
    net, _ = build(golden)
    img = torch.from_numpy(golden['A|img'].astype(np.float32)).to(DEV)
    calls = []
    real = hip_ops.call
    monkeypatch.setattr(hip_ops, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    with bn_eval():
        fused = [o.data.clone() for o in net(Var(img, False), None)]
        assert calls.count('pfst_hr_fuse') == OUTPUTS
        from pfst_amd import models
        monkeypatch.setattr(models.HRModule, '_exchange', models.HRModule._exchange_composed)       # every output through the existing ops
        del calls[:]
        composed = [o.data.clone() for o in net(Var(img, False), None)]
        assert calls.count('pfst_hr_fuse') == 0 and calls.count('pfst_resize_bilinear') > 0
    for i, (f, c) in enumerate(zip(fused, composed)):
        assert bool(torch.isfinite(f).all()) and torch.equal(f, c), f'level {i}'


def test_shared_gated_buffer_equals_the_copying_wiring(golden):
    """models.HR_SHARE_GATED: the exchange's backward gates dL/dout in place and hands that buffer to x_i as its gradient buffer; switched off
    it writes a buffer of its own and adds it with one more pass per output.  Same gradients, bit for bit (deterministic mode)"""
    from pfst_amd import hip_ops, layers, models
    was, prev = hip_ops.is_deterministic(), layers.CONV_MATH
    hip_ops.set_deterministic(True)
    layers.CONV_MATH = 'f32'
    try:
        got = {}
        for share in (True, False):
            models.HR_SHARE_GATED = share
            calls = {}
            net, head, outs, logits, feats, res, dimg = run(golden, 'A', calls)
            got[share] = [dimg.clone()] + [p.grad.clone() for p in net.parameters()]
            assert calls['backward'].count('pfst_copy_planes') == (1 if share else 1 + OUTPUTS)
    finally:
        models.HR_SHARE_GATED = True
        layers.CONV_MATH = prev
        hip_ops.set_deterministic(was)
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False]))
