"""Which kernel family every convolution of the DeepLabV3+ segmentor takes -- forward, data gradient, weight gradient -- under each of the
three arithmetics, asserted on the CPU: Conv2dP.plan / set_plan decide without allocating or launching, Conv2dP.wgrad_route names the
weight-gradient kernel for an input size.  The expectations are a table written by hand, by layer class, from DESIGN.md section 4 and
checked against the launch trace of a b = 8 x 1024^2 train step (profiles/conv_dispatch_refactor.txt); no GPU, only the built library
(the Winograd layers' route asks it for pfst_wino_tiles, as tests/test_abi.py asks it for the ABI version)."""
import re

import pytest

from helpers import SIZES, model_cfg

# families: 'fp32' the fp32-input MFMA kernel, 'bf16x6' / 'f16x3' the split kernels, 'wino_*' through the Winograd domain with that GEMM.
# weight-gradient routes: Conv2dP.wgrad_route's answers.
# class -> {arithmetic: (forward, data gradient, weight gradient)}; first matching row wins
WINO = dict(f16x3=('wino_f16x3', 'wino_f16x3', 'wino_f16x3'), bf16x6=('wino_bf16x6', 'wino_bf16x6', 'wino_bf16x6'),
            f32=('wino_f32', 'wino_f32', 'wino_f32'))
# 1x1, stride 1, more than 64 output channels, contraction over whole 16-channel blocks: the 128- / 256-row f16x3 tiles, whole-line weight gradient
WIDE_1X1 = dict(f16x3=('f16x3', 'f16x3', 'line_f16x3'), bf16x6=('bf16x6', 'bf16x6', 'quad_bf16x6'), f32=('fp32', 'fp32', 'generic'))
# 1x1, stride 1, 33 ... 64 output channels: the 64-row f16x3 tile; the weight gradient is HBM-bound and stays on the K-quad bf16x6 kernel
NARROW_1X1 = dict(f16x3=('f16x3', 'f16x3', 'quad_bf16x6'), bf16x6=('bf16x6', 'bf16x6', 'quad_bf16x6'), f32=('fp32', 'fp32', 'generic'))
# stride 2 (3x3 or 1x1): the weight gradient on the generic kernel in every arithmetic
STRIDE2 = dict(f16x3=('f16x3', 'f16x3', 'generic'), bf16x6=('bf16x6', 'bf16x6', 'generic'), f32=('fp32', 'fp32', 'generic'))
# classifiers (512 / 256 -> 6 classes, bias): 6 output rows forward -> bf16x6; the data gradient contracts over 6 channels -> fp32 MFMA
CLASSIFIER = dict(f16x3=('bf16x6', 'fp32', 'quad_bf16x6'), bf16x6=('bf16x6', 'fp32', 'quad_bf16x6'), f32=('fp32', 'fp32', 'generic'))
TABLE = [
    # 3 -> 32, stride 2: the forward contraction is not a multiple of 16 channels -> fp32 MFMA in every mode
    (r'backbone\.stem\.0$', dict(f16x3=('fp32', 'bf16x6', 'generic'), bf16x6=('fp32', 'bf16x6', 'generic'), f32=('fp32', 'fp32', 'generic'))),
    # 32 -> 32: <= 32 output rows both ways -> bf16x6; direct stride-1 3x3 weight gradient -> K-quad f16x3
    (r'backbone\.stem\.3$', dict(f16x3=('bf16x6', 'bf16x6', 'quad_f16x3'), bf16x6=('bf16x6', 'bf16x6', 'generic'), f32=('fp32', 'fp32', 'generic'))),
    # 32 -> 64: 64 rows forward (64-row f16x3 tile), 32 rows in the data gradient (bf16x6)
    (r'backbone\.stem\.6$', dict(f16x3=('f16x3', 'bf16x6', 'quad_f16x3'), bf16x6=('bf16x6', 'bf16x6', 'generic'), f32=('fp32', 'fp32', 'generic'))),
    (r'backbone\.layer1\.\d\.conv1$', NARROW_1X1),
    # 64 x 64 stays outside the Winograd dispatch (transform-bound)
    (r'backbone\.layer1\.\d\.conv2$', dict(f16x3=('f16x3', 'f16x3', 'quad_f16x3'), bf16x6=('bf16x6', 'bf16x6', 'generic'), f32=('fp32', 'fp32', 'generic'))),
    (r'backbone\.layer2\.0\.(conv2|downsample\.0)$', STRIDE2),
    (r'backbone\.layer[234]\.\d\.conv2$', WINO),                                    # 3x3 stride 1 from 128 x 128 channels
    (r'backbone\.layer\d\.\d\.(conv1|conv3|downsample\.0)$', WIDE_1X1),
    # the image-pool branch sees N x 2048 x 1 x 1: no float4 of a plane for the whole-line / K-quad weight gradients
    (r'decode_head\.image_pool\.1\.conv$', dict(f16x3=('f16x3', 'f16x3', 'generic'), bf16x6=('bf16x6', 'bf16x6', 'generic'), f32=('fp32', 'fp32', 'generic'))),
    (r'decode_head\.(aspp_modules\.0|aspp_modules\.\d\.pointwise_conv|sep_bottleneck\.\d\.pointwise_conv)\.conv$', WIDE_1X1),
    (r'decode_head\.bottleneck\.conv$', WINO),
    (r'decode_head\.c1_bottleneck\.conv$', NARROW_1X1),                             # 256 -> 48
    (r'auxiliary_head\.convs\.0\.conv$', WINO),
    (r'(decode_head|auxiliary_head)\.conv_seg$', CLASSIFIER),
]


def _lookup(rows, name):
    for pat, val in rows:
        if re.match(pat, name):
            return val
    raise AssertionError(f'no row of the table covers {name}')


@pytest.fixture(scope='module')
def convs():
    import pfst_amd  # noqa: F401
    from pfst_amd import layers
    from pfst_amd.registry import SEGMENTORS
    model = SEGMENTORS.build(model_cfg())
    return [(n, m) for n, m in model.named_modules() if isinstance(m, layers.Conv2dP)]


def test_the_segmentor_has_the_layers_the_table_was_written_for(convs):
    from pfst_amd import layers
    assert (layers.WINOGRAD, layers.WINO_MIN_CC, layers.WINO_MIN_CC_WGRAD, layers.ops.WINO_TILE) == (True, 128 * 128, 128 * 128, 4)
    dense = [(n, c) for n, c in convs if not c.depthwise]
    assert (len(convs), len(dense), len(convs) - len(dense)) == (72, 67, 5)
    # 14 layers through the Winograd domain: 13 forward + 14 ... launches of pfst_wino_gemm_f16x3 in tests/test_fullsize_gpu.py
    assert sum(c._wino_eligible() for _, c in dense) == 14
    assert sum(_lookup(TABLE, n) is WINO for n, _ in dense) == 14
    for n, _ in dense:
        _lookup(SIZES, n)


@pytest.mark.parametrize('need_dgrad', [True, False])
@pytest.mark.parametrize('math', ['f16x3', 'bf16x6', 'f32'])
def test_every_layer_takes_the_kernels_of_its_class(convs, math, need_dgrad):
    from pfst_amd import layers
    prev = layers.CONV_MATH
    layers.CONV_MATH = math
    try:
        checked = 0
        for name, conv in convs:
            plan = conv.plan(need_dgrad)
            if conv.depthwise:
                assert plan == layers.ConvPlan(), name          # the depthwise kernels are not part of this dispatch
                continue
            fwd, dgrad, wgrad = _lookup(TABLE, name)[math]
            if not need_dgrad:
                dgrad = None
            want = layers.ConvPlan(wino=fwd.startswith('wino'), wino_f16=fwd == 'wino_f16x3', f16_f=fwd == 'f16x3', f16_d=dgrad == 'f16x3',
                                   split_f=fwd == 'bf16x6', split_d=dgrad == 'bf16x6', fp32_f=fwd == 'fp32', fp32_d=dgrad == 'fp32')
            assert plan == want, (name, math, need_dgrad, plan, want)
            # exactly one family per direction that runs
            assert plan.wino + plan.f16_f + plan.split_f + plan.fp32_f == 1, (name, plan)
            assert plan.wino + plan.f16_d + plan.split_d + plan.fp32_d == (1 if need_dgrad or plan.wino else 0), (name, plan)
            assert conv.set_plan(need_dgrad) == plan
            assert (conv.wino, conv.wino_f16, conv.f16_f, conv.f16_d, conv.split_f, conv.split_d) == tuple(plan[:6])
            assert conv.fprop_reads_amax == (fwd in ('f16x3', 'wino_f16x3')), name
            size = _lookup(SIZES, name)
            assert conv.wgrad_route(size, size) == wgrad, (name, math, size, conv.wgrad_route(size, size), wgrad)
            assert (wgrad in layers.WGRAD_READS_AMAX) == wgrad.endswith('f16x3')
            checked += 1
        assert checked == 67
    finally:
        layers.CONV_MATH = prev
        for _, conv in convs:
            conv.set_plan(True)
