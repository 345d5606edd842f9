"""The decision EncoderDecoder.repack_weights replays on, without a GPU: repack_signature -- the switches of layers.repack_key, the version
of the module tree and the address of EVERY convolution's weight and bias.  Equal signatures mean "replay the recorded packing launches",
unequal ones "walk the layers again".  On a CPU-built DeepLabV3+ segmentor: rebinding `.data` of any single weight or bias, replacing any
Conv2dP and flipping any switch change it; in-place updates and zero_grad do not.  The same bookkeeping under a ParamArena: a rebound
`.data` is re-adopted, a replaced Parameter object raises before anything else happens."""
import pytest
import torch

from helpers import model_cfg


@pytest.fixture(scope='module')
def seg():
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import SEGMENTORS
    return SEGMENTORS.build(model_cfg())


def named_convs(model):
    from pfst_amd import layers
    return [(n, m) for n, m in model.named_modules() if isinstance(m, layers.Conv2dP)]


def test_the_signature_covers_every_convolution(seg):
    """one (weight, bias) address pair per Conv2dP of the model, depthwise layers included; two calls on an untouched model agree"""
    from pfst_amd import layers
    convs = named_convs(seg)
    assert len(convs) > 60
    sig = seg.repack_signature(True)
    assert len(sig) == len(layers.repack_key(True)) + 1 + 2 * len(convs)
    assert sig == seg.repack_signature(True)
    assert sig != seg.repack_signature(False)
    ptrs = set(sig[len(layers.repack_key(True)) + 1:])
    for name, c in convs:
        assert c.weight.data_ptr() in ptrs, name
        if c.bias is not None:
            assert c.bias.data_ptr() in ptrs, name
    assert sum(c.bias is not None for _, c in convs) == 2           # the two classifiers


def test_rebinding_any_single_weight_or_bias_changes_the_decision(seg):
    """`p.data = other storage` on each conv weight and each conv bias in turn, same values: the signature moves every time and stays
    moved (the new storage is what the next plan records), and never returns to an earlier one while that storage is alive"""
    keep = []
    for name, c in named_convs(seg):
        for p in (c.weight, c.bias):
            if p is None:
                continue
            before = seg.repack_signature(True)
            keep.append(p.data)                      # the old storage stays alive, as it does inside a recorded plan
            p.data = p.data.clone()
            after = seg.repack_signature(True)
            assert after != before, f'{name}: a rebound tensor of {tuple(p.shape)} leaves the decision unchanged'
            assert after == seg.repack_signature(True)
    assert len(keep) > 60


def test_replacing_any_conv_changes_the_decision(seg):
    """every Conv2dP swapped for a new module of the same geometry (setattr on its parent): the signature moves, the conv list follows"""
    from pfst_amd import layers
    for name, c in named_convs(seg):
        parent = seg.get_submodule(name.rsplit('.', 1)[0]) if '.' in name else seg
        before = seg.repack_signature(True)
        new = layers.Conv2dP(c.cin, c.cout, c.k, c.stride, c.padding, c.dilation, c.groups, bias=c.bias is not None)
        setattr(parent, name.rsplit('.', 1)[-1], new)
        after = seg.repack_signature(True)
        assert after != before, name
        walk = seg.__dict__['_conv_list']
        assert any(m is new for m in walk) and not any(m is c for m in walk), name
        assert [id(m) for m in walk] == [id(m) for _, m in named_convs(seg)], name


def test_a_new_classifier_with_another_class_count_changes_the_decision(seg):
    from pfst_amd import layers
    before = seg.repack_signature(False)
    old = seg.decode_head.conv_seg
    seg.decode_head.conv_seg = layers.Conv2dP(old.cin, 9, 1, bias=True)
    after = seg.repack_signature(False)
    assert after != before and len(after) == len(before)
    # a replaced ancestor (the whole auxiliary head) as well
    import copy
    before = after
    seg.auxiliary_head = copy.deepcopy(seg.auxiliary_head)
    assert seg.repack_signature(False) != before


SWITCHES = [('layers', 'CONV_MATH', 'bf16x6'), ('layers', 'CONV_MATH', 'f32'), ('layers', 'WINOGRAD', False), ('layers', 'WINO_MIN_CC', 256 * 256),
            ('layers', 'WINO_MIN_CC_WGRAD', 256 * 256), ('ops', 'WINO_TILE', 2), ('ops', 'F16X3_MIN_ROWS', 128), ('batch', 'enabled', False)]


@pytest.mark.parametrize('where,name,value', SWITCHES)
def test_each_switch_changes_the_decision(seg, where, name, value):
    from pfst_amd import hip_ops, layers
    holder = dict(layers=layers, ops=hip_ops, batch=layers.WeightBatch)[where]
    old = getattr(holder, name)
    assert old != value
    before = seg.repack_signature(True)
    setattr(holder, name, value)
    try:
        assert seg.repack_signature(True) != before
    finally:
        setattr(holder, name, old)
    assert seg.repack_signature(True) == before


def test_need_dgrad_changes_the_decision(seg):
    assert seg.repack_signature(True) != seg.repack_signature(False)
    assert seg.repack_signature(1) == seg.repack_signature(True)


def test_in_place_updates_and_zero_grad_leave_the_decision_alone(seg):
    before = seg.repack_signature(True)
    with torch.no_grad():
        for p in seg.parameters():
            p.mul_(1.7).add_(0.01)
    assert seg.repack_signature(True) == before
    for p in seg.parameters():
        p.grad = torch.zeros_like(p)
    assert seg.repack_signature(True) == before
    seg.zero_grad(set_to_none=False)
    assert seg.repack_signature(True) == before
    seg.zero_grad(set_to_none=True)
    assert seg.repack_signature(True) == before
    with torch.no_grad():
        for p in seg.parameters():
            p.copy_(torch.zeros_like(p))
    assert seg.repack_signature(True) == before
    # BatchNorm parameters are not weight images: rebinding one leaves the packing decision alone (the arena re-adopts it, below)
    bn = seg.backbone.layer1[0].bn1
    bn.weight.data = bn.weight.data.clone()
    assert seg.repack_signature(True) == before


# ---------------------------------------------------------------------------------------------------------------------- the arena
@pytest.fixture()
def arena_model():
    import pfst_amd  # noqa: F401
    from pfst_amd.engine import ParamArena
    from pfst_amd.registry import SEGMENTORS
    model = SEGMENTORS.build(model_cfg())
    arena = ParamArena(list(model.named_parameters()), torch.device('cpu'), with_grad=True)
    arena.sync(model)
    return model, arena


def test_a_rebound_parameter_is_readopted_into_its_slot(arena_model):
    """`.data` of a conv weight, a BatchNorm weight and a bias pointed at other storage with other values: sync copies the values into the
    slot and rebinds `.data` to it; every other slot and every byte of padding is untouched, and so is the gradient view"""
    model, arena = arena_model
    picks = {'backbone.layer2.1.conv2.weight': None, 'backbone.layer1.0.bn1.weight': None, 'decode_head.conv_seg.bias': None}
    params = dict(model.named_parameters())
    flat_before = arena.data.clone()
    for i, name in enumerate(picks):
        p = params[name]
        picks[name] = torch.randn(p.shape, generator=torch.Generator().manual_seed(i))
        p.data = picks[name].clone()
        assert p.data_ptr() != arena.view(arena.data, name).data_ptr()
    arena.sync(model)
    want = flat_before.clone()
    for name, val in picks.items():
        p = params[name]
        assert p.data_ptr() == arena.view(arena.data, name).data_ptr(), name
        assert p.grad.data_ptr() == arena.view(arena.grad, name).data_ptr(), name
        assert p._pfst_arena is arena
        assert torch.equal(p.data, val), name
        arena.view(want, name).copy_(val)
    assert torch.equal(arena.data, want)
    assert torch.equal(model.state_dict()['backbone.layer2.1.conv2.weight'], picks['backbone.layer2.1.conv2.weight'])
    arena.sync(model)                                 # nothing moved: nothing changes
    assert torch.equal(arena.data, want)


def test_a_rebound_parameter_of_another_shape_raises(arena_model):
    model, arena = arena_model
    p = model.decode_head.conv_seg.bias
    p.data = torch.zeros(p.numel() + 1)
    with pytest.raises(RuntimeError, match=r"decode_head\.conv_seg\.bias"):
        arena.sync(model)


@pytest.mark.parametrize('how', ['setattr', 'assign', 'module'])
def test_a_replaced_parameter_object_raises_naming_it(arena_model, how):
    """the optimizer and the arena hold the old object: stepping would train a tensor the model no longer reads"""
    from pfst_amd import layers
    model, arena = arena_model
    flat_before = arena.data.clone()
    if how == 'setattr':
        bn = model.backbone.layer3[2].bn2
        bn.weight = torch.nn.Parameter(bn.weight.data.clone())
        name = r'backbone\.layer3\.2\.bn2\.weight'
    elif how == 'assign':
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(sd, assign=True)
        name = r'backbone\.stem\.0\.weight'                # the first one the walk meets
    else:
        old = model.decode_head.conv_seg
        model.decode_head.conv_seg = layers.Conv2dP(old.cin, 9, 1, bias=True)
        name = r'decode_head\.conv_seg\.weight'
    with pytest.raises(RuntimeError, match=name):
        arena.sync(model)
    assert torch.equal(arena.data, flat_before)
    with pytest.raises(RuntimeError, match=name):      # and again: the error does not clear itself
        arena.sync(model)
