"""The code that decides once and then replays, bit for bit, against parameters that were rebound under it.

A. EncoderDecoder.repack_weights replays recorded packing launches (and layers.WeightBatch its job tables) while repack_signature stands.
   After a replay -- weights changed in place, a weight's `.data` rebound, a Conv2dP replaced, need_dgrad or a switch flipped -- every weight
   image and every published maximum equals, with torch.equal, a fresh per-layer pack of a second model that has never replayed
   (WeightBatch.enabled = False) and was loaded from the first model's state_dict() at that moment.
C. Continuing must equal restarting: in deterministic mode a model that took a step, had parameters rebound (same values in other storage;
   other values; zero_grad(set_to_none=True)) and took another step equals, bit for bit, a model built fresh from its state_dict() and its
   optimizer's state_dict() at the moment after the event -- through EncoderDecoder.train_step with SGD and PFGST.train_step with AdamW,
   for a student and for a teacher parameter.  A replaced Parameter OBJECT raises.
D. hip_ops.h2d_small with the same tag twice while the stream is busy: each device tensor holds its own values."""
import random

import numpy as np
import pytest
import torch

from helpers import model_cfg, to_dev, uda_cfg
from test_supervised_gpu import build_model, seeded_segmentor_state, sup_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
IMAGES = ('w4f', 'w4d', 'uf', 'ud', 'wf', 'wd', 'w6f', 'w6d')
MAXIMA = ('w_amax', 'uf_amax', 'ud_amax')


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from pfst_amd import hip_ops
    return hip_ops


def g(seed=0):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------- A. weight images
def live_attrs(c, need_dgrad):
    """the images and maxima Conv2dP.repack writes for plan(need_dgrad) -- what the layer's kernels read.  (A buffer of an earlier plan, a
    transform-domain set after WINOGRAD was switched off, stays allocated and stale by design: nothing reads it.)"""
    if c.depthwise:
        return []
    p = c.plan(need_dgrad)
    out = []
    if p.wino:
        out += ['uf'] + (['ud'] if need_dgrad else [])
        if p.wino_f16:
            out += ['uf_amax'] + (['ud_amax'] if need_dgrad else [])
    out += [a for a, on in (('wf', p.fp32_f), ('wd', p.fp32_d), ('w4f', p.f16_f), ('w4d', p.f16_d), ('w6f', p.split_f), ('w6d', p.split_d)) if on]
    if p.f16_f or p.f16_d:
        out.append('w_amax')
    return out


def snapshot(model, need_dgrad, ops, fresh=False):
    """{(layer, attribute): clone} of every live image, the maxima reduced per slot group, + the layer's modes.  fresh: the model was packed
    once, under this plan: then the live set must be everything it holds (the table above misses nothing)"""
    from pfst_amd import layers
    out = {}
    for name, c in model.named_modules():
        if not isinstance(c, layers.Conv2dP):
            continue
        live = live_attrs(c, need_dgrad)
        if fresh:
            held = [a for a in IMAGES + MAXIMA if getattr(c, a) is not None]
            assert sorted(held) == sorted(live), (name, held, live)
        for a in live:
            t = getattr(c, a)
            if t is None:
                out[name, a] = None                  # a layer that was never packed
            elif a in MAXIMA:
                out[name, a] = t.view(-1, ops.AMAX_SUB).max(dim=1).values.clone()
            else:
                out[name, a] = t.clone()
        out[name, 'modes'] = (c.wino, c.wino_f16, c.f16_f, c.f16_d, c.split_f, c.split_d)
    return out


def new_segmentor(seed=None):
    import pfst_amd  # noqa: F401
    from pfst_amd.registry import SEGMENTORS
    from pfst_amd.synthetic import fill_state_dict
    model = SEGMENTORS.build(model_cfg())
    if seed is not None:
        fill_state_dict(model.state_dict(), seed)
    return model


class Reference:
    """the second model: WeightBatch.enabled = False around everything it does, so it has no plan and never replays; loaded from the model
    under test each time it is asked"""

    def __init__(self, ops):
        self.ops, self.model, self.fresh = ops, None, True

    def images(self, model, need_dgrad, prepare=None):
        from pfst_amd import layers
        was, layers.WeightBatch.enabled = layers.WeightBatch.enabled, False
        try:
            if self.model is None or prepare is not None:
                self.model, self.fresh = new_segmentor(), True
                if prepare is not None:
                    prepare(self.model)
                self.model.to(DEV)
            res = self.model.load_state_dict(model.state_dict(), strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            self.model.repack_weights(need_dgrad)
            assert self.model.__dict__.get('_repack_plan') is None
            snap = snapshot(self.model, need_dgrad, self.ops, fresh=self.fresh)
            self.fresh = False
            return snap
        finally:
            layers.WeightBatch.enabled = was


def differences(got, want):
    if got.keys() != want.keys():
        return [f'different image sets: {sorted(set(got) ^ set(want))[:6]}']
    bad = []
    for k, w in want.items():
        gk = got[k]
        if k[1] == 'modes':
            ok = gk == w
        else:
            ok = gk is not None and gk.shape == w.shape and torch.equal(gk, w)
        if not ok:
            bad.append('.'.join(k))
    return bad


class RepackCalls:
    """counts Conv2dP.repack calls (the walk) while active: a replay makes none"""

    def __enter__(self):
        from pfst_amd import layers
        self.cls, self.orig, self.seen = layers.Conv2dP, layers.Conv2dP.repack, []
        orig, seen = self.orig, self.seen

        def repack(conv, *a, **kw):
            seen.append(conv)
            return orig(conv, *a, **kw)
        layers.Conv2dP.repack = repack
        return self

    def __exit__(self, *a):
        self.cls.repack = self.orig


@pytest.fixture()
def switches():
    """the switches of layers.repack_key, restored afterwards"""
    from pfst_amd import hip_ops, layers
    names = [(layers, n) for n in ('CONV_MATH', 'WINOGRAD', 'WINO_MIN_CC', 'WINO_MIN_CC_WGRAD')] + \
            [(hip_ops, 'WINO_TILE'), (hip_ops, 'F16X3_MIN_ROWS'), (layers.WeightBatch, 'enabled')]
    old = [getattr(h, n) for h, n in names]
    try:
        yield
    finally:
        for (h, n), v in zip(names, old):
            setattr(h, n, v)


# a layer of each packing family (tests/test_conv_dispatch_cpu.py has the whole table): under f16x3 layer1's 3x3 is convolved directly
# from two-piece fp16 images and layer3's / layer4's go through the Winograd domain (WeightBatch packs both kinds); under bf16x6 the
# same layers are split-packed per layer; the classifier's data gradient and the stem's forward read fp32 K-major images in every mode
REBOUND = ['backbone.layer1.0.conv2', 'backbone.layer3.1.conv2', 'backbone.layer4.0.conv2', 'decode_head.conv_seg', 'backbone.stem.0']


@pytest.mark.parametrize('need_dgrad', [True, False])
@pytest.mark.parametrize('math', ['f32', 'bf16x6', 'f16x3'])
def test_replayed_weight_images_follow_the_parameters(ops, switches, math, need_dgrad):
    """after a first repack_weights that recorded a plan: weights changed in place (the replay branch, proven by counting Conv2dP.repack
    calls); one mid-network weight rebound with other values, a layer of each packing family in turn, and the classifier's bias; the
    classifier replaced by a new module with another output count.  Each state against the fresh per-layer pack."""
    from pfst_amd import layers
    layers.CONV_MATH, layers.WeightBatch.enabled = math, True
    model = new_segmentor(3).to(DEV)
    ref = Reference(ops)
    named = dict(model.named_modules())
    fam = {n: named[n].plan(need_dgrad) for n in REBOUND}
    assert fam['backbone.layer3.1.conv2'].wino and fam['backbone.layer4.0.conv2'].wino and fam['backbone.stem.0'].fp32_f
    assert fam['backbone.layer1.0.conv2'].f16_f == (math == 'f16x3') and fam['backbone.layer1.0.conv2'].split_f == (math == 'bf16x6')
    assert fam['backbone.layer3.1.conv2'].wino_f16 == (math == 'f16x3')
    assert fam['decode_head.conv_seg'].fp32_d == need_dgrad and fam['decode_head.conv_seg'].split_f == (math != 'f32')
    problems = []

    def check(stage, prepare=None):
        bad = differences(snapshot(model, need_dgrad, ops), ref.images(model, need_dgrad, prepare))
        print(f'{stage}: {len(bad)} images differ from the fresh per-layer pack {bad[:4]}')
        if bad:
            problems.append((stage, len(bad), bad[:4]))

    model.repack_weights(need_dgrad)
    plan = model.__dict__['_repack_plan']
    assert plan is not None
    check('first pack')
    assert not problems

    # nothing rebound, weights changed in place: the replay branch, reading live storage
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.7).add_(0.01)
    with RepackCalls() as calls:
        model.repack_weights(need_dgrad)
    assert not calls.seen and model.__dict__['_repack_plan'] is plan, 'in-place updates must take the replay branch'
    check('in place')
    assert not problems, problems

    # one weight rebound with other values
    for i, name in enumerate(REBOUND):
        conv = named[name]
        conv.weight.data = (torch.randn(conv.weight.shape, generator=g(40 + i)) * 0.05).to(DEV)
        model.repack_weights(need_dgrad)
        check(f'rebound {name}.weight')
    conv = model.decode_head.conv_seg
    conv.bias.data = torch.randn(conv.bias.shape, generator=g(50)).to(DEV)
    with RepackCalls() as calls:
        model.repack_weights(need_dgrad)
    if not calls.seen:
        problems.append(('rebound decode_head.conv_seg.bias', 'replayed: the bias is not part of the decision'))
    check('rebound decode_head.conv_seg.bias')
    with RepackCalls() as calls:                     # ... and the new plan replays in its turn
        model.repack_weights(need_dgrad)
    if calls.seen:
        problems.append(('after the rebinds', f'{len(calls.seen)} layers walked again with nothing changed'))

    # a Conv2dP replaced by a new module
    old = model.decode_head.conv_seg
    torch.manual_seed(7)
    new = layers.Conv2dP(old.cin, 9, 1, bias=True).to(DEV)
    model.decode_head.conv_seg = new
    with RepackCalls() as calls:
        model.repack_weights(need_dgrad)
    if not any(c is new for c in calls.seen):
        problems.append(('replaced conv_seg', 'the new module was not packed'))
    if any(c is old for c in calls.seen):
        problems.append(('replaced conv_seg', 'the old module is still walked'))

    def same_head(m):
        m.decode_head.conv_seg = layers.Conv2dP(old.cin, 9, 1, bias=True)
    check('replaced conv_seg', prepare=same_head)
    assert not problems, problems


@pytest.mark.parametrize('math', ['f32', 'bf16x6', 'f16x3'])
def test_data_gradient_images_after_need_dgrad_went_off_and_on(ops, switches, math):
    """need_dgrad True -> in-place weight change -> False -> True: the data-gradient images are those of the current weights, and the
    forward images in between as well"""
    from pfst_amd import layers
    layers.CONV_MATH, layers.WeightBatch.enabled = math, True
    model = new_segmentor(3).to(DEV)
    ref = Reference(ops)
    model.repack_weights(True)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.7).add_(0.01)
    model.repack_weights(False)
    bad = differences(snapshot(model, False, ops), ref.images(model, False))
    assert not bad, ('need_dgrad False', len(bad), bad[:6])
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.5).sub_(0.02)
    model.repack_weights(True)
    bad = differences(snapshot(model, True, ops), ref.images(model, True))
    assert not bad, ('need_dgrad True again', len(bad), bad[:6])
    assert sum(k[1] in ('ud', 'wd', 'w4d', 'w6d') for k in snapshot(model, True, ops)) > 50


FLIPS = [('layers', 'CONV_MATH', 'bf16x6'), ('layers', 'CONV_MATH', 'f32'), ('layers', 'WINOGRAD', False), ('layers', 'WINO_MIN_CC', 256 * 256),
         ('layers', 'WINO_MIN_CC_WGRAD', 256 * 256), ('ops', 'WINO_TILE', 2), ('ops', 'F16X3_MIN_ROWS', 64), ('batch', 'enabled', False)]


def test_each_switch_flipped_between_two_calls_forces_a_walk(ops, switches):
    """every switch of layers.repack_key in turn, off its default and back: the call after the flip walks the layers again and leaves the
    images of a fresh per-layer pack under that switch -- and the call after the flip back those of the default"""
    from pfst_amd import hip_ops, layers
    holders = dict(layers=layers, ops=hip_ops, batch=layers.WeightBatch)
    layers.CONV_MATH, layers.WeightBatch.enabled = 'f16x3', True
    model = new_segmentor(3).to(DEV)
    ref = Reference(ops)
    model.repack_weights(True)
    problems = []
    for where, name, value in FLIPS:
        h = holders[where]
        default = getattr(h, name)
        assert default != value
        for v, what in ((value, f'{name} = {value}'), (default, f'{name} back to {default}')):
            setattr(h, name, v)
            with torch.no_grad():
                for p in model.parameters():
                    p.mul_(1.01)
            with RepackCalls() as calls:
                model.repack_weights(True)
            if not calls.seen:
                problems.append((what, 'replayed'))
            # (the reference flips WeightBatch.enabled itself; everything else it reads as set here)
            bad = differences(snapshot(model, True, ops), ref.images(model, True))
            print(f'{what}: {len(bad)} images differ {bad[:4]}')
            if bad:
                problems.append((what, len(bad), bad[:4]))
    assert not problems, problems


# ---------------------------------------------------------------------------------------------------------------------- C. continue = restart
@pytest.fixture()
def deterministic():
    from pfst_amd import hip_ops
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        yield
    finally:
        hip_ops.set_deterministic(was)


def cpu_copy(obj):
    if torch.is_tensor(obj):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return type(obj)((k, cpu_copy(v)) for k, v in obj.items())
    if isinstance(obj, (list, tuple)):
        return type(obj)(cpu_copy(v) for v in obj)
    return obj


def assert_same_state(got, want, what):
    assert list(got) == list(want)
    bad = []
    for k in want:
        a, b = got[k], want[k]
        if torch.is_tensor(b):
            if not torch.equal(a, b):
                bad.append((k, int((a != b).sum()), b.numel()))
        else:
            assert a == b, (what, k, a, b)
    assert not bad, f'{what}: {len(bad)} of {len(want)} entries differ between the model that continued and the one rebuilt: {bad[:6]}'


SUP_PICKS = ('backbone.layer2.1.conv2.weight', 'backbone.layer3.0.bn1.weight', 'decode_head.conv_seg.bias')


def rebind(params, names, other_values):
    for i, n in enumerate(names):
        p = params[n]
        if other_values is None:
            p.data = p.data.clone()
        else:
            p.data = other_values(n, p, i)
        assert p.data_ptr() != p._pfst_arena.view(p._pfst_arena.data, n).data_ptr()


@pytest.mark.parametrize('event', ['same_values', 'other_values', 'zero_grad_none'])
def test_supervised_step_after_an_event_equals_a_restart(deterministic, event):
    """EncoderDecoder.train_step with SGD (momentum 0.9): model B steps, the event happens, model C is built from B's state_dict() and B's
    optimizer state; both step on the same batch: equal log values, and every entry of state_dict() equal bit for bit.
    (tests/test_supervised_gpu.py::test_resume_is_bit_exact is the oracle: a rebuilt model steps like one that continued.)"""
    state = seeded_segmentor_state(9)
    batches = [to_dev(sup_batch(1234 + i), DEV) for i in range(2)]
    b_model, b_opt = build_model(state)
    b_model.train_step(batches[0], b_opt)
    params = dict(b_model.named_parameters())
    if event == 'same_values':
        rebind(params, SUP_PICKS, None)
    elif event == 'other_values':
        rebind(params, SUP_PICKS, lambda n, p, i: p.data * 0.9 + 0.01 * (i + 1))
    else:
        b_opt.zero_grad(set_to_none=True)
        b_model.zero_grad(set_to_none=True)
    c_model, c_opt = build_model(cpu_copy(b_model.state_dict()))
    c_opt.load_state_dict(cpu_copy(b_opt.state_dict()))
    out_b = b_model.train_step(batches[1], b_opt)
    out_c = c_model.train_step(batches[1], c_opt)
    torch.cuda.synchronize()
    print('continued:', out_b['log_vars'], '\nrebuilt:  ', out_c['log_vars'])
    assert out_b['log_vars'] == out_c['log_vars']
    assert_same_state(b_model.state_dict(), c_model.state_dict(), event)
    for n in SUP_PICKS:                               # re-adopted: the module reads its arena slot again
        assert params[n].data_ptr() == b_model.param_arena.view(b_model.param_arena.data, n).data_ptr(), n
    mom_b, mom_c = list(b_opt._flat.values())[0]['buf'], list(c_opt._flat.values())[0]['buf']
    assert torch.equal(mom_b, mom_c) and float(mom_b.abs().max()) > 0


def test_supervised_step_with_a_replaced_parameter_object_raises(deterministic):
    """the optimizer holds the old object: RuntimeError naming the parameter, and the model is not stepped"""
    b_model, b_opt = build_model(seeded_segmentor_state(9))
    batch = to_dev(sup_batch(1234), DEV)
    b_model.train_step(batch, b_opt)
    torch.cuda.synchronize()
    before = b_model.param_arena.data.clone()
    bn = b_model.backbone.layer3[0].bn1
    bn.weight = torch.nn.Parameter(bn.weight.data.clone())
    with pytest.raises(RuntimeError, match=r'backbone\.layer3\.0\.bn1\.weight'):
        b_model.train_step(batch, b_opt)
    torch.cuda.synchronize()
    assert torch.equal(b_model.param_arena.data, before)
    b_model.load_state_dict(cpu_copy(b_model.state_dict()), assign=True)
    with pytest.raises(RuntimeError, match=r'backbone\.stem\.0\.weight'):
        b_model.train_step(batch, b_opt)


def build_pfgst(state):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import UDA
    model = UDA.build(uda_cfg(threshold=0.30))
    res = model.load_state_dict(state, strict=False)
    assert not res.unexpected_keys
    model.cuda()
    return model, build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))


def seeded(seed):
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed); torch.cuda.manual_seed_all(seed)


PFGST_PICKS = ('backbone.layer2.1.conv2.weight', 'backbone.layer3.0.bn1.weight', 'decode_head.conv_seg.bias',
               'backbone.layer4.2.conv3.weight', 'auxiliary_head.convs.0.bn.bias', 'auxiliary_head.conv_seg.bias')


@pytest.mark.parametrize('side', ['student', 'teacher'])
def test_pfgst_step_after_rebinding_equals_a_restart(deterministic, side):
    """PFGST.train_step with AdamW at 2 x 128^2.  The event, on the student's or on the teacher's parameters: a conv weight, a BatchNorm
    weight and a bias rebound to other storage with the same values; three more rebound to the values of the OTHER network's tensor (the
    swap an evaluation hook makes); and the optimizer's zero_grad(set_to_none=True).  Then as above, for every entry of the wrapper's
    state_dict() -- student, teacher, iteration count -- and of the teacher's own.  Last, a replaced Parameter object on that side raises."""
    from oracle import pfst_oracle as O
    from helpers import seeded_pfgst_state
    from pfst_amd.synthetic import synth_batch
    both, _, _ = seeded_pfgst_state(O, 9)
    batches = [to_dev(synth_batch(2, 128, 6, seed=77 + i), DEV) for i in range(2)]
    b_model, b_opt = build_pfgst(both)
    seeded(5)
    b_model.train_step(batches[0], b_opt)
    nets = dict(student=b_model.get_model(), teacher=b_model.get_ema_model())
    mine, other = dict(nets[side].named_parameters()), dict(nets['teacher' if side == 'student' else 'student'].named_parameters())
    rebind(mine, PFGST_PICKS[:3], None)
    rebind(mine, PFGST_PICKS[3:], lambda n, p, i: other[n].data.clone())
    b_opt.zero_grad(set_to_none=True)
    c_model, c_opt = build_pfgst(cpu_copy(b_model.state_dict()))
    assert c_model.local_iter == b_model.local_iter == 1
    c_opt.load_state_dict(cpu_copy(b_opt.state_dict()))
    seeded(6)
    out_b = b_model.train_step(batches[1], b_opt)['log_vars']
    seeded(6)
    out_c = c_model.train_step(batches[1], c_opt)['log_vars']
    torch.cuda.synchronize()
    print('continued:', out_b, '\nrebuilt:  ', out_c)
    assert out_b == out_c
    assert_same_state(b_model.state_dict(), c_model.state_dict(), side)
    assert_same_state(b_model.get_ema_model().state_dict(), c_model.get_ema_model().state_dict(), side + ', teacher')
    flat_b, flat_c = list(b_opt._flat.values())[0], list(c_opt._flat.values())[0]
    assert flat_b['step'] == flat_c['step'] == 2 and torch.equal(flat_b['m'], flat_c['m']) and torch.equal(flat_b['v'], flat_c['v'])

    bn = nets[side].backbone.layer3[0].bn1
    bn.weight = torch.nn.Parameter(bn.weight.data.clone(), requires_grad=side == 'student')
    with pytest.raises(RuntimeError, match=r'backbone\.layer3\.0\.bn1\.weight'):
        b_model.train_step(batches[1], b_opt)


# ---------------------------------------------------------------------------------------------------------------------- D. h2d_small
def busy(ops, y, x, launches=60):
    """some milliseconds of device work on the current stream: a chain of axpy launches over 256 MB buffers"""
    for _ in range(launches):
        ops.axpy_(y, x, 1e-3)


@pytest.mark.parametrize('side_stream', [False, True])
def test_h2d_small_twice_with_one_tag_under_a_busy_stream(ops, side_stream):
    """the second and the third call rewrite the cached pinned staging buffer of the first: each device tensor must still receive the
    values of its own call, on the current stream and on a side stream"""
    dev = torch.device('cuda', torch.cuda.current_device())
    n = 64 * 1024 * 1024
    y, x = torch.zeros(n, device=dev), torch.ones(n, device=dev)
    hosts = [torch.full((3, 5), float(i + 1)) + torch.arange(15.0).view(3, 5) / 100 for i in range(3)]
    ints = [torch.arange(7, dtype=torch.int32) + 10 * i for i in range(3)]
    tag = ('test_host_caches', side_stream)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        busy(ops, y, x)
        got = [ops.h2d_small(h, dev, tag) for h in hosts[:2]]
        got_i = [ops.h2d_small(h, dev, tag) for h in ints[:2]]
        busy(ops, y, x)
        got.append(ops.h2d_small(hosts[2], dev, tag))
        got_i.append(ops.h2d_small(ints[2], dev, tag))
        y.record_stream(stream), x.record_stream(stream)
        for t in got + got_i:
            t.record_stream(stream)
    torch.cuda.synchronize()
    for i, (t, h) in enumerate(zip(got + got_i, hosts + ints)):
        assert t.device == dev and t.dtype == h.dtype
        assert torch.equal(t.cpu(), h), f'call {i % 3 + 1} of 3 with one tag received {t.cpu().flatten()[:4].tolist()}, sent {h.flatten()[:4].tolist()}'
    # a later call, long after the copies have run, takes the same buffer and does not wait
    again = ops.h2d_small(hosts[0], dev, tag)
    torch.cuda.synchronize()
    assert torch.equal(again.cpu(), hosts[0])
