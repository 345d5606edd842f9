"""Supervised training on the GPU: the flat SGD kernel against torch.optim.SGD, EncoderDecoder.train_step against the CPU oracle (log
values, gradients against fp64), the optimizer inside the step, bit-exact resume, the train / test CLIs on a config without `uda` (and a
self-training run started from that checkpoint), and the overlapped gradient reducer behind a supervised step."""
import os
import sys
from collections import OrderedDict

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import model_cfg, to_dev, uda_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-3                                    # tests/test_train_step_gpu.py
SCHEDULE_40K = dict(optimizer=dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005),
                    lr_config=dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False), max_iters=40000)


def g(seed=0):
    return torch.Generator().manual_seed(seed)


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def assert_close(a, b, tol=1e-3, what=''):
    """tests/test_hip_ops.py's helper, restated: max |a - b| / max |b|"""
    e = rel_err(a, b)
    print(f'{what}: rel err {e:.3e} (bound {tol})')
    assert e < tol, f'{what} rel err {e:.3e} >= {tol}'


def rel(a, b):
    """tests/test_train_step_gpu.py's norm-wise error"""
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(params=['f32', 'bf16x6', 'f16x3'])
def conv_math(request):
    from pfst_amd import layers
    prev, layers.CONV_MATH = layers.CONV_MATH, request.param
    yield request.param
    layers.CONV_MATH = prev


# ---------------------------------------------------------------------------------------------------------------------- 1. kernel
SGD_CASES = [
    # momentum, dampening, nesterov, weight_decay, grad_scale
    (0.0, 0.0, False, 0.0, 1.0),
    (0.9, 0.0, False, 5e-4, 1.0),
    (0.9, 0.1, False, 5e-4, 1.0),
    (0.9, 0.0, True, 5e-4, 1.0),
    (0.9, 0.0, False, 5e-4, 0.125),
]


@pytest.mark.parametrize('n', [10007, 'arena'])
@pytest.mark.parametrize('momentum,dampening,nesterov,wd,gscale', SGD_CASES)
def test_sgd_step_against_torch(n, momentum, dampening, nesterov, wd, gscale):
    """three steps of pfst_sgd_step against torch.optim.SGD on the CPU: a length that is no multiple of 4 (float4 body + scalar tail) and
    one of the size of the segmentor's arena (the grid-stride loop runs many rounds); grad_scale against pre-scaled gradients"""
    from pfst_amd import hip_ops as ops
    if n == 'arena':
        import pfst_amd  # noqa: F401
        from pfst_amd.registry import build_segmentor
        n = sum((p.numel() + 3) // 4 * 4 for p in build_segmentor(model_cfg()).parameters())
        assert n > 40_000_000
    p = torch.randn(n, generator=g(1)).requires_grad_()
    grad = torch.randn(n, generator=g(3))
    lr = 0.01
    opt = torch.optim.SGD([p], lr=lr, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    pd = p.detach().clone().to(DEV)
    buf = torch.full((n,), float('nan'), device=DEV) if momentum != 0 else None         # the first step must not read it
    for step in (1, 2, 3):
        p.grad = grad * step * gscale
        opt.step()
        ops.sgd_step_(pd, (grad * step).to(DEV), buf, lr, momentum, dampening, wd, nesterov, first_step=step == 1, grad_scale=gscale)
    print(f'elements that differ from torch bit for bit: {int((pd.cpu() != p.detach()).sum())} of {n}')
    assert_close(pd, p, 1e-6, 'sgd parameters')
    if momentum != 0:
        assert_close(buf, opt.state[p]['momentum_buffer'], 1e-6, 'sgd momentum buffer')


def test_sgd_step_on_a_loose_unaligned_tensor():
    """a tensor that does not start on a 16-byte boundary takes the scalar loop"""
    from pfst_amd import hip_ops as ops
    n = 1001
    p = torch.randn(n, generator=g(5)).requires_grad_()
    grad = torch.randn(n, generator=g(6))
    opt = torch.optim.SGD([p], lr=0.05, momentum=0.9, weight_decay=5e-4)
    store = torch.zeros(n + 1, device=DEV)
    pd = store[1:]
    pd.copy_(p.detach())
    assert pd.data_ptr() % 16 == 4
    buf = torch.empty(n, device=DEV)
    for step in (1, 2):
        p.grad = grad.clone()
        opt.step()
        ops.sgd_step_(pd, grad.to(DEV), buf, 0.05, 0.9, 0.0, 5e-4, False, first_step=step == 1)
    assert_close(pd, p, 1e-6, 'sgd, unaligned')
    assert float(store[0]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------- 2. the step
def seeded_segmentor_state(seed):
    from oracle import pfst_oracle as O
    from pfst_amd.synthetic import fill_state_dict
    return fill_state_dict(O.init_state_dict(6, 3), seed)


def build_model(state, optimizer=None):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.registry import build_segmentor
    model = build_segmentor(model_cfg(dropout=0.0))
    res = model.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    return model, build_optimizer(model, dict(optimizer or SCHEDULE_40K['optimizer']))


def sup_batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return {k: v for k, v in synth_batch(2, 128, 6, seed=seed).items() if not k.startswith('target_')}


def oracle_step(state, batch, dtype):
    """oracle.segmentor_forward_train + parse_losses + loss.backward() on the CPU -> (log values, {name: gradient})"""
    from oracle import pfst_oracle as O
    sd = OrderedDict((k, (v.to(dtype) if v.is_floating_point() else v).clone()) for k, v in state.items())
    keys = O.param_keys(sd)
    for k in keys:
        sd[k].requires_grad_(True)
    losses = O.segmentor_forward_train(sd, batch['img'].to(dtype), batch['gt_semantic_seg'])[0]
    loss, log = O.parse_losses(losses)
    loss.backward()
    return log, OrderedDict((k, sd[k].grad.clone()) for k in keys)


def test_train_step_matches_oracle(conv_math):
    """log_vars: the reference's keys in its order, each within 1e-3 * max(|ref|, 1e-2).  Gradients by the criterion of
    tests/test_train_step_gpu.py: through ~70 train-mode BatchNorm layers of a random-init network the oracle's own fp32 path is percents
    away from fp64, so every tensor must be as close to the fp64 gradient as the fp32 oracle is (x5, floor 1e-3; the flat gradient x2), and
    the three head tensors next to the loss within 1e-3 of the fp32 oracle directly."""
    from pfst_amd.hostinfo import usable_cpus
    torch.set_num_threads(usable_cpus())
    state = seeded_segmentor_state(9)
    batch = sup_batch()
    olog, g32 = oracle_step(state, batch, torch.float32)
    _, g64 = oracle_step(state, batch, torch.float64)
    model, opt = build_model(state)
    out = model.train_step(to_dev(batch, DEV), opt)
    torch.cuda.synchronize()
    lv = out['log_vars']
    assert list(lv.keys()) == list(olog.keys()) == ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss']
    assert out['num_samples'] == 2 and out['states'] == {} and out['loss'] == lv['loss'] and isinstance(out['loss'], float)
    for k in olog:
        print(f'{conv_math} {k}: {lv[k]!r} oracle {olog[k]!r}')
    for k in olog:
        assert abs(lv[k] - olog[k]) <= TOL * max(abs(olog[k]), 1e-2), (k, lv[k], olog[k])
    arena = model.param_arena
    assert list(arena.names) == list(g64.keys())
    rows = [(name, rel(arena.view(arena.grad, name), g64[name]), rel(g32[name], g64[name])) for name in g64]
    worst = max(rows, key=lambda t: t[1] / max(t[2], 1e-12))
    print(f'{conv_math}: worst per-tensor gradient ratio HIP / oracle-fp32 vs fp64 {worst[1] / max(worst[2], 1e-12):.2f} '
          f'({worst[0]}: {worst[1]:.2e} / {worst[2]:.2e}); worst HIP rel err {max(r[1] for r in rows):.2e}')
    flat_64 = torch.cat([v.flatten() for v in g64.values()])
    flat_o = torch.cat([v.flatten() for v in g32.values()])
    flat_m = torch.cat([arena.view(arena.grad, n).flatten() for n in g64])
    print('flat gradient rel err vs fp64: HIP %.3e  oracle-fp32 %.3e' % (rel(flat_m, flat_64), rel(flat_o, flat_64)))
    for name, a, r in rows:
        assert a <= max(TOL, 5.0 * r), (name, a, r)
    for name in ('decode_head.conv_seg.bias', 'auxiliary_head.conv_seg.weight', 'auxiliary_head.conv_seg.bias'):
        e = rel(arena.view(arena.grad, name), g32[name])
        print(f'   {name}: rel err vs oracle-fp32 {e:.2e}')
        assert e < TOL, (name, e)
    assert rel(flat_m, flat_64) <= max(TOL, 2.0 * rel(flat_o, flat_64))


def test_train_step_bad_labels_vis_states_and_extra_keys():
    from pfst_amd.synthetic import synth_batch
    model, opt = build_model(seeded_segmentor_state(9))
    with pytest.raises(KeyError, match='target_img'):
        model.train_step(to_dev(synth_batch(2, 128, 6), DEV), opt)
    model.return_vis_states = True
    st = model.train_step(to_dev(sup_batch(), DEV), opt)['states']
    assert {'seg_logits', 'decoded_features', 'aux.seg_logits', 'img', 'gt'} <= set(st)
    assert tuple(st['seg_logits'].shape) == (2, 6, 32, 32)
    model.return_vis_states = False
    bad = to_dev(sup_batch(56), DEV)
    bad['gt_semantic_seg'][0, 0, 40:44, 40:44] = 7
    with pytest.raises(ValueError, match='outside'):
        model.train_step(bad, opt)


# ---------------------------------------------------------------------------------------------------------------------- 3. optimizer in the step
def test_sgd_inside_two_train_steps():
    """two steps under the runner's schedule_40k learning rates; a CPU torch.optim.SGD fed the step's own gradients from the same start
    lands on the same parameters: weight decay, the first-step buffer, the learning rate handed over through param_groups"""
    from pfst_amd import supervised
    from pfst_amd.optim import poly_lr
    model, opt = build_model(seeded_segmentor_state(9))
    arena = supervised.ensure_arena(model, torch.device('cuda', torch.cuda.current_device()))
    p = arena.data.clone().cpu().requires_grad_()
    ref = torch.optim.SGD([p], **{k: v for k, v in SCHEDULE_40K['optimizer'].items() if k != 'type'})
    lrs = [poly_lr(0.01, it, 40000, power=0.9, min_lr=1e-4, warmup_iters=0) for it in range(2)]
    assert lrs[0] == 0.01 and 1e-4 < lrs[1] < 0.01
    for it, lr in enumerate(lrs):
        for group in opt.param_groups:
            group['lr'] = lr
        ref.param_groups[0]['lr'] = lr
        model.train_step(to_dev(sup_batch(1234 + it), DEV), opt)
        torch.cuda.synchronize()
        assert model.param_arena is arena
        p.grad = arena.grad.clone().cpu()
        assert float(p.grad.abs().max()) > 0
        ref.step()
    assert len(opt._flat) == 1, 'the whole arena takes one flat launch'
    st = list(opt._flat.values())[0]
    assert_close(arena.data, p, 1e-6, 'parameters after two steps')
    assert_close(st['buf'], ref.state[p]['momentum_buffer'], 1e-6, 'momentum buffer after two steps')
    # the parameters of the module ARE the arena: what a checkpoint saves is what the optimizer stepped
    name = 'decode_head.conv_seg.weight'
    assert torch.equal(model.state_dict()[name], arena.view(arena.data, name))


# ---------------------------------------------------------------------------------------------------------------------- 4. resume
def test_resume_is_bit_exact(tmp_path):
    from pfst_amd import hip_ops
    from pfst_amd.config import Config
    from pfst_amd.runner import IterBasedRunner
    state = seeded_segmentor_state(9)
    batches = [to_dev(sup_batch(1234 + i), DEV) for i in range(2)]

    def make(work):
        cfg = Config(dict(runner=dict(type='IterBasedRunner', max_iters=SCHEDULE_40K['max_iters']), lr_config=dict(SCHEDULE_40K['lr_config']),
                          log_config=dict(interval=1), checkpoint_config=dict(interval=1), optimizer=dict(SCHEDULE_40K['optimizer'])))
        model, opt = build_model(state)
        return model, opt, IterBasedRunner(model, opt, cfg, str(work), log=lambda s: None)

    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        model, opt, runner = make(tmp_path / 'a')
        runner.run(iter(batches), max_iters=2)
        torch.cuda.synchronize()
        want_p, want_b = model.param_arena.data.clone().cpu(), list(opt._flat.values())[0]['buf'].clone().cpu()
        model, opt, runner = make(tmp_path / 'b')
        runner.run(iter(batches[:1]), max_iters=1)
        ck = tmp_path / 'b' / 'iter_1.pth'
        assert ck.exists()
        saved = torch.load(ck, map_location='cpu', weights_only=False)
        assert list(saved['state_dict'])[0].startswith('backbone.') and saved['optimizer']['pfst_flat'][0]['stepped'] is True
        del model, opt, runner
        model, opt, runner = make(tmp_path / 'c')
        runner.resume(str(ck))
        assert runner.iter == 1
        runner.run(iter(batches[1:]), max_iters=2)
        torch.cuda.synchronize()
        got_p, got_b = model.param_arena.data.clone().cpu(), list(opt._flat.values())[0]['buf'].clone().cpu()
    finally:
        hip_ops.set_deterministic(was)
    assert torch.equal(got_p, want_p), f'parameters differ after resume: {int((got_p != want_p).sum())} elements'
    assert torch.equal(got_b, want_b), f'momentum buffer differs after resume: {int((got_b != want_b).sum())} elements'
    assert not torch.equal(want_b, torch.zeros_like(want_b))


# ---------------------------------------------------------------------------------------------------------------------- 5. CLI
def test_supervised_train_cli_test_cli_and_init_student_from(tmp_path):
    """tools/train.py on a config without `uda` (data.train a plain ISPRSDataset dict, schedule_40k's optimizer and schedule, validation),
    tools/test.py on its checkpoint WITHOUT key revision, then a PFGST run started from it with --init-student-from."""
    import json
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import test as test_cli
    import train as train_cli
    from test_data_pipeline_cpu import SOURCE, TARGET, TEST, _tile
    for dom, n in (('pots', 4), ('vaih', 3)):
        os.makedirs(tmp_path / dom / 'img_dir/train'), os.makedirs(tmp_path / dom / 'ann_dir/train')
        for i in range(n):
            img, seg = _tile(7 * n + i, 256)
            Image.fromarray(img).save(tmp_path / dom / 'img_dir/train' / f't{i}.png')
            Image.fromarray(seg).save(tmp_path / dom / 'ann_dir/train' / f't{i}.png')
    small = lambda pl: [dict(s, crop_size=(128, 128)) if s['type'] == 'RandomCrop' else dict(s, size=(128, 128)) if s['type'] == 'Pad' else
                        dict(s, img_scale=(192, 192)) if s['type'] == 'Resize' else s for s in pl]
    test_pl = [TEST[0], dict(TEST[1], img_scale=(128, 128))]
    ds = lambda dom, pl: dict(type='ISPRSDataset', data_root=str(tmp_path / dom), img_dir='img_dir/train', ann_dir='ann_dir/train',
                              gt_seg_map_loader_cfg=dict(reduce_zero_label=True), pipeline=pl)
    tail = ('checkpoint_config = dict(by_epoch=False, interval=%d)\nevaluation = dict(interval=%d, metric="mIoU")\n'
            'log_config = dict(interval=1)\nseed = 0\ndata = %r\n')
    text = ('model = %r\noptimizer = %r\noptimizer_config = dict()\nlr_config = %r\nrunner = dict(type="IterBasedRunner", max_iters=2)\n'
            % (model_cfg(), SCHEDULE_40K['optimizer'], SCHEDULE_40K['lr_config'])
            + tail % (2, 2, dict(samples_per_gpu=2, workers_per_gpu=0, train=ds('pots', small(SOURCE)), val=ds('vaih', test_pl),
                                 test=ds('vaih', test_pl))))
    cfg_path = tmp_path / 'toy_supervised.py'
    cfg_path.write_text(text)
    work = tmp_path / 'work'
    train_cli.main([str(cfg_path), '--work-dir', str(work), '--seed', '0'])
    lines = [json.loads(l) for l in open(work / 'log.json')]
    train = [l for l in lines if l['mode'] == 'train']
    assert [l['iter'] for l in train] == [1, 2]
    assert all(k in train[0] for k in ('decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss'))
    assert train[0]['lr'] == 0.01 and 1e-4 < train[1]['lr'] < 0.01
    val = [l for l in lines if l['mode'] == 'val']
    assert len(val) == 1 and val[0]['iter'] == 2 and 0.0 <= val[0]['mIoU'] <= 100.0 and 'aAcc' in val[0]
    ck = work / 'iter_2.pth'
    assert ck.exists()
    res = test_cli.main([str(cfg_path), str(ck), '--eval', 'mIoU', '--split', 'val'])            # bare keys: no --revise-checkpoint-key
    print('mIoU of the train run %r, of the test CLI %r' % (val[0]['mIoU'], res['mIoU']))
    assert abs(res['mIoU'] - val[0]['mIoU']) < 1e-6
    sup = torch.load(ck, map_location='cpu', weights_only=False)
    assert all(k.split('.')[0] in ('backbone', 'decode_head', 'auxiliary_head') for k in sup['state_dict'])

    # ---- self-training from that checkpoint
    cfg = uda_cfg(threshold=0.3)
    mcfg = cfg.pop('model')
    cfg.pop('max_iters')
    from pfst_amd.presets import LR_CONFIG, OPTIMIZER
    text = ('model = %r\nuda = %r\noptimizer = %r\nlr_config = %r\nrunner = dict(type="IterBasedRunner", max_iters=1)\n'
            % (mcfg, cfg, dict(OPTIMIZER), dict(LR_CONFIG))
            + tail % (1, 0, dict(samples_per_gpu=2, workers_per_gpu=0,
                                 train=dict(type='UDADataset', source=ds('pots', small(SOURCE)), target=ds('vaih', small(TARGET)),
                                            rare_class_sampling=None))))
    uda_path = tmp_path / 'toy_pfst.py'
    uda_path.write_text(text)
    work2 = tmp_path / 'work_uda'
    train_cli.main([str(uda_path), '--work-dir', str(work2), '--seed', '0', '--no-validate', '--init-student-from', str(ck)])
    out = torch.load(work2 / 'iter_1.pth', map_location='cpu', weights_only=False)['state_dict']
    params = [k for k, v in sup['state_dict'].items() if not any(k.endswith(s) for s in ('running_mean', 'running_var', 'num_batches_tracked'))]
    assert len(params) > 150
    for k in params:
        # _init_ema_weights runs at local_iter 0: the teacher is the (loaded) student before its first update
        assert torch.equal(out['ema_model.' + k], sup['state_dict'][k]), k
    moved = [k for k in params if not torch.equal(out['model.' + k], sup['state_dict'][k])]
    assert len(moved) > 150, 'the student trained on from the loaded weights'
    nbt = [k for k in sup['state_dict'] if k.endswith('num_batches_tracked')]
    assert nbt
    assert all(int(out['model.' + k]) > int(sup['state_dict'][k]) for k in nbt), 'the loaded BatchNorm step counts advance'
    # any missing or unexpected key fails loudly
    broken = dict(sup, state_dict=OrderedDict((k, v) for k, v in sup['state_dict'].items() if k != 'decode_head.conv_seg.bias'))
    torch.save(broken, tmp_path / 'broken.pth')
    with pytest.raises(KeyError, match='missing'):
        train_cli.main([str(uda_path), '--work-dir', str(tmp_path / 'work3'), '--seed', '0', '--no-validate',
                        '--init-student-from', str(tmp_path / 'broken.pth')])
    with pytest.raises(SystemExit):
        train_cli.main([str(cfg_path), '--work-dir', str(tmp_path / 'work4'), '--init-student-from', str(ck)])     # not a `uda` config


# ---------------------------------------------------------------------------------------------------------------------- 6. reducer
def _rccl_supervised_worker(rank, world, port, outdir):
    """one supervised step in a single-rank RCCL group with the exchange forced on (PFST_DDP_FORCE=1), overlap on"""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      PFST_DDP_FORCE='1', PFST_DDP_OVERLAP='1', PFST_DDP_BUCKET_MB='8')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=rank, world_size=world, device_id=torch.device('cuda', 0))
    from pfst_amd import dist as pdist
    from pfst_amd import layers
    assert pdist.is_distributed() and pdist.OVERLAP_ALLREDUCE
    snaps, markers = [], []
    launch, ready = pdist.GradReducer._launch, pdist.GradReducer.ready

    def recording_launch(self, lo, hi):
        if hi > lo:
            layers.join_side_stream()                         # as _launch does before it hands the range to the collective
            snaps.append((lo, hi, self.flat[lo:hi].clone()))  # the values the collective is handed, in stream order
        return launch(self, lo, hi)

    def recording_ready(self, offset):
        markers.append(int(offset))
        return ready(self, offset)
    pdist.GradReducer._launch, pdist.GradReducer.ready = recording_launch, recording_ready
    model, opt = build_model(seeded_segmentor_state(9))
    out = model.train_step(to_dev(sup_batch(), DEV), opt)
    torch.cuda.synchronize()
    arena = model.param_arena
    grad = arena.grad.clone().cpu()
    ok = all(bool(torch.equal(snap.cpu(), grad[lo:hi])) for lo, hi, snap in snaps)
    cover = sorted((lo, hi) for lo, hi, _ in snaps)
    contiguous = bool(cover) and cover[0][0] == 0 and cover[-1][1] == grad.numel() and all(a[1] == b[0] for a, b in zip(cover, cover[1:]))
    want = [arena.offsets[next(n for n in arena.names if not n.startswith('backbone.'))]] + \
        [arena.offsets[next(n for n in arena.names if n.startswith(f'backbone.layer{i}.'))] for i in (4, 3, 2, 1)]
    torch.save(dict(ok=ok, buckets=len(snaps), contiguous=contiguous, markers=markers, want_markers=want, log=out['log_vars'],
                    sizes=[hi - lo for lo, hi, _ in snaps], grad_norm=float(grad.norm())), os.path.join(outdir, 'rccl_supervised.pt'))
    dist.destroy_process_group()


def test_overlapped_reducer_behind_a_supervised_step(tmp_path):
    """The bucketed reducer all-reduces the finished TAIL of the gradient arena while the backward sweep keeps writing lower offsets: every
    bucket's content at launch must be bit-identical to the arena after the step (no writer after its range's marker), the buckets tile the
    arena exactly once, and the markers fire heads, layer4 .. layer1, in that order."""
    port = 29900 + (os.getpid() % 1000)
    mp.spawn(_rccl_supervised_worker, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    res = torch.load(tmp_path / 'rccl_supervised.pt', weights_only=False)
    print('overlapped buckets (elements):', res['sizes'], 'markers', res['markers'])
    assert res['markers'] == res['want_markers']
    assert res['buckets'] >= 3 and res['contiguous'], (res['buckets'], res['contiguous'])
    assert res['ok'], 'a gradient range was written after the marker that declared it final'
    assert res['grad_norm'] > 0 and list(res['log']) == ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg', 'loss']
