"""DomainAdaptorAdv.train_step on the GPU: b = 2 x 160^2 (logits 40 x 40), six classes, dropout 0, the seeded segmentor state of the other step
tests, an FCDiscriminator(ndf = 4) with the scaled seeded parameters of tests/golden/advent.npz, AdamW on both sides.  All steps run in
deterministic mode from identical weights, so steps that launch the same kernels on the same values agree bit for bit.

What is compared with what:
  * the adversarial part -- loss_disc_src / loss_disc_trg / loss_gen, the discriminator's gradient arena and parameters after its step, and the
    gradient that the generator receives at the target pass's logits -- against the fp64 oracle (tests/advent_oracle.py) driven with the
    same discriminator weights and the step's own captured logits: losses within 1e-5 relative, everything else per element within
    |hip - ref| <= 1e-4 max|ref| + 1e-3 |ref|, the bound of one link;
  * the source pass's log values and the generator's parameter gradients at loss_gen = 0 against the supervised step of the same segmentor
    from the same state (tests/test_supervised_gpu.py holds THAT step against the whole-network oracle): the log values bit for bit, the
    gradients within the bound;
  * the generator's parameter gradients for loss_gen = W and 2 W: affine in the weight, within the bound -- the chain from the logits'
    gradient to the parameters is the existing backward sweep.
A whole-network fp64 comparison of the parameter gradients is not repeated here: through ~70 train-mode BatchNorm layers of a random-init
network an fp32 path is percents away from fp64 (tests/test_supervised_gpu.py), which no per-link bound can hold.

W_GEN is chosen as in tests/test_uda_baselines_gpu.py: the subject of the affinity test is a difference of arenas, which the bound resolves
only where the term's share is a tenth of the arena's largest element or more (asserted)."""
import os
import warnings
from collections import OrderedDict

import numpy as np
import pytest
import torch

import advent_oracle as orc
from advent_oracle import per_link_excess
from helpers import model_cfg, to_dev

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = 160
W_GEN = 1.0
WEIGHTS = dict(loss_disc_src=0.5, loss_disc_trg=0.7)
GEN_OPT = dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
DISC_OPT = dict(type='AdamW', lr=1e-2, betas=(0.9, 0.99), weight_decay=0.01)
SRC_KEYS = ['decode.loss_ce', 'decode.acc_seg', 'aux.loss_ce', 'aux.acc_seg']
ADV_KEYS = ['loss_disc_src', 'loss_disc_trg', 'loss_gen']


def seeded_segmentor_state(seed=9):
    from oracle import pfst_oracle as O
    from pfst_amd.synthetic import fill_state_dict
    return fill_state_dict(O.init_state_dict(6, 3), seed)


def disc_params(golden_dir):
    g = np.load(os.path.join(golden_dir, 'advent.npz'))
    return orc.golden_case(g, 'c6')['params']


def build(state, dparams, w_gen=W_GEN):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizers
    from pfst_amd.presets import advent_cfg
    from pfst_amd.registry import build_segmentor
    cfg = advent_cfg(model_cfg(dropout=0.0), ndf=4, weights=dict(WEIGHTS, loss_gen=w_gen))['model']
    model = build_segmentor(cfg)
    sd = OrderedDict((k, v.clone()) for k, v in state.items())
    sd.update(('discriminator.' + k, p.clone()) for k, p in zip(orc.KEYS, dparams))
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.cuda()
    return model, build_optimizers(model, dict(generator=dict(GEN_OPT), discriminator=dict(DISC_OPT)))


def batch(seed=1234):
    from pfst_amd.synthetic import synth_batch
    return synth_batch(2, S, 6, seed=seed)


def one_step(state, dparams, w_gen, b):
    """-> dict(out, gen arena grad, disc arena grad, disc params after, captured logits_src / logits_trg and the gradient at logits_trg,
    weight-gradient launches of the step)"""
    from pfst_amd import hip_ops
    model, opts = build(state, dparams, w_gen)
    seen = []
    head_forward = model.decode_head.forward

    def recording_forward(*a, **k):                                # the step calls the head's forward directly: no module hook fires
        res = head_forward(*a, **k)
        seen.append(res[0] if isinstance(res, tuple) else res)
        return res
    model.decode_head.forward = recording_forward
    g_logits = []
    map_bwd = hip_ops.entropy_map_bwd_

    def recording_map_bwd(dlogits, logits, grad_ent, accumulate=True, **k):
        assert not accumulate                                      # loss_gen is the only term on the target pass's logits: the first writer
        g_logits.append(map_bwd(dlogits, logits, grad_ent, accumulate=accumulate, **k).clone())
        return dlogits
    hip_ops.entropy_map_bwd_ = recording_map_bwd
    before = hip_ops.ADV_WGRAD_LAUNCHES
    try:
        out = model.train_step(to_dev(b, DEV), opts)
        torch.cuda.synchronize()
    finally:
        del model.decode_head.forward
        hip_ops.entropy_map_bwd_ = map_bwd
    assert len(seen) == 2 and len(g_logits) == 1                   # the source pass, then the target pass; one gradient into the logits
    return dict(out=out, gen_grad=model.param_arena.grad.clone(), disc_grad=model.disc_param_arena.grad.clone(),
                disc_after=[p.detach().clone().cpu() for p in model.discriminator.parameters()],
                logits_src=seen[0].data.clone().cpu(), logits_trg=seen[1].data.clone().cpu(), g_logits_trg=g_logits[0].cpu(),
                wgrads=hip_ops.ADV_WGRAD_LAUNCHES - before, model=model, opts=opts)


@pytest.fixture(scope='module')
def runs(golden_dir):
    from pfst_amd import hip_ops
    state, dparams, b = seeded_segmentor_state(), disc_params(golden_dir), batch()
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        r = dict(w1=one_step(state, dparams, W_GEN, b), w2=one_step(state, dparams, 2 * W_GEN, b), w0=one_step(state, dparams, 0.0, b))
        # the supervised step of the same segmentor from the same state on the source side of the batch
        from pfst_amd.optim import build_optimizer
        from pfst_amd.registry import build_segmentor
        sup = build_segmentor(model_cfg(dropout=0.0))
        sup.load_state_dict(state, strict=True)
        sup.cuda()
        out = sup.train_step(to_dev({k: v for k, v in b.items() if not k.startswith('target_')}, DEV), build_optimizer(sup, dict(GEN_OPT)))
        torch.cuda.synchronize()
        r['sup'] = dict(out=out, gen_grad=sup.param_arena.grad.clone(), model=sup)
    finally:
        hip_ops.set_deterministic(was)
    r.update(state=state, dparams=dparams, batch=b)
    return r


@pytest.fixture(scope='module')
def oracle(runs):
    """the adversarial part in fp64 on the captured logits of the W_GEN step: disc losses and gradients, the AdamW step of D, loss_gen with
    the parameters before and after that step"""
    r = runs['w1']
    w = dict(WEIGHTS, loss_gen=W_GEN)
    dg = orc.disc_grads(runs['dparams'], r['logits_src'], r['logits_trg'], w)
    new, _, _ = orc.adamw_step(runs['dparams'], dg['grads'], DISC_OPT['lr'], DISC_OPT['betas'], 1e-8, DISC_OPT['weight_decay'], step=1)
    return dict(disc=dg, new=new, gen_after=orc.gen_loss(new, r['logits_trg'], w), gen_before=orc.gen_loss(runs['dparams'], r['logits_trg'], w))


def test_log_values_and_discriminator_update_against_the_oracle(runs, oracle):
    r = runs['w1']
    lv = r['out']['log_vars']
    assert list(lv) == SRC_KEYS + ADV_KEYS
    assert r['out']['num_samples'] == 4 and r['out']['states'] == {}
    assert r['out']['loss'] == pytest.approx(lv['decode.loss_ce'] + lv['aux.loss_ce'] + lv['loss_gen'], rel=1e-12)
    assert tuple(r['logits_trg'].shape) == (2, 6, 40, 40)
    want = dict(loss_disc_src=oracle['disc']['loss_disc_src'], loss_disc_trg=oracle['disc']['loss_disc_trg'], loss_gen=oracle['gen_after']['loss_gen'])
    for k in ADV_KEYS:
        rel = abs(lv[k] - want[k]) / abs(want[k])
        print(f'{k}: {lv[k]:.8g}, fp64 oracle on the captured logits {want[k]:.8g}: rel {rel:.2e} (bound 1e-5)')
        assert rel <= 1e-5
    # the L1 gradient is a sign: every |d_n - label| must be far from 0 for the comparison to be one of values, not of rounding
    d = oracle['disc']
    assert float(d['d_src'].abs().min()) > 1e-3 and float((d['d_trg'] - 1).abs().min()) > 1e-3 and float(oracle['gen_after']['d_trg'].abs().min()) > 1e-3
    # (a) D's gradient arena and its parameters after the step; (b) they are the disc-only update: ten weight-gradient launches (5 layers x 2
    # domains) and none in the frozen generator pass, whose loss leaves nothing in D's arena
    model = r['model']
    arena = model.disc_param_arena
    for key, g64, p64, p in zip(orc.KEYS, d['grads'], oracle['new'], r['disc_after']):
        ex = per_link_excess(arena.view(r['disc_grad'], key).cpu().numpy(), g64.numpy())
        exp = per_link_excess(p.numpy(), p64.numpy())
        print(f'discriminator {key}: gradient excess over the per-link bound {ex:.2e}, parameter after the step {exp:.2e}')
        assert ex <= 0 and exp <= 0, key
    assert r['wgrads'] == 10


def test_generator_receives_the_gradient_of_the_updated_discriminator(runs, oracle):
    r = runs['w1']
    after, before = oracle['gen_after'], oracle['gen_before']
    ex = per_link_excess(r['g_logits_trg'].numpy(), after['grad'].numpy())
    print(f'd loss_gen / d logits_trg: max |ref| {float(after["grad"].abs().max()):.3e}, excess over the per-link bound {ex:.2e}')
    assert ex <= 0
    # (d) with the discriminator as it was BEFORE its step the oracle gives another loss and another gradient, more than 100 bounds away
    lv = r['out']['log_vars']
    gap = abs(after['loss_gen'] - before['loss_gen']) / abs(after['loss_gen'])
    print(f'loss_gen with the updated discriminator {after["loss_gen"]:.8g}, with the old one {before["loss_gen"]:.8g}: rel. gap {gap:.2e}')
    assert gap > 100 * 1e-5
    assert abs(lv['loss_gen'] - before['loss_gen']) > 50 * 1e-5 * abs(before['loss_gen'])
    assert per_link_excess(r['g_logits_trg'].numpy(), before['grad'].numpy()) > 0


def test_generator_gradient_is_affine_in_the_weight_and_supervised_at_zero(runs):
    a0, a1, a2 = (runs[k]['gen_grad'].double().cpu().numpy() for k in ('w0', 'w1', 'w2'))
    d1, d2 = a1 - a0, a2 - a0
    ex = per_link_excess(2 * d1, d2)
    print(f'arena(2W) - arena(0): max {np.abs(d2).max():.3e} beside max |arena(0)| {np.abs(a0).max():.3e}; against 2 (arena(W) - arena(0)): '
          f'max |diff| {np.abs(2 * d1 - d2).max():.2e}, excess over the per-link bound {ex:.2e}')
    assert np.abs(d2).max() > 0.1 * np.abs(a0).max(), 'the term\'s share is large enough for the bound to resolve the difference (module docstring)'
    assert ex <= 0
    assert runs['w2']['out']['log_vars']['loss_gen'] == pytest.approx(2 * runs['w1']['out']['log_vars']['loss_gen'], rel=1e-6)
    # the discriminator's side does not depend on the generator's weight
    assert torch.equal(runs['w0']['disc_grad'], runs['w1']['disc_grad']) and torch.equal(runs['w2']['disc_grad'], runs['w1']['disc_grad'])
    # at 0: the supervised source-pass gradient (the target pass back-propagates zeros), and the source pass's log values
    sup = runs['sup']
    ex0 = per_link_excess(a0, sup['gen_grad'].double().cpu().numpy())
    print(f'arena(0) against the supervised step: max |diff| {np.abs(a0 - sup["gen_grad"].double().cpu().numpy()).max():.2e}, excess {ex0:.2e}')
    assert ex0 <= 0
    assert runs['w0']['out']['log_vars']['loss_gen'] == 0.0
    for k in SRC_KEYS:
        assert runs['w1']['out']['log_vars'][k] == sup['out']['log_vars'][k], k


def test_every_batchnorm_sees_both_domains_the_auxiliary_heads_included(runs):
    """domain_adaptor_adv.py:264-284: backbone, decode head AND auxiliary head run on the source and on the target batch in training mode, so
    after one step every BatchNorm has tracked two batches (the supervised step: one), and the auxiliary head's running statistics differ
    from the source-only ones"""
    sd = runs['w1']['model'].state_dict()
    counts = {k: int(v) for k, v in sd.items() if k.endswith('num_batches_tracked')}
    assert any(k.startswith('auxiliary_head.') for k in counts) and any(k.startswith('decode_head.') for k in counts)
    assert {k for k, v in counts.items() if v != 2} == set()
    sup = runs['sup']['model'].state_dict()
    assert {int(v) for k, v in sup.items() if k.endswith('num_batches_tracked')} == {1}
    k = 'auxiliary_head.convs.0.bn.running_mean'
    assert not torch.equal(sd[k], sup[k]) and not torch.equal(sup[k].cpu(), runs['state'][k].cpu())


def two_steps(state, dparams, batches):
    model, opts = build(state, dparams)
    for b in batches:
        model.train_step(b, opts)
    torch.cuda.synchronize()
    return model, opts


def test_deterministic_two_step_runs_are_bit_identical(runs):
    from pfst_amd import hip_ops
    batches = [to_dev(batch(1234 + i), DEV) for i in range(2)]
    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        got = []
        for _ in range(2):
            model, _ = two_steps(runs['state'], runs['dparams'], batches)
            got.append([t.clone() for t in (model.param_arena.data, model.param_arena.grad, model.disc_param_arena.data, model.disc_param_arena.grad)])
    finally:
        hip_ops.set_deterministic(was)
    for a, b in zip(*got):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert float(got[0][3].abs().max()) > 0


def test_checkpoint_resume_and_evaluation(runs, tmp_path):
    """(f) a checkpoint, then runner.resume, continues bit for bit with both optimizers' states; (g) the checkpoint loads into a bare
    EncoderDecoder the way tools/test.py loads it -- the discriminator's keys unexpected and ignored, none missing -- and predicts what
    the adversarial model itself predicts"""
    from pfst_amd import hip_ops
    from pfst_amd.config import Config
    from pfst_amd.registry import build_segmentor
    from pfst_amd.runner import IterBasedRunner
    batches = [to_dev(batch(1234 + i), DEV) for i in range(2)]

    def make(work):
        cfg = Config(dict(runner=dict(type='IterBasedRunner', max_iters=100), lr_config=dict(policy='poly', power=1.0, min_lr=0.0, by_epoch=False),
                          log_config=dict(interval=1), checkpoint_config=dict(interval=1)))
        model, opts = build(runs['state'], runs['dparams'])
        return model, opts, IterBasedRunner(model, opts, cfg, str(work), log=lambda s: None)

    def snapshot(model, opts):
        return [t.clone().cpu() for t in (model.param_arena.data, model.disc_param_arena.data)] + \
               [st[k].clone().cpu() for o in opts.values() for st in o._flat.values() for k in ('m', 'v')]

    was = hip_ops.is_deterministic()
    hip_ops.set_deterministic(True)
    try:
        model, opts, runner = make(tmp_path / 'a')
        assert runner.base_lr == [GEN_OPT['lr'], DISC_OPT['lr']]
        runner.run(iter(batches), max_iters=2)
        torch.cuda.synchronize()
        assert [g['lr'] for g in opts.param_groups] == pytest.approx([GEN_OPT['lr'] * 0.99, DISC_OPT['lr'] * 0.99], rel=1e-12)    # the schedule reached both optimizers
        want = snapshot(model, opts)
        model, opts, runner = make(tmp_path / 'b')
        runner.run(iter(batches[:1]), max_iters=1)
        ck = tmp_path / 'b' / 'iter_1.pth'
        saved = torch.load(ck, map_location='cpu', weights_only=False)
        assert sorted(saved['optimizer']) == ['discriminator', 'generator']
        assert {k.split('.')[0] for k in saved['state_dict']} == {'backbone', 'decode_head', 'auxiliary_head', 'discriminator'}
        model, opts, runner = make(tmp_path / 'c')
        runner.resume(str(ck))
        assert runner.iter == 1
        runner.run(iter(batches[1:]), max_iters=2)
        torch.cuda.synchronize()
        got = snapshot(model, opts)
    finally:
        hip_ops.set_deterministic(was)
    assert len(got) == len(want) == 6
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f'tensor {i} differs after resume: {int((a != b).sum())} elements'
    # (g)
    plain = build_segmentor(model_cfg(dropout=0.0))
    res = plain.load_state_dict(saved['state_dict'], strict=False)
    assert not [k for k in res.missing_keys if not k.endswith('num_batches_tracked')]
    assert sorted(res.unexpected_keys) == sorted('discriminator.' + k for k in orc.KEYS)
    plain.cuda().eval()
    adv, _ = build(runs['state'], runs['dparams'])
    adv.load_state_dict(saved['state_dict'], strict=True)
    adv.cuda().eval()
    img = batches[0]['target_img']
    meta = [dict(ori_shape=(S, S, 3), img_shape=(S, S, 3), pad_shape=(S, S, 3), flip=False) for _ in range(2)]
    a, b = plain.simple_test(img, meta), adv.simple_test(img, meta)
    a, b = (a[0] if isinstance(a, tuple) else a), (b[0] if isinstance(b, tuple) else b)
    assert len(a) == 2 and all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0].shape == (S, S)


def test_one_blocking_host_read_per_step(runs, monkeypatch):
    """(h) after a warm-up step: one Event.synchronize and nothing else that makes the host wait (torch's sync debug mode reports every
    implicitly synchronizing call)"""
    model, opts = build(runs['state'], runs['dparams'])
    b = to_dev(batch(), DEV)
    model.train_step(b, opts)
    torch.cuda.synchronize()
    calls = []
    real = torch.cuda.Event.synchronize
    monkeypatch.setattr(torch.cuda.Event, 'synchronize', lambda self: (calls.append(1), real(self))[1])
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: calls.append('device'))
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            out = model.train_step(b, opts)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    sync_warnings = [str(w.message) for w in caught if 'synchroniz' in str(w.message).lower()]
    assert calls == [1], calls
    assert not sync_warnings, sync_warnings
    assert np.isfinite(out['loss'])
