"""PFGSTLoss at kernel_size 3 / 5 / 7 and top_k up to kernel_size^2 - 1 on the GPU: every entry of the C ABI that takes `ksize` against
plain torch (fp64), the two similarity-map implementations at K = 3 against each other, the top-k selection under exact ties against a
stable sort, the PFGSTLoss module against the executed reference's vectors (tests/golden/pfgst_kernel_size.npz), one whole train step
at kernel_size 5 against the oracle, and deterministic mode."""
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import assert_live_target_side, seeded_pfgst_state, to_dev
from test_pfgst_kernel_size_cpu import KERNEL_SIZE_VARIANTS, module_cfg

pytestmark = pytest.mark.gpu

DEV = 'cuda'
EPS = 1e-8
W4 = (0.1, 0.2, 0.3, 0.4)


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    from pfst_amd import hip_ops
    return hip_ops


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def assert_close(a, b, tol=1e-3, what=''):
    e = rel_err(a, b)
    assert e < tol, f'{what} rel err {e:.3e} >= {tol}'


def unfold(x, K, d):
    B, C, H, W = x.shape
    return F.unfold(x, K, dilation=d, padding=(K // 2) * d).view(B, C, K * K, H, W)


def t_sim(x, K, d, sim_type, sigma):
    """the similarity map in torch (nn.Unfold's zero padding; each norm clamped like the kernels)"""
    u = unfold(x, K, d)
    if sim_type == 'gaussian':
        return torch.exp(-((u - x.unsqueeze(2)) ** 2).sum(1) / sigma ** 2)
    return (u * x.unsqueeze(2)).sum(1) / (x.norm(dim=1, keepdim=True).clamp_min(EPS) * u.norm(dim=1).clamp_min(EPS))


def labels(n, H, W, seed):
    """full-resolution (2H x 2W) labels: classes 0..3 in 2 x 2 blocks (class 0 is also the padding band's label), a 255 corner"""
    gen = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, 4, (n, 1, H, W), generator=gen).repeat_interleave(2, 2).repeat_interleave(2, 3)
    gt[:, :, :5, :7] = 255
    mix = (torch.rand(n, 1, 2, 2, generator=gen) > 0.5).long()
    mix = F.interpolate(mix.float(), size=(2 * H, 2 * W), mode='nearest').long()
    mix[0] = 0                                             # image 0 un-mixed: valid pixels even at K = 7, d = 3
    return gt, mix


def t_valid(gt, mix, H, W, K, d):
    g = F.interpolate(gt.float(), size=(H, W), mode='nearest')
    region = F.interpolate((1 - mix).float(), size=(H, W), mode='nearest') > 0.5
    all_in = unfold(region.double(), K, d).sum(2) == K * K
    return all_in & (g != 255), all_in


# ----------------------------------------------------------------------------------------------------------------- K x K vs torch
KD = [(K, d) for K in (3, 5, 7) for d in (1, 2, 3)]


@pytest.mark.parametrize('sim_type', ['cosine', 'gaussian'])
@pytest.mark.parametrize('K,d', KD)
def test_sim_map_k_and_adjoint_against_torch(ops, K, d, sim_type):
    """the similarity map and its adjoint (accumulating and not): W not a multiple of 4, partial 16 x 16 tiles, C not a multiple
    of the LDS chunk, taps in the zero-padding band"""
    gen = torch.Generator().manual_seed(K * 10 + d)
    n, C, H, W = 2, 37, 21, 23
    x = torch.randn(n, C, H, W, generator=gen, dtype=torch.float64) * 0.5
    sigma = 4.0
    xr = x.clone().requires_grad_()
    ref = t_sim(xr, K, d, sim_type, sigma)
    sim, norm = torch.empty(n, K * K, H, W, device=DEV), torch.empty(n, H, W, device=DEV)
    st = ops.SIM_TYPES[sim_type]
    xf = x.float().to(DEV)
    ops.call('pfst_sim_map_k', xf.data_ptr(), n, C, H, W, K, d, st, sigma, sim.data_ptr(), norm.data_ptr(), 0)
    assert_close(sim, ref, 1e-5, 'sim')
    if sim_type == 'cosine':
        assert_close(norm, x.norm(dim=1), 1e-6, 'norm')
    gs = torch.randn(n, K * K, H, W, generator=gen, dtype=torch.float64)
    ref.backward(gs)
    base = torch.randn(n, C, H, W, generator=gen)
    for accumulate in (0, 1):
        out = base.clone().to(DEV)
        coef = torch.empty(n * (K * K + 1) * H * W, device=DEV)
        ops.call('pfst_sim_map_bwd_k', xf.data_ptr(), sim.data_ptr(), norm.data_ptr(), gs.float().to(DEV).data_ptr(), n, C, H, W, K, d, st,
                 sigma, out.data_ptr(), accumulate, coef.data_ptr(), 0)
        want = xr.grad + (base.double() if accumulate else 0)
        assert_close(out, want, 1e-5, f'adjoint (accumulate={accumulate})')
    # the wrapper dispatches on ksize and returns the same map
    s2, _ = ops.sim_map(xf, d, sim_type, sigma, ksize=K)
    assert torch.equal(s2, sim) if K != 3 else rel_err(s2, sim) < 1e-5


@pytest.mark.parametrize('K,d', KD)
def test_source_target_and_cross_prob_k_against_torch(ops, K, d):
    """source statistics / gradients (mean_std, margin2, src_perc), target validity, the top-k losses (overlapping sets at
    top_k > (K^2-1)/2) and the cross-probability gradient into the logits"""
    gen = torch.Generator().manual_seed(100 + K * 10 + d)
    n, Cc, H, W = 2, 6, 22, 26
    gt, mix = labels(n, H, W, 7 * K + d)
    gt8, mm8 = ops.to_u8(gt.to(DEV)), ops.to_u8(mix.to(DEV))
    N = n * K * K * H * W                                  # distinct values (also in fp32): the sorted src_perc prefix is unique
    sim = (torch.randperm(N, generator=gen).double() / N * 2 - 1).view(n, K * K, H, W)
    g = F.interpolate(gt.float(), size=(H, W), mode='nearest')
    nb = unfold(g.double(), K, d).squeeze(1)
    ctr = g.expand(n, K * K, H, W)
    vs = (g != 255).expand(n, K * K, H, W)
    # --- source, mean_std and margin2 (all pairs)
    for lt_name in ('mean_std', 'margin2'):
        s = sim.clone().requires_grad_()
        pos, neg = s[(nb == ctr) & vs], s[(nb != ctr) & vs]
        if lt_name == 'mean_std':
            want = torch.stack([-pos.mean() * W4[0], neg.mean() * W4[1], pos.std() * W4[2], neg.std() * W4[3]])
        else:
            want = torch.stack([(F.relu(0.7 - pos) ** 2).mean() * W4[0], (F.relu(neg - 0.2) ** 2).mean() * W4[1]])
        want.sum().backward()
        losses, gsim = ops.src_sim_losses(sim.float().to(DEV), gt8, d, *W4, loss_type=lt_name, margin=(0.7, 0.2), ksize=K)
        assert_close(losses[:want.numel()], want, 1e-5, f'source losses {lt_name}')
        assert_close(gsim, s.grad, 1e-5, f'source gradient {lt_name}')
    # --- source, src_perc (tie-free values: the sorted prefix is unique)
    s = sim.clone().requires_grad_()
    pos, neg = s[(nb == ctr) & vs], s[(nb != ctr) & vs]
    pos, neg = pos.sort()[0][:int(pos.numel() * 0.4)], neg.sort(descending=True)[0][:int(neg.numel() * 0.4)]
    want = torch.stack([-pos.mean() * W4[0], neg.mean() * W4[1], pos.std() * W4[2], neg.std() * W4[3]])
    want.sum().backward()
    losses, gsim = ops.src_sim_losses(sim.float().to(DEV), gt8, d, *W4, src_perc=0.4, ksize=K)
    assert_close(losses, want, 1e-5, 'source losses src_perc')
    assert_close(gsim, s.grad, 1e-5, 'source gradient src_perc')
    # --- target validity
    valid_ref, all_ref = t_valid(gt, mix, H, W, K, d)
    valid, all_in, cnt = ops.trg_valid_mask(gt8, mm8, (H, W), d, ksize=K)
    assert torch.equal(valid.cpu().bool(), valid_ref) and torch.equal(all_in.cpu().bool(), all_ref)
    assert int(cnt) == int(valid_ref.sum())
    assert int(cnt) > 1, 'the test input must have valid target pixels'
    # --- top-k losses: disjoint sets, overlapping sets, all pairs
    logits = torch.randn(n, Cc, 2 * H, 2 * W, generator=gen, dtype=torch.float64) * 2
    prob = torch.softmax(logits[:, :, ::2, ::2], 1)
    ema = torch.rand(n, K * K, H, W, generator=gen, dtype=torch.float64) * 2 - 1
    kk = K * K
    for top_k in sorted({1, (kk - 1) // 2, (kk - 1) // 2 + 1, kk - 1, None} - {0}, key=lambda t: -1 if t is None else t):
        cp = (prob.unsqueeze(2) * unfold(prob, K, d)).sum(1).requires_grad_()
        es = ema.clone().requires_grad_()
        if top_k is None:
            lp, ln = es * -cp, (1 - es) * -(1 - cp)
        else:
            imax, imin = torch.topk(es, top_k + 1, dim=1)[1], torch.topk(es, top_k, dim=1, largest=False)[1]
            lp = torch.gather(es, 1, imax) * -torch.gather(cp, 1, imax)
            ln = (1 - torch.gather(es, 1, imin)) * -torch.gather(1 - cp, 1, imin)
        m = valid_ref
        want = torch.stack([lp[m.expand_as(lp)].mean() * 0.3, ln[m.expand_as(ln)].mean() * 0.7])
        want.sum().backward()
        out, gP, gS = ops.sim_topk_loss(ema.float().to(DEV), prob.float().to(DEV), valid, cnt, d, top_k, 0.3, 0.7, want_sim_grad=True,
                                        ksize=K)
        assert_close(out, want, 1e-5, f'top-k losses top_k={top_k}')
        assert_close(gP, cp.grad, 1e-5, f'd/d cross_prob top_k={top_k}')
        assert_close(gS, es.grad, 1e-5, f'd/d ema_sim top_k={top_k}')
    # --- cross-probability gradient into the logits (ds = 2), both detach_unfold settings
    gPr = torch.randn(n, kk, H, W, generator=gen, dtype=torch.float64) * valid_ref
    for unfold_grad in (False, True):
        lg = logits.clone().requires_grad_()
        pr = torch.softmax(lg[:, :, ::2, ::2], 1)
        q = unfold(pr, K, d)
        cp = (pr.unsqueeze(2) * (q if unfold_grad else q.detach())).sum(1)
        (cp * gPr).sum().backward()
        dl = torch.zeros(n, Cc, 2 * H, 2 * W, device=DEV)
        ops.cross_prob_bwd_(dl, prob.float().to(DEV), gPr.float().to(DEV), d, 2, unfold_grad, ksize=K)
        assert_close(dl, lg.grad, 1e-5, f'd logits (unfold_grad={unfold_grad})')


def test_out_of_range_arguments_are_refused(ops):
    from pfst_amd._lib import PfstHipError
    x = torch.randn(1, 8, 16, 16, device=DEV)
    for K, d in ((4, 1), (9, 1), (7, 13)):            # even / too large kernels; a halo tile beyond the LDS budget (r * d > 37)
        sim, norm = torch.empty(1, K * K, 16, 16, device=DEV), torch.empty(1, 16, 16, device=DEV)
        with pytest.raises(PfstHipError):
            ops.call('pfst_sim_map_k', x.data_ptr(), 1, 8, 16, 16, K, d, 0, 1.0, sim.data_ptr(), norm.data_ptr(), 0)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = torch.empty(2, device=DEV)
    with pytest.raises(PfstHipError):
        ops.call('pfst_sim_loss_finalize', acc.data_ptr(), cnt.data_ptr(), 5, 25, 0.1, 0.1, out.data_ptr(), 0)
    prob = torch.softmax(torch.randn(1, 6, 16, 16, device=DEV), 1)
    valid = torch.zeros(1, 1, 16, 16, dtype=torch.uint8, device=DEV)
    for K, top_k in ((4, 1), (3, 9)):                 # an even kernel; top_k beyond K^2 - 1
        ema, gP = torch.zeros(1, K * K, 16, 16, device=DEV), torch.empty(1, K * K, 16, 16, device=DEV)
        with pytest.raises(PfstHipError):
            ops.call('pfst_sim_topk_loss', ema.data_ptr(), prob.data_ptr(), valid.data_ptr(), cnt.data_ptr(), 1, 6, 16, 16, K, 1, top_k,
                     0.1, 0.1, gP.data_ptr(), acc.data_ptr(), 0, 0)


# ------------------------------------------------------------------------------------- the two similarity maps at K = 3 against each other
@pytest.mark.parametrize('d', [1, 2, 3])
@pytest.mark.parametrize('sim_type', ['cosine', 'gaussian'])
def test_k3_entries_match_the_3x3_entries(ops, d, sim_type):
    """pfst_sim_map / _bwd (3x3 strip and generic kernels) against pfst_sim_map_k / _bwd_k (halo tiles) at K = 3, the one job of the
    loss with two implementations: same inputs, exact ties included (duplicated feature columns give similarities equal to the
    centre tap's), floats within 1e-6 of each other"""
    gen = torch.Generator().manual_seed(40 + d)
    n, C, H, W = 2, 64, 32, 64                             # W = 64: the 3x3 cosine entry takes its strip kernel at d = 1, 2
    x = torch.randn(n, C, H, W, generator=gen)
    x[:, :, :, 6] = x[:, :, :, 5]
    x[:, :, 9, :] = x[:, :, 8, :]
    xf = x.to(DEV)
    sigma = 6.0
    s3, n3 = ops.sim_map(xf, d, sim_type, sigma)
    sk, nk = torch.empty_like(s3), torch.empty_like(n3)
    ops.call('pfst_sim_map_k', xf.data_ptr(), n, C, H, W, 3, d, ops.SIM_TYPES[sim_type], sigma, sk.data_ptr(), nk.data_ptr(), 0)
    assert rel_err(sk, s3) < 1e-6 and rel_err(nk, n3) < 1e-6
    gs = torch.randn(n, 9, H, W, generator=gen).to(DEV)
    b3 = ops.sim_map_bwd(xf, s3, n3, gs, d, sim_type=sim_type, sigma=sigma)
    bk = torch.empty_like(xf)
    coef = torch.empty(n * 10 * H * W, device=DEV)
    ops.call('pfst_sim_map_bwd_k', xf.data_ptr(), s3.data_ptr(), n3.data_ptr(), gs.data_ptr(), n, C, H, W, 3, d, ops.SIM_TYPES[sim_type], sigma,
             bk.data_ptr(), 0, coef.data_ptr(), 0)
    assert rel_err(bk, b3) < 1e-6


# ------------------------------------------------------------------------------------------------- top-k selection under exact ties
@pytest.mark.parametrize('K', [3, 5])
def test_topk_selection_under_exact_ties_against_torch(ops, K):
    """similarities on a grid of 21 values, so that most pixels hold equal taps: the selected sets must be those of a STABLE descending
    sort (the lower tap index first on ties), for disjoint and overlapping top / bottom sets and for all pairs.  gP and g_sim within
    1e-6 of the oracle's values (the same fp32 expressions), the losses within 1e-5, and for disjoint sets the zero pattern of g_sim
    equal to the oracle's selection"""
    gen = torch.Generator().manual_seed(60 + K)
    n, Cc, H, W, d, kk = 2, 6, 22, 26, 2, K * K
    ema = ((torch.rand(n, kk, H, W, generator=gen) * 2 - 1) * 10).round() / 10
    ties = int((ema.unsqueeze(1) == ema.unsqueeze(2)).sum()) - ema.numel()
    assert ties > 0, 'the input must hold exact ties'
    gt, mix = labels(n, H, W, 11 + K)
    gt8, mm8 = ops.to_u8(gt.to(DEV)), ops.to_u8(mix.to(DEV))
    valid, _, cnt = ops.trg_valid_mask(gt8, mm8, (H, W), d, ksize=K)
    count = int(cnt)
    assert count > 1, 'the test input must have valid target pixels'
    vm = valid.cpu().bool()                                                   # [n, 1, H, W]
    prob = torch.softmax(torch.randn(n, Cc, H, W, generator=gen), 1)          # fp32, the kernel's input
    P = (prob.double().unsqueeze(2) * unfold(prob.double(), K, d)).sum(1)     # cross-probabilities [n, kk, H, W]
    Pv = P.float()[vm.expand_as(P)]
    assert bool((Pv > 0).all()) and bool((1 - Pv > 0).all()), 'prob must be a strict softmax: neither P nor 1 - P is 0'
    # rank of every tap in a stable descending sort == #{i : s_i > s_j or (s_i == s_j and i < j)}
    order = torch.sort(ema, dim=1, descending=True, stable=True)[1]
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(kk).view(1, kk, 1, 1).expand_as(order))
    si, sj = ema.unsqueeze(2), ema.unsqueeze(1)                               # [n, i, 1, ..], [n, 1, j, ..]
    lower = torch.arange(kk).view(kk, 1) < torch.arange(kk).view(1, kk)       # i < j
    assert torch.equal(rank, ((si > sj) | ((si == sj) & lower.view(1, kk, kk, 1, 1))).sum(1))
    s = ema.double()
    w_pos, w_neg = 0.3, 0.7
    half = (kk - 1) // 2
    for top_k in (None, 1, half, half + 1, kk - 1):
        if top_k is None:
            pos, neg, npos, nneg = torch.ones_like(rank, dtype=torch.bool), torch.ones_like(rank, dtype=torch.bool), kk, kk
        else:
            pos, neg, npos, nneg = rank <= top_k, rank >= kk - top_k, top_k + 1, top_k
        pos, neg = pos & vm, neg & vm
        cpos, cneg = w_pos / (count * npos), w_neg / (count * nneg)
        want = torch.stack([(-s * P)[pos].sum() * cpos, (-(1 - s) * (1 - P))[neg].sum() * cneg])
        want_gP = torch.where(pos, -s * cpos, 0.0) + torch.where(neg, (1 - s) * cneg, 0.0)
        want_gS = torch.where(pos, -P * cpos, 0.0) + torch.where(neg, (1 - P) * cneg, 0.0)
        out, gP, gS = ops.sim_topk_loss(ema.to(DEV), prob.to(DEV), valid, cnt, d, top_k, w_pos, w_neg, want_sim_grad=True, ksize=K)
        e = dict(gP=rel_err(gP, want_gP), g_sim=rel_err(gS, want_gS), losses=rel_err(out, want))
        print(f'K={K} top_k={top_k}: ' + ' '.join(f'{k} {v:.3e}' for k, v in e.items()))
        assert e['gP'] < 1e-6 and e['g_sim'] < 1e-6, (top_k, e)
        assert e['losses'] < 1e-5, (top_k, e)
        if top_k is not None and top_k <= half:             # disjoint sets: a tap is in at most one, and its g_sim term is not 0
            assert torch.equal(gS.cpu() != 0, pos | neg), top_k


# --------------------------------------------------------------------------------------------------------- PFGSTLoss vs the reference
@pytest.mark.parametrize('name', list(KERNEL_SIZE_VARIANTS))
def test_pfgst_loss_kernel_size_variants_against_golden(ops, golden_dir, name):
    """the PFGSTLoss module at kernel_size 3 / 5 / 7 and large top_k: loss values, both input gradients, the density map and the
    projection's gradients against vectors from the executed reference (bounds of tests/test_hip_ops.py's option variants)"""
    from pfst_amd.engine import Tape, Var
    from pfst_amd.uda import PFGSTLoss
    z = np.load(os.path.join(golden_dir, 'pfgst_kernel_size.npz'))
    loss = PFGSTLoss(**module_cfg(name)).to(DEV)
    if loss.proj_net is not None:
        with torch.no_grad():
            loss.proj_net.weight.copy_(torch.from_numpy(z[name + '|proj_weight']))
            loss.proj_net.bias.copy_(torch.from_numpy(z[name + '|proj_bias']))
    lt = Var(torch.from_numpy(z['logits_trg']).to(DEV), True)
    xs = Var(torch.from_numpy(z['x_src']).to(DEV), True)
    xe = Var(torch.from_numpy(z['x_ema']).to(DEV), False)
    tape = Tape()
    out = loss(dict(logits_trg=lt, x_ema=xe, x_src=xs, gt_src=ops.to_u8(torch.from_numpy(z['gt_src']).to(DEV)),
                    mix_masks=ops.to_u8(torch.from_numpy(z['mix_masks']).to(DEV)), want_vis=True), tape)
    names = [k for k in out if not k.startswith('vis|')]
    assert names == list(z[name + '|names'])
    got = np.array([float(out[k].sum()) for k in names])
    assert np.allclose(got, z[name + '|losses'], rtol=1e-4, atol=1e-7), (got, z[name + '|losses'])
    tape.backward()
    assert_close(lt.grad, torch.from_numpy(z[name + '|grad_logits']), 1e-3, 'd logits_trg')
    assert_close(xs.grad, torch.from_numpy(z[name + '|grad_xsrc']), 1e-3, 'd x_src')
    assert_close(out['vis|density_sim_feat'][1], torch.from_numpy(z[name + '|density']), 1e-4, 'density')
    if loss.proj_net is not None:
        assert_close(loss.proj_net.weight.grad, torch.from_numpy(z[name + '|grad_proj_weight']), 1e-3, 'd proj_net.weight')
        assert_close(loss.proj_net.bias.grad, torch.from_numpy(z[name + '|grad_proj_bias']), 1e-3, 'd proj_net.bias')


# ----------------------------------------------------------------------------------------------------------------- whole train steps
K5_OPTS = dict(kernel_size=5, dilation=1, top_k=16)


def _k5_model(O, det=False):
    import pfst_amd  # noqa: F401
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import uda_cfg as preset_cfg
    from pfst_amd.registry import UDA
    cfg = preset_cfg(6, 3, dropout=0.0, blur=False, color_jitter_probability=2.0, pseudo_threshold=0.3)
    cfg['aux_losses'][0].update(K5_OPTS)
    model = UDA.build(cfg)
    both, student, teacher = seeded_pfgst_state(O, 9)
    model.load_state_dict(both, strict=False)
    model.cuda()
    opt = build_optimizer(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    return model, opt, student, teacher


def test_train_step_with_kernel_size_5_matches_oracle():
    """one whole PFGST.train_step with PFGSTLoss(kernel_size=5, top_k=16: overlapping top / bottom sets) against the oracle, with the
    bounds of test_step_with_pfgst_loss_option_variants"""
    from oracle import pfst_oracle as O
    from pfst_amd.synthetic import synth_batch
    model, opt, student, teacher = _k5_model(O)
    batch = synth_batch(2, 128, 6, seed=77)
    oracle = O.OraclePFGST(student, pseudo_threshold=0.3, teacher_sd=teacher,
                           loss_opts=dict(k=K5_OPTS['kernel_size'], dil=K5_OPTS['dilation'], top_k=K5_OPTS['top_k']))
    random.seed(3); np.random.seed(3)
    olog, ex = oracle.train_step(batch, return_extras=True)
    random.seed(3); np.random.seed(3)
    out = model.train_step(to_dev(batch, 'cuda'), opt)
    assert set(olog) == set(out['log_vars'])
    for k, v in olog.items():
        tol = 100.0 * 40 / (2 * 128 * 128) if k.endswith('acc_seg') else 5e-3 * max(abs(v), 1e-2)
        assert abs(out['log_vars'][k] - v) <= tol, (k, out['log_vars'][k], v)
    assert_live_target_side(olog, ex)


def test_kernel_size_5_steps_are_bit_identical_in_deterministic_mode():
    from oracle import pfst_oracle as O
    from pfst_amd import hip_ops
    from pfst_amd.synthetic import synth_batch

    def two_steps():
        model, opt, _, _ = _k5_model(O)
        batch = to_dev(synth_batch(2, 128, 6, seed=77), 'cuda')
        random.seed(5); np.random.seed(5); torch.manual_seed(5)
        logs = [model.train_step(batch, opt)['log_vars'] for _ in range(2)]
        torch.cuda.synchronize()
        return logs, model.student_arena.grad.clone().cpu(), model.student_arena.data.clone().cpu()

    hip_ops.set_deterministic(True)
    try:
        a, b = two_steps(), two_steps()
    finally:
        hip_ops.set_deterministic(False)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), 'gradients / weights after two steps differ between two runs'
    for la, lb in zip(a[0], b[0]):
        for k in la:
            assert abs(la[k] - lb[k]) <= 1e-12 * max(1.0, abs(la[k])), k       # fp64 atomics of the log sums (as test_deterministic_gpu)
