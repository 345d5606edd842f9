"""fp64 torch restatement of the adversarial (ADVENT) baseline, written from its formulas: the per-class entropy map, the five-layer
FCDiscriminator, the L1 losses of AdvLoss(loss_type='advent') and one alternating step of DomainAdaptorAdv.

  ent(z)_c = -p_c log2(p_c + 1e-30) / log2(C),  p = softmax_c(z)                    (a map with C channels, not summed over the classes)
  D(e)     = mean_px conv5(lrelu(conv4(lrelu(conv3(lrelu(conv2(lrelu(conv1(e)))))))))  every conv 4x4 / stride 2 / padding 1 with bias,
             lrelu = LeakyReLU(0.2); d has one value per image
  disc:  loss_disc_src = w_src mean_n |D(ent(z_src)) - 0|,  loss_disc_trg = w_trg mean_n |D(ent(z_trg)) - 1|   on detached logits
  gen:   loss_gen = w_gen mean_n |D(ent(z_trg)) - 0|        gradient to z_trg, none to D

Everything here runs on the CPU in float64; the kernels under test and the executed reference (tests/golden/advent.npz) are compared to it."""
import numpy as np
import torch
import torch.nn.functional as F

from entropy_oracle import per_link_excess  # noqa: F401  (the per-link bound, shared)

SLOPE = 0.2
KEYS = [f'net.{i}.{p}' for i in (0, 2, 4, 6, 8) for p in ('weight', 'bias')]


def t64(a):
    return a.detach().double().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).double()


def entropy_map(z):
    z = t64(z)
    p = torch.softmax(z, dim=1)
    return -(p * torch.log2(p + 1e-30)) / np.log2(z.shape[1])


def conv4s2(x, w, b=None, slope=None):
    y = F.conv2d(x, w, b, stride=2, padding=1)
    return y if slope is None else F.leaky_relu(y, slope)


def discriminator(params, e, keep=False):
    """params: the ten tensors in KEYS order -> d [N] (and the five layer outputs)"""
    acts, x = [], e
    for i in range(5):
        x = conv4s2(x, params[2 * i], params[2 * i + 1], SLOPE if i < 4 else None)
        acts.append(x)
    d = x.mean(dim=(1, 2, 3))
    return (d, acts) if keep else d


def l1(d, label, weight):
    return weight * (d - label).abs().mean()


def disc_losses(params, z_src, z_trg, weights):
    """-> (loss_disc_src, loss_disc_trg, d_src, d_trg) as fp64 tensors; params may require grad, the logits are detached"""
    d_src = discriminator(params, entropy_map(z_src).detach())
    d_trg = discriminator(params, entropy_map(z_trg).detach())
    return l1(d_src, 0.0, weights['loss_disc_src']), l1(d_trg, 1.0, weights['loss_disc_trg']), d_src, d_trg


def disc_grads(params, z_src, z_trg, weights):
    """the disc losses and the gradient of their sum with respect to the ten parameters"""
    ps = [t64(p).clone().requires_grad_(True) for p in params]
    ls, lt, d_src, d_trg = disc_losses(ps, z_src, z_trg, weights)
    grads = torch.autograd.grad(ls + lt, ps)
    return dict(loss_disc_src=float(ls.detach()), loss_disc_trg=float(lt.detach()), d_src=d_src.detach(), d_trg=d_trg.detach(), grads=[g.detach() for g in grads])


def gen_loss(params, z_trg, weights):
    """-> dict(loss_gen, d_trg, grad = d loss_gen / d z_trg); the parameters are constants"""
    z = t64(z_trg).clone().requires_grad_(True)
    d = discriminator([t64(p) for p in params], entropy_map_graph(z))
    loss = l1(d, 0.0, weights['loss_gen'])
    g, = torch.autograd.grad(loss, z)
    return dict(loss_gen=float(loss.detach()), d_trg=d.detach(), grad=g)


def entropy_map_graph(z):
    p = torch.softmax(z, dim=1)
    return -(p * torch.log2(p + 1e-30)) / np.log2(z.shape[1])


def adamw_step(params, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, step=1, m=None, v=None):
    """torch.optim.AdamW's update (amsgrad off) in fp64 -> (new params, m, v)"""
    out, ms, vs = [], [], []
    for i, (p, g) in enumerate(zip(params, grads)):
        p, g = t64(p), t64(g)
        mi = (torch.zeros_like(p) if m is None else m[i]) * betas[0] + (1 - betas[0]) * g
        vi = (torch.zeros_like(p) if v is None else v[i]) * betas[1] + (1 - betas[1]) * g * g
        p = p * (1 - lr * weight_decay)
        mhat, vhat = mi / (1 - betas[0] ** step), vi / (1 - betas[1] ** step)
        out.append(p - lr * mhat / (vhat.sqrt() + eps))
        ms.append(mi)
        vs.append(vi)
    return out, ms, vs


# ---- the cases of tests/golden/advent.npz (tests/golden/make_golden_advent.py)
GOLDEN_CASES = ('c6', 'c2', 'c19', 'min', 'wide')


def golden_case(golden, name):
    """-> dict(logits_src, logits_trg (fp32 tensors), params (the ten fp32 tensors in KEYS order), weights): the stored target logits, the
    source logits derived from them (images in reverse order, negated), the wide case derived from `min` (scaled by 40)"""
    scale = 40.0 if name == 'wide' else 1.0
    zt = torch.from_numpy(golden[('min' if name == 'wide' else name) + '|logits_trg']).float() * scale
    C = zt.shape[1]
    params = [torch.from_numpy(golden[f'param|c{C}|{k}' if k.startswith('net.0.') else f'param|{k}']) for k in KEYS]
    w = golden['weights']
    return dict(logits_src=-zt.flip(0), logits_trg=zt, params=params,
                weights=dict(loss_disc_src=float(w[0]), loss_disc_trg=float(w[1]), loss_gen=float(w[2])))
