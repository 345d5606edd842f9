#!/usr/bin/env python3
"""Golden vectors for the adversarial (ADVENT) baseline, produced by EXECUTING the reference's losses/adv_loss.py (AdvLoss,
loss_type='advent', net_type 'disc' and 'gen') and discriminators/fc_discriminator.py (FCDiscriminator) on the CPU in fp32 through
make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns are stored).

AdvLoss.l1_loss moves its label tensor with `.to(y_pred.get_device())`, which is -1 for a CPU tensor and raises: torch.Tensor.get_device is
patched to return 'cpu' around the reference calls and restored afterwards.  Nothing else of the reference is altered.

Cases (ndf = 4 everywhere: channels C -> 4 -> 8 -> 16 -> 32 -> 1):
  c6, c2, c19   logits 2 x C x 37 x 45: ragged, 37 -> 18 -> 9 -> 4 -> 2 -> 1 rows
  min           1 x 6 x 32 x 32: the smallest input that leaves 1 x 1 out of all five layers
  wide          the `min` logits scaled by 40: probabilities underflow to exactly 0 in fp32
The target logits are seeded N(0, 1) draws rounded to multiples of 1/4 and stored as float16 (exact); the source logits are the target
logits with the images in reverse order, negated, and the wide case is `min` scaled by 40: both are derived by the tests as well, not stored.  The discriminator's parameters are seeded draws scaled so that its outputs are of order 1 (with the default initialisation d is
about 1e-2 and the gradient to the logits about 1e-8, which would test nothing).

Stored per case: `<case>|logits_trg` (float16; not for wide), 
`<case>|d_src`, `<case>|d_trg` (fp32, D before any update), `<case>|loss_disc_src`, `<case>|loss_disc_trg`, `<case>|loss_gen` (float64 of
the fp32 scalars), `<case>|grad_trg` (d loss_gen / d logits_trg, fp32), `<case>|dgrad|<key>` (d (loss_disc_src + loss_disc_trg) / d parameter);
once: `param|<key>` (layers 2 .. 5, shared by all cases), `param|c<C>|net.0.{weight,bias}` (the first layer per class count), `keys` (the
discriminator's state-dict keys), `weights` (loss_disc_src, loss_disc_trg, loss_gen).

Condition asserted here: the L1 gradient is a sign, so every |d_n - label| must exceed 100 x the fp32-vs-fp64 difference of that d_n (the
discriminator is run in fp64 as well to measure it); seeds and scale are chosen so that the reference alone meets it.

Usage:  python tests/golden/make_golden_advent.py        (writes tests/golden/advent.npz)
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402

# name: (C, N, (h, w), seed, scale)
SHAPES = {'c6': (6, 2, (37, 45), 0, 1.0), 'c2': (2, 2, (37, 45), 1, 1.0), 'c19': (19, 2, (37, 45), 2, 1.0), 'min': (6, 1, (32, 32), 3, 1.0),
          'wide': (6, 1, (32, 32), 3, 40.0)}
WEIGHTS = dict(loss_disc_src=0.5, loss_disc_trg=0.7, loss_gen=0.3)
NDF = 4
GAIN = 2.5


def seeded_logits(name):
    C, N, hw, seed, scale = SHAPES[name]
    g = torch.Generator().manual_seed(9400 + seed)
    z = torch.randn(N, C, *hw, generator=g)
    z = (z * 4).round() / 4                         # multiples of 1/4 within (-8, 8): exact in float16, and the archive stays small
    assert torch.equal(z.half().float(), z)
    return source_of(z) * scale, z * scale


def source_of(logits_trg):
    """the source logits of a case are derived from its target logits (images in reverse order, negated), so that only one of the two is
    stored; the tests derive them the same way (tests/advent_oracle.py)"""
    return -logits_trg.flip(0)


def seeded_params(disc, C):
    """layers 2 .. 5 are the same draws in every case (stored once); the first layer, whose width is C, is drawn per class count"""
    g = torch.Generator().manual_seed(9500)
    g0 = torch.Generator().manual_seed(9500 + C)
    with torch.no_grad():
        for name, p in disc.named_parameters():
            gen = g0 if name.startswith('net.0.') else g
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=gen) * GAIN / (p.shape[1] * 16) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)


def gen_advent(ref):
    pkg = types.ModuleType('rsiseg.models.discriminators')
    pkg.__path__ = []
    sys.modules['rsiseg.models.discriminators'] = pkg
    _load('rsiseg.models.discriminators.fc_discriminator', 'rsiseg/models/discriminators/fc_discriminator.py')
    _load('rsiseg.models.losses.adv_loss', 'rsiseg/models/losses/adv_loss.py')
    out = dict(cases=np.array(list(SHAPES)), weights=np.array([WEIGHTS['loss_disc_src'], WEIGHTS['loss_disc_trg'], WEIGHTS['loss_gen']]))
    get_device = torch.Tensor.get_device
    torch.Tensor.get_device = lambda self: 'cpu'
    try:
        for name, (C, N, hw, seed, scale) in SHAPES.items():
            zs, zt = seeded_logits(name)
            if name != 'wide':
                out[name + '|logits_trg'] = zt.half().numpy()
            D = ref.builder.build_discriminator(dict(type='FCDiscriminator', num_in_channels=C, ndf=NDF))
            seeded_params(D, C)
            out['keys'] = np.array(list(D.state_dict().keys()))
            for k, v in D.state_dict().items():
                out[f'param|c{C}|{k}' if k.startswith('net.0.') else f'param|{k}'] = v.numpy().copy()
            disc = ref.builder.build_loss(dict(type='AdvLoss', loss_type='advent', net_type='disc', weights=dict(WEIGHTS)))
            gen = ref.builder.build_loss(dict(type='AdvLoss', loss_type='advent', net_type='gen', weights=dict(WEIGHTS)))
            # the discriminator's outputs, in fp32 (as the losses see them) and in fp64 (the condition above)
            D64 = ref.builder.build_discriminator(dict(type='FCDiscriminator', num_in_channels=C, ndf=NDF)).double()
            D64.load_state_dict({k: v.double() for k, v in D.state_dict().items()})
            for side, z, label in (('src', zs, 0.0), ('trg', zt, 1.0), ('trg', zt, 0.0)):
                with torch.no_grad():
                    e = disc.prob2ent(torch.softmax(z, dim=1))
                    d32 = D(e).flatten()
                    d64 = D64(e.double()).flatten()
                margin = (d32.double() - label).abs()
                err = (d32.double() - d64).abs()
                assert bool((margin > 100 * err).all()), (name, side, label, margin.tolist(), err.tolist())
                out[f'{name}|d_{side}'] = d32.numpy().copy()
                print(name, side, 'label', label, 'd', d32.tolist(), 'fp32-vs-fp64', err.tolist())
            res = disc(D, dict(logits_src=zs.clone(), logits_trg=zt.clone()))
            assert list(res) == ['loss_disc_src', 'loss_disc_trg'], list(res)
            D.zero_grad()
            (res['loss_disc_src'] + res['loss_disc_trg']).backward()
            for k, p in D.named_parameters():
                out[f'{name}|dgrad|{k}'] = p.grad.numpy().copy()
            out[f'{name}|loss_disc_src'] = np.array(float(res['loss_disc_src'].detach()), dtype=np.float64)
            out[f'{name}|loss_disc_trg'] = np.array(float(res['loss_disc_trg'].detach()), dtype=np.float64)
            for p in D.parameters():
                p.requires_grad_(False)
            z = zt.clone().requires_grad_()
            resg = gen(D, dict(logits_trg=z))
            assert list(resg) == ['loss_gen'], list(resg)
            resg['loss_gen'].backward()
            assert bool(torch.isfinite(z.grad).all()), name
            out[f'{name}|loss_gen'] = np.array(float(resg['loss_gen'].detach()), dtype=np.float64)
            out[f'{name}|grad_trg'] = z.grad.numpy().copy()
            print(name, {k: float(v.detach()) for k, v in list(res.items()) + list(resg.items())}, 'max |grad_trg|', float(z.grad.abs().max()),
                  'zeros', int((z.grad == 0).sum()))
    finally:
        torch.Tensor.get_device = get_device
    p = torch.softmax(seeded_logits('wide')[1], dim=1)
    assert int((p == 0).sum()) > 0, 'the wide case must have probabilities that are exactly 0'
    path = os.path.join(OUT, 'advent.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, 'bytes')
    assert size <= os.path.getsize(os.path.join(OUT, 'entropy_loss.npz')), 'larger than the largest golden committed so far'


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_advent(load_reference())
