#!/usr/bin/env python3
"""Golden vectors for EntropyLoss (MinEnt and max-squares), produced by EXECUTING the reference's losses/entropy_loss.py on CPU in fp32
through make_golden.py's loader (same rules: only seeded inputs and the numbers the reference returns are stored).

Cases, each with loss_type 'entropy' (weights {'loss_ent': 0.7}) and 'max_square' (weights {'loss_max_square': 1.3}); N = 2:
  c6    C =  6, 19 x 17, N(0, 1) logits
  c2    C =  2,  5 x  7: the normaliser is log2(2) = 1
  c11   C = 11,  7 x  9: the generic (class-loop) form
  c19   C = 19, 37 x 41 = 1517 pixels per image: several workgroups with a ragged last one
  wide  the c6 logits scaled by 40: probabilities underflow to exactly 0 in fp32, and the + 1e-30 is what keeps the reference finite
        (asserted here for its loss and its gradient)
Stored per case: `<case>|logits`, and per type `<case>|<type>|loss` (float64 of the fp32 scalar), `<case>|<type>|grad` (autograd's d loss /
d logits, fp32).

Usage:  python tests/golden/make_golden_entropy.py        (writes tests/golden/entropy_loss.npz)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402

# name: (C, (h, w), seed, scale)
SHAPES = {'c6': (6, (19, 17), 0, 1.0), 'c2': (2, (5, 7), 1, 1.0), 'c11': (11, (7, 9), 2, 1.0), 'c19': (19, (37, 41), 3, 1.0),
          'wide': (6, (19, 17), 0, 40.0)}
TYPES = {'entropy': {'loss_ent': 0.7}, 'max_square': {'loss_max_square': 1.3}}


def seeded_logits(name):
    C, hw, seed, scale = SHAPES[name]
    g = torch.Generator().manual_seed(9300 + seed)
    return torch.randn(2, C, *hw, generator=g) * scale


def gen_entropy(ref):
    _load('rsiseg.models.losses.entropy_loss', 'rsiseg/models/losses/entropy_loss.py')
    out = dict(cases=np.array(list(SHAPES)), types=np.array(list(TYPES)))
    for t, w in TYPES.items():
        out[t + '|weights'] = np.array([list(w.values())[0]], dtype=np.float64)
    for name in SHAPES:
        logits = seeded_logits(name)
        out[name + '|logits'] = logits.numpy()
        for t, w in TYPES.items():
            L = ref.builder.build_loss(dict(type='EntropyLoss', loss_type=t, weights=dict(w)))
            z = logits.clone().requires_grad_()
            res = L(dict(logits_trg=z))
            assert list(res) == [list(w)[0]], list(res)
            loss = res[list(w)[0]]
            assert loss.dim() == 0 and loss.dtype == torch.float32
            loss.backward()
            assert bool(torch.isfinite(loss)) and bool(torch.isfinite(z.grad).all()), (name, t)
            out[f'{name}|{t}|loss'] = np.array(float(loss.detach()), dtype=np.float64)
            out[f'{name}|{t}|grad'] = z.grad.numpy().copy()
            print(name, t, float(loss.detach()), 'max |grad|', float(z.grad.abs().max()), 'zeros', int((z.grad == 0).sum()))
    p = torch.softmax(seeded_logits('wide'), dim=1)
    assert int((p == 0).sum()) > 0, 'the wide case must have probabilities that are exactly 0'
    path = os.path.join(OUT, 'entropy_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    torch.set_num_threads(8)
    gen_entropy(load_reference())
