#!/usr/bin/env python3
"""Every launch of a documented workload as one line of text -- what a host-side refactor is compared by: two versions that load the same
libpfst_hip.so (PFST_HIP_LIB) behave the same exactly when their traces are equal line for line (profiles/conv_dispatch_refactor.txt section 1,
profiles/norm_fold_refactor.txt).

    python tools/launch_trace.py OUT [--folds-off] [--deterministic] [--no-train] [--no-eval]

hip_ops.call is wrapped; a line is the entry name, every scalar argument by value and every pointer argument (the stream included) as
null / ptr by the kinds of _lib.parse_header(), a non-null pfst_bnb_fuse_t as (relu, y set?, y_mask set?).
Workload: the flagship preset (b = 8 x 1024^2), fill_state_dict(seed 0), synth_batch(seed 1234), two train steps (the second replays the
recorded packing launches); then one sliding-window inference as tests/test_eval_gpu.py runs it (2 x 3 x 160 x 224, crop 128, stride 85)
with the SHA-256 of the returned probabilities as the last line.  The arithmetic is the environment's PFST_CONV_MATH.
--folds-off: layers.DEFER_BN_APPLY = False, every normalised tensor is written.
--deterministic: ops.set_deterministic(True); after each step a line with the SHA-256 of the gradient arena, of the student's and the
teacher's parameters, and the step's log values as float.hex."""
import argparse
import ctypes
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def install(lines):
    """wrap hip_ops.call: append one line per launch to `lines`"""
    from pfst_amd import _lib, hip_ops
    decls, inner = _lib.parse_header(), hip_ops.call

    def fmt(kind, name, v):
        if kind is not ctypes.c_void_p:
            return f'{name}={v!r}'
        if not v:
            return f'{name}=null'
        if name == 'bnb':
            s = hip_ops._BnbFuseStruct.from_address(v)
            return f'bnb=(relu={s.relu}, y={bool(s.y)}, y_mask={bool(s.y_mask)})'
        return f'{name}=ptr'

    def call(name, *args):
        lines.append(name + ' ' + ' '.join(fmt(k, a, v) for (k, a), v in zip(decls[name][1], args)))
        return inner(name, *args)
    hip_ops.call = call


def train_steps(lines, deterministic):
    from pfst_amd import hip_ops
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import OPTIMIZER, workload_cfg
    from pfst_amd.registry import UDA
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    cfg, w = workload_cfg('pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8')
    batch = synth_batch(w['per_gpu_batch'], w['size'], w['num_classes'], w['in_channels'], seed=1234, device='cuda')
    hip_ops.set_deterministic(deterministic)
    model = UDA.build(cfg)
    fill_state_dict(model.state_dict(), 0)
    model.cuda()
    opt = build_optimizer(model, OPTIMIZER)
    random.seed(0); np.random.seed(0); torch.manual_seed(0); torch.cuda.manual_seed_all(0)
    for step in range(2):
        lines.append(f'# train step {step}')
        log = model.train_step(batch, opt)['log_vars']
        torch.cuda.synchronize()
        if deterministic:
            lines.append(f'# step{step} grad {sha(model.student_arena.grad)} student {sha(model.student_arena.data)} '
                         f'teacher {sha(model._teacher_arena.data)} log ' + ' '.join(f'{k}={float(v).hex()}' for k, v in log.items()))
    hip_ops.set_deterministic(False)
    del model, opt, batch
    torch.cuda.empty_cache()


def slide_eval(lines):
    from helpers import seeded_pfgst_state, uda_cfg
    from oracle import pfst_oracle as O
    from pfst_amd.registry import UDA
    cfg = uda_cfg()
    cfg['model']['test_cfg'] = dict(mode='slide', crop_size=(128, 128), stride=(85, 85))
    model = UDA.build(cfg)
    both, _, _ = seeded_pfgst_state(O, 9)
    g = torch.Generator().manual_seed(1)
    for k, v in both.items():                      # non-trivial running statistics
        if k.endswith('running_mean'):
            v.copy_(0.05 * torch.randn(v.shape, generator=g))
        elif k.endswith('running_var'):
            v.copy_(0.8 + 0.4 * torch.rand(v.shape, generator=g))
    model.load_state_dict(both, strict=False)
    model.cuda()
    img = torch.randn(2, 3, 160, 224, generator=torch.Generator().manual_seed(3))
    metas = [dict(ori_shape=(176, 232, 3), flip=False)] * 2
    lines.append('# sliding-window eval')
    probs, _ = model.get_model().inference_probs(img.cuda(), metas, True)
    torch.cuda.synchronize()
    lines.append(f'# probabilities {sha(probs)}')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('out')
    ap.add_argument('--folds-off', action='store_true')
    ap.add_argument('--deterministic', action='store_true')
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--no-eval', action='store_true')
    args = ap.parse_args()
    import pfst_amd  # noqa: F401
    from pfst_amd import layers
    if args.folds_off:
        layers.DEFER_BN_APPLY = False
    lines = []
    install(lines)
    if not args.no_train:
        train_steps(lines, args.deterministic)
    if not args.no_eval:
        slide_eval(lines)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print(f'{args.out}: {sum(not l.startswith("#") for l in lines)} launches, math {layers.CONV_MATH}')


if __name__ == '__main__':
    main()
