#!/usr/bin/env python3
"""Golden vectors for the offline pseudo-labels, produced by EXECUTING the reference's
PseudoLabelingHookV4._cal_threshold (rsiseg/core/hook/pseudo_labeling_hookv4.py:173-205) and LoadAnnotationsPseudoLabelsV2.__call__
(rsiseg/datasets/pipelines/loading.py:435-520) on the CPU through make_golden.py's loader.  Neither file needs more than import stand-ins:
empty modules for h5py, tqdm, mmcv's hook classes, pycocotools, cv2 and tifffile, and an in-memory stand-in for `h5py.File` that hands the
loader the arrays the hook would have written (`seg_logits`, `thre@r`).  Only seeded inputs and the numbers the reference returns are stored.

Input: full-resolution fp32 logits N(0, 3^2), N = 2, C = 6, 40 x 36 (the identity-size case of the kernels).  The hook is called with
thre_sample_ratio = 1.0, which drops ONE pixel of a seeded random permutation; its flat index (over N, H, W) is recorded as `dropped`.
The script checks its own seed: against the float64 restatement (tests/pseudo_label_oracle.py) at most 1 % of the pixels may have a top-2
probability gap below 1e-5 or an entropy within 1e-5 of their class's threshold (the pixels the GPU test leaves out).

Usage:  python tests/golden/make_golden_pseudo_labels.py        (writes tests/golden/pseudo_labels.npz)
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, _load, _install_loader_shims  # noqa: E402
import pseudo_label_oracle as oracle  # noqa: E402

SEED, NP_SEED = 11, 5
N, C, H, W = 2, 6, 40, 36
RATIOS = [0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5]
LABEL_RATIO = 0.5

_H5 = {}          # path -> {dataset name: array}: what the hook's h5py.File(...).create_dataset calls would have left on disk


class MemoryH5File:
    def __init__(self, path, mode='r'):
        self.store = _H5.setdefault(path, {})

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def __getitem__(self, key):
        return self.store[key]

    def create_dataset(self, name, data=None):
        self.store[name] = np.asarray(data)

    def close(self):
        pass


def install_stand_ins():
    sys.dont_write_bytecode = True
    _install_loader_shims()

    def mod(name, **attrs):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__dict__.update(attrs)
        if not hasattr(m, '__path__'):
            m.__path__ = []
        sys.modules[name] = m
        return m

    class Hook:
        def every_n_iters(self, runner, n):
            return False

    Registry = sys.modules['mmcv.utils'].Registry
    mod('h5py', File=MemoryH5File)
    mod('tqdm', tqdm=lambda it, *a, **k: it)
    mod('pycocotools')
    mod('pycocotools.mask')
    mod('cv2', imread=None)
    mod('tifffile')
    mod('mmcv.utils', digit_version=lambda v: tuple(int(x) for x in v.split('.')[:3]))
    mod('mmcv.runner', HOOKS=Registry('hook'))
    mod('mmcv.runner.dist_utils', master_only=lambda f: f)
    mod('mmcv.runner.hooks', Hook=Hook)
    mod('mmcv.runner.hooks.checkpoint', CheckpointHook=Hook)
    mod('mmcv.runner.hooks.logger')
    mod('mmcv.runner.hooks.logger.wandb', WandbLoggerHook=Hook)
    for pkg in ('rsiseg', 'rsiseg.core', 'rsiseg.core.hook', 'rsiseg.ops', 'rsiseg.datasets', 'rsiseg.datasets.pipelines'):
        mod(pkg)
    sys.modules['rsiseg.ops'].resize = None
    sys.modules['rsiseg.core'].DistEvalHook = sys.modules['rsiseg.core'].EvalHook = Hook
    mod('rsiseg.datasets.builder', PIPELINES=Registry('pipeline'))


def main():
    install_stand_ins()
    hook_mod = _load('rsiseg.core.hook.pseudo_labeling_hookv4', 'rsiseg/core/hook/pseudo_labeling_hookv4.py')
    load_mod = _load('rsiseg.datasets.pipelines.loading', 'rsiseg/datasets/pipelines/loading.py')
    g = torch.Generator().manual_seed(SEED)
    logits = (torch.randn(N, C, H, W, generator=g) * 3).contiguous()

    hook = hook_mod.PseudoLabelingHookV4(log_dir=tempfile.mkdtemp(), cls_thre_ratios=list(RATIOS))
    np.random.seed(NP_SEED)
    thre_map = hook._cal_threshold(logits.clone(), sample_ratio=1.0)
    np.random.seed(NP_SEED)
    dropped = np.random.permutation(N * H * W)[N * H * W - 1:]          # [:int(n * 1.0) - 1] keeps all but the last
    table = np.array([[np.float32(v) for v in thre_map[f'thre@{r}']] for r in RATIOS], dtype=np.float32)

    labels = []
    for i in range(N):
        with MemoryH5File(f'mem/tile{i}.h5', 'w') as hf:                   # what after_train_iter writes per tile (:132-137, :157-160)
            hf.create_dataset('seg_logits', data=logits[i].numpy())
            for key, value in thre_map.items():
                hf.create_dataset(key, data=value)
        loader = load_mod.LoadAnnotationsPseudoLabelsV2(pseudo_labels_dir='mem', pseudo_ratio=LABEL_RATIO)
        res = loader(dict(img_info=dict(filename=f'tile{i}.png'), seg_fields=[], img_shape=(H, W)))
        labels.append(res['gt_semantic_seg'])
    labels = np.stack(labels).astype(np.uint8)

    # the seed's own check against the float64 restatement
    z = oracle.upsample64(logits.numpy(), (H, W))
    p = oracle.softmax64(z)
    e0, q0 = oracle.hook_entropy(p)
    e1, q1 = oracle.loader_entropy(z, p)
    t64, n_c = oracle.thresholds(e0, q0, RATIOS, C, drop=dropped)
    thr = table[RATIOS.index(LABEL_RATIO)].astype(np.float64)
    excluded = (oracle.top2_gap(p) < 1e-5) | (np.abs(e1 - thr[q1]) <= 1e-5)
    lab64, _ = oracle.labels(e1, q1, thr)
    print('thresholds: max |reference - fp64|', float(np.abs(table - t64).max()), 'n_c', n_c.tolist())
    print('labels: excluded', int(excluded.sum()), 'of', excluded.size, '; mismatches outside', int(((lab64 != labels) & ~excluded).sum()),
          '; kept', int((labels != 255).sum()))
    assert excluded.mean() <= 0.01 and not ((lab64 != labels) & ~excluded).any() and np.abs(table - t64).max() <= 1e-5

    path = os.path.join(OUT, 'pseudo_labels.npz')
    np.savez_compressed(path, logits=logits.numpy(), ratios=np.array(RATIOS, np.float64), label_ratio=np.float64(LABEL_RATIO), thresholds=table,
                        labels=labels, dropped=dropped.astype(np.int64))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
