"""Offline pseudo-labels of a target split with class-wise entropy thresholds: what the reference's PseudoLabelingHookV4
(rsiseg/core/hook/pseudo_labeling_hookv4.py) and LoadAnnotationsPseudoLabelsV2 (rsiseg/datasets/pipelines/loading.py:392-520) compute
together, as a tool that runs beside the evaluation instead of inside (and ending) a training run.

  * thresholds: for every predicted class the entropy below which a share r of that class's pixels lies, over ALL pixels of ALL tiles --
    `thre@r`.  The cut is class-balanced: a rare, uncertain class keeps the same share of its pixels as a frequent, confident one.
  * labels: a pixel keeps its predicted class where its entropy lies below that class's threshold and is 255 elsewhere.

Only the low-resolution logits of the tiles are kept (on the device).  The order statistics come from an exact radix select over integer
histograms of the entropies' bit patterns (pfst_entropy_class_hist): no sort, no sampling, and nothing per pixel between the passes -- every
pass forms the entropies again from the low-resolution logits.  Deviations from the reference are listed in DESIGN.md §8i; the one that
changes numbers: with `thre_sample_ratio=1.0` the reference drops one pixel of a random permutation, here every pixel counts."""
import bisect

import numpy as np
import torch

from . import hip_ops as ops

DEFAULT_RATIOS = (0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)     # PseudoLabelingHookV4(cls_thre_ratios=...)
DEFAULT_LABEL_RATIO = 0.5                                  # LoadAnnotationsPseudoLabelsV2(pseudo_ratio=...)
BLOCK_TILES = 64                                           # tiles of one shape per launch
LDS_ENTRIES = 12288                                        # csrc/entropy_labels.hip: counters a workgroup privatises


def check_ratios(ratios, label_ratio=None):
    """-> the ratios as a list of floats.  0 <= r < 1 (the reference indexes sorted[int(n r)]: out of range at 1); `label_ratio`, when
    given, must be one of them"""
    ratios = [float(r) for r in ratios]
    if not ratios:
        raise ValueError('at least one threshold ratio is needed')
    for r in ratios:
        if not 0.0 <= r < 1.0:
            raise ValueError(f'threshold ratio {r} is outside [0, 1): thre@r is the entropy at rank int(n r) of n sorted values')
    if label_ratio is not None and float(label_ratio) not in ratios:
        raise ValueError(f'the label ratio {label_ratio} is not one of the threshold ratios {ratios}')
    return ratios


def rank_of(n, r):
    """the reference's `int(len(sorted_map) * cls_thre_ratio)`: a Python float product, truncated"""
    return int(int(n) * float(r))


def radix_levels(num_classes):
    """[(shift, bits), ...] from the most significant digit down, covering the 32 key bits: the widest digit (at most 11 bits: three
    levels) whose per-class table a workgroup can still privatise in LDS; from 49 classes on 8-bit digits through global atomics"""
    bits = next((b for b in (11, 10, 9, 8) if (num_classes << b) <= LDS_ENTRIES), 8)
    levels, rest = [], 32
    while rest > 0:
        b = min(bits, rest)
        levels.append((rest - b, b))
        rest -= b
    return levels


def digit_walk(hist_fn, ranks, levels, top=None):
    """The radix select as a pure function.  ranks[c]: the 0-based rank wanted in class c, or None for an empty class.
    hist_fn(shift, bits, prefix) -> integer array [C][1 << bits]: per class the counts of digit (key >> shift) & (2^bits - 1) over the keys
    whose higher bits equal prefix[c] (np.uint32 [C]; None at the first level: every key).  Per level and class: which bin holds the rank,
    and what rank remains inside it.  `top`: the first level's table when the caller has it already.
    -> np.uint32 [C], the key at rank ranks[c] of class c's keys in ascending order (0 for an empty class)"""
    C = len(ranks)
    prefix = [0] * C
    rem = [None if k is None else int(k) for k in ranks]
    assert sum(b for _, b in levels) == 32 and levels[-1][0] == 0 and all(levels[i][0] == levels[i + 1][0] + levels[i + 1][1]
                                                                         for i in range(len(levels) - 1))
    for li, (shift, bits) in enumerate(levels):
        if li == 0:
            h = top if top is not None else hist_fn(shift, bits, None)
        else:
            h = hist_fn(shift, bits, np.array(prefix, dtype=np.uint32))
        h = np.asarray(h)
        assert h.shape == (C, 1 << bits), (h.shape, C, bits)
        for c in range(C):
            if rem[c] is None:
                continue
            cum = np.cumsum(h[c].astype(np.int64))
            d = int(np.searchsorted(cum, rem[c], side='right'))           # the first bin whose cumulative count exceeds the rank
            if rem[c] < 0 or d >= cum.size:
                raise ValueError(f'class {c}: rank {ranks[c]} is outside its {int(cum[-1])} keys at level {li}')
            rem[c] -= int(cum[d - 1]) if d else 0
            prefix[c] = (prefix[c] << bits) | d
    return np.array(prefix, dtype=np.uint32)


class ClassEntropyThresholds:
    """Keeps the low-resolution logits of every tile on `device` and selects the class-wise entropy thresholds from them.  Tiles of equal
    shape (logits and target size) are gathered into blocks of up to BLOCK_TILES, one launch each."""

    def __init__(self, num_classes, device='cuda', max_bytes=None):
        if not 1 <= int(num_classes) <= 255:
            raise ValueError(f'ClassEntropyThresholds: {num_classes} classes (1 .. 255)')
        self.num_classes, self.device = int(num_classes), torch.device(device)
        self.max_bytes = max_bytes                 # None: what the device has free
        self.levels = radix_levels(self.num_classes)
        self._groups = {}                          # (h, w, H, W) -> dict(blocks=[tensor], starts=[int], pending=[tensor], tags=[...], n=int)
        self.bytes = 0
        self.passes = 0

    def __len__(self):
        return sum(g['n'] for g in self._groups.values())

    def _room(self):
        if self.max_bytes is not None:
            return int(self.max_bytes) - self.bytes
        free, _ = torch.cuda.mem_get_info(self.device)
        return free + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)

    def add(self, logits, size, tags=None):
        """logits [n, C, h, w] float32 on the device (copied), the tiles' full size (H, W), one tag per tile (a file stem; default: the
        running index)"""
        ops._chk(logits, ops.F32, 4)
        n, c, h, w = logits.shape
        if c != self.num_classes:
            raise ValueError(f'ClassEntropyThresholds.add: {c} classes, expected {self.num_classes}')
        tags = list(tags) if tags is not None else list(range(len(self), len(self) + n))
        if len(tags) != n:
            raise ValueError(f'ClassEntropyThresholds.add: {len(tags)} tags for {n} tiles')
        need = logits.numel() * 4
        key = (h, w, int(size[0]), int(size[1]))
        waiting = sum(t.shape[0] for t in self._groups[key]['pending']) if key in self._groups else 0
        # the copy, and the one concatenation that gathers the waiting tiles with these into blocks (now, or later for a last short block)
        if need + max(BLOCK_TILES, waiting + n) * c * h * w * 4 > self._room():
            raise MemoryError(f'the low-resolution logits of {len(self) + n} tiles ({(self.bytes + need) / 2 ** 20:.0f} MiB) do not fit in the '
                              "device's free memory: label fewer tiles at a time (--max-images)")
        g = self._groups.setdefault(key, dict(blocks=[], starts=[], pending=[], tags=[], n=0))
        g['pending'].append(logits.detach().clone(memory_format=torch.contiguous_format))
        g['tags'] += tags
        g['n'] += n
        self.bytes += need
        if sum(t.shape[0] for t in g['pending']) >= BLOCK_TILES:
            self._flush(g)
        return self

    @staticmethod
    def _flush(g):
        if g['pending']:
            block = g['pending'][0] if len(g['pending']) == 1 else torch.cat(g['pending'], 0)
            g['pending'] = []
            for i in range(0, block.shape[0], BLOCK_TILES):            # one add() may bring more than a block
                part = block[i:i + BLOCK_TILES]
                g['starts'].append(g['starts'][-1] + g['blocks'][-1].shape[0] if g['blocks'] else 0)
                g['blocks'].append(part)

    def blocks(self):
        """-> [(logits block [n, C, h, w], (H, W), tags of its tiles)] in group order"""
        out = []
        for (h, w, H, W), g in self._groups.items():
            self._flush(g)
            for start, b in zip(g['starts'], g['blocks']):
                out.append((b, (H, W), g['tags'][start:start + b.shape[0]]))
        return out

    def tile(self, tag):
        """-> (logits [1, C, h, w], (H, W)) of the tile added under `tag`"""
        for (h, w, H, W), g in self._groups.items():
            if tag in g['tags']:
                self._flush(g)
                j = g['tags'].index(tag)
                k = bisect.bisect_right(g['starts'], j) - 1
                return g['blocks'][k][j - g['starts'][k]:j - g['starts'][k] + 1], (H, W)
        raise KeyError(tag)

    def class_hist(self, shift, bits, prefix=None):
        """one radix level over every tile -> np.int64 [C][1 << bits] (one small device read)"""
        hist = torch.zeros(self.num_classes, 1 << bits, dtype=torch.int64, device=self.device)
        pre = None if prefix is None else torch.from_numpy(np.asarray(prefix, np.uint32).view(np.int32).copy()).to(self.device)
        for block, size, _ in self.blocks():
            ops.entropy_class_hist(block, size, shift, bits, hist, pre)
        self.passes += 1
        return hist.cpu().numpy()

    def thresholds(self, ratios=DEFAULT_RATIOS):
        """-> (table float32 [R][C]: thre@r of every class, n_c int64 [C]: pixels predicted per class).  thr = sorted(H | pred == c)[int(n_c r)]
        over all tiles, bit for bit; 0 for a class that is never predicted.  The first level is shared by all ratios; every further level is
        one pass over the tiles per ratio (1 + (L - 1) R passes).  A known simplification: one pass per level could serve all ratios with a
        prefix table per ratio; at the measured cost of a pass it would not be noticed beside the network forwards."""
        ratios = check_ratios(ratios)
        if len(self) == 0:
            raise ValueError('ClassEntropyThresholds.thresholds: no tiles were added')
        top = self.class_hist(*self.levels[0])
        n_c = top.sum(axis=1).astype(np.int64)
        table = np.zeros((len(ratios), self.num_classes), np.float32)
        for i, r in enumerate(ratios):
            ranks = [rank_of(n, r) if n > 0 else None for n in n_c]
            table[i] = digit_walk(self.class_hist, ranks, self.levels, top=top).view(np.float32)
        return table, n_c


def label_maps(logits, size, thr, annotation_space=False, counts=None):
    """logits [N, C, h, w] on the device, thr: C floats (a row of the threshold table) -> (labels uint8 [N, H, W] on the device, counts
    int64 [C, 2] on the device, += per class (predicted, kept)).  annotation_space: arg-max + 1 and 0 instead of arg-max and 255, the
    files a dataset with reduce_zero_label=True reads."""
    thr_d = torch.as_tensor(np.asarray(thr, np.float32)).to(logits.device) if not torch.is_tensor(thr) else thr
    return ops.entropy_pseudo_label(logits, size, thr_d, annotation_space, counts)


@torch.no_grad()
def collect(seg, dataset, acc, max_images=None):
    """One pass over a TileFolder built with test_mode=True: per tile ONE EncoderDecoder.eval_features forward whose low-resolution logits
    go into `acc` (a ClassEntropyThresholds) under the file's stem.  Labels must land on the image grid: single-view items only, not
    flipped, input size == ori_shape; whole-image inference only.  -> the stems, in dataset order"""
    mode = (getattr(seg, 'test_cfg', None) or {}).get('mode', 'whole')
    if mode != 'whole':
        raise NotImplementedError(f'pseudo-labels are made from whole-tile logits; test_cfg mode {mode!r} is not built')
    dev = next(seg.parameters()).device
    n = len(dataset) if max_images is None else min(len(dataset), max_images)
    stems = []
    for i in range(n):
        item = dataset[i]
        if isinstance(item['img'], list):
            raise ValueError('collect reads single-view items; the pipeline makes several views (test-time augmentation)')
        meta = item['img_metas']
        size = tuple(item['img'].shape[1:])
        if meta.get('flip'):
            raise ValueError(f"{meta.get('filename')}: a flipped view; its labels would not land on the image grid")
        if 'ori_shape' in meta and tuple(meta['ori_shape'][:2]) != size:
            raise ValueError(f"{meta.get('filename')}: the pipeline resizes {tuple(meta['ori_shape'][:2])} to {size}; pseudo-labels are written on "
                             'the image grid, take the Resize out of the pipeline')
        stem = str(meta.get('filename', i)).split('/')[-1].rsplit('.', 1)[0]
        if stem in stems:
            raise ValueError(f'two tiles share the stem {stem!r}: their label maps would overwrite each other')
        out = seg.eval_features(item['img'][None].to(dev))
        acc.add(out['seg_logits'], size, [stem])
        stems.append(stem)
    return stems
