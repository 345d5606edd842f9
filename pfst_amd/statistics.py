"""Pseudo-feature statistics over a labelled set: what the reference's PlotStatisticsHook
(rsiseg/core/hook/plot_statistics_hook.py) collects to justify PFGSTLoss's options, restated as a diagnostic that runs beside the evaluation
instead of inside (and ending) a training run.  For every pixel pair (centre, dilated neighbour) of a feature map:

  * similarity histograms, split by whether the prediction and the annotation each call the pair "same class" -- the paper's cases
    1a / 1b / 2b / 2a: does this feature level / similarity type / dilation separate classes at all?
  * the local-rank table: how often the neighbour at rank r of the centre's similarity order really has the centre's class, and with it the
    purity of a positive set of the r most similar neighbours.

The counting is one kernel (pfst_sim_pair_stats) behind the similarity map the loss already uses; everything here is bookkeeping around it."""
import numpy as np
import torch

from . import hip_ops as ops

CASES = ('1a', '1b', '2b', '2a')      # histogram rows: (pred same, gt same), (pred same, gt different), (both different), (pred different, gt same)
MAX_BINS = 256


def bin_edges(bins, lo, hi):
    """bins + 1 float32 edges: lo + (hi - lo) i / bins in float64, then rounded -- the table the kernel bins against"""
    i = np.arange(bins + 1, dtype=np.float64)
    return (np.float64(lo) + (np.float64(hi) - np.float64(lo)) * i / np.float64(bins)).astype(np.float32)


def _share(a, b):
    return None if b == 0 else a / b


class SimStatistics:
    """The accumulator of one setting (kernel size, feature-grid dilation, similarity type, bins): owns the edge table and the int64
    counter tensor on `device`.  Counters are exact integers that launches add to, so a result does not depend on the order of the images,
    of the summation or of the streams."""

    def __init__(self, ksize=3, dilation=2, sim_type='cosine', sigma=30.0, bins=25, lo=0.0, hi=1.0, device='cuda'):
        if ksize not in (3, 5, 7) or int(dilation) < 1 or sim_type not in ops.SIM_TYPES:
            raise ValueError(f'SimStatistics: kernel size {ksize} (3 | 5 | 7), dilation {dilation} (>= 1), sim_type {sim_type!r}')
        if not (1 <= int(bins) <= MAX_BINS) or not float(lo) < float(hi):
            raise ValueError(f'SimStatistics: bins {bins} (1 .. {MAX_BINS}), range [{lo}, {hi}]')
        if sim_type == 'gaussian' and not float(sigma) > 0:
            raise ValueError(f'SimStatistics: sigma {sigma}')
        self.ksize, self.dilation, self.sim_type, self.sigma = int(ksize), int(dilation), sim_type, float(sigma)
        self.bins, self.lo, self.hi = int(bins), float(lo), float(hi)
        self.edges_host = bin_edges(self.bins, self.lo, self.hi)
        self.edges = torch.from_numpy(self.edges_host).to(device)
        kk = self.ksize * self.ksize
        self.counters = torch.zeros(4 * (self.bins + 2) + 2 * (kk - 1) + 2, dtype=torch.int64, device=device)

    def settings(self):
        return dict(kernel_size=self.ksize, dilation=self.dilation, sim_type=self.sim_type, sigma=self.sigma, bins=self.bins,
                    range=[self.lo, self.hi])

    def update(self, feat, pred_u8, gt_u8):
        """feat [N, C, h, w] float32, pred_u8 [N, hp, wp], gt_u8 [N, hg, wg] (255 = ignore), all on the device: the similarity map of
        `feat`, then its pair statistics added to the counters"""
        sim, _ = ops.sim_map(feat, self.dilation, self.sim_type, self.sigma, ksize=self.ksize)
        ops.sim_pair_stats(sim, pred_u8, gt_u8, self.dilation, self.ksize, self.edges, self.counters)
        return self

    def merge(self, other):
        """adds the counters of another accumulator of the same setting (it may live on another device)"""
        if self.settings() != other.settings():
            raise ValueError(f'SimStatistics.merge: {self.settings()} != {other.settings()}')
        self.counters += other.counters.to(self.counters.device)
        return self

    def result(self):
        """One device read -> a plain dict (JSON-ready): the settings, `edges`, the integer counters
            hist[4][bins + 2]   rows in CASES order; per row the bins, then the counts below `lo` and above `hi`
            rank[K^2 - 1][2]    per local rank (same class, different class)
            n_centres, n_correct_centres
        and three tables derived from them in Python (None where a denominator is empty):
            hist_norm[4][bins]  each case's in-range histogram normalised to sum 1 (the bar heights the reference plots)
            rank_same[r]        rank[r][0] / (rank[r][0] + rank[r][1])
            rank_purity[r]      the same share over the ranks 0 .. r together: the purity of a top_k = r + 1 positive set"""
        c = [int(v) for v in self.counters.cpu().tolist()]
        hs, kk = self.bins + 2, self.ksize * self.ksize
        hist = [c[i * hs:(i + 1) * hs] for i in range(4)]
        rank = [c[4 * hs + 2 * r:4 * hs + 2 * r + 2] for r in range(kk - 1)]
        hist_norm = []
        for row in hist:
            tot = sum(row[:self.bins])
            hist_norm.append([_share(v, tot) for v in row[:self.bins]])
        same = diff = 0
        rank_same, rank_purity = [], []
        for a, b in rank:
            same, diff = same + a, diff + b
            rank_same.append(_share(a, a + b))
            rank_purity.append(_share(same, same + diff))
        out = self.settings()
        out.update(cases=list(CASES), edges=[float(e) for e in self.edges_host], hist=hist, rank=rank, n_centres=c[-2],
                   n_correct_centres=c[-1], hist_norm=hist_norm, rank_same=rank_same, rank_purity=rank_purity)
        return out


def _feature_stride(backbone, level):
    """input pixels per pixel of backbone feature map `level` (ResNetV1c: a stride-4 stem, then the stages' strides)"""
    s = 4
    for st in tuple(backbone.get('strides', (1, 2, 2, 2)))[:level + 1]:
        s *= int(st)
    return s


def feature_dilation(cfg, feature, dilation, downscale):
    """A PFGSTLoss `dilation` (in pixels of the loss grid) in pixels of the grid of `feature` ('decoded' or a backbone level), the way
    PFGSTLoss.forward derives it: the loss grid is the 1/4-resolution logit grid scaled by `downscale`, a coarser feature map is replicated
    u x u onto it, and a dilation-d neighbourhood there is the dilation-d/u neighbourhood of the feature grid."""
    model = cfg['model']
    backbone = model['backbone']
    ds = 1 if downscale is None else int(round(1.0 / downscale))
    loss_stride = _feature_stride(backbone, 0) * ds                        # the decode head's logits live on the c1 (level 0) grid
    level = model['decode_head'].get('in_index', -1) if feature == 'decoded' else int(feature)
    if isinstance(level, (list, tuple)):                                   # a multi-level head (UPerHead) decodes on the grid of its first level
        level = int(level[0])
    level = level % len(tuple(backbone.get('out_indices', (0, 1, 2, 3))))
    fs = _feature_stride(backbone, level)
    if feature == 'decoded' and model.get('neck') is not None and 'feature_strides' in model['decode_head']:
        # behind a neck (Semantic FPN) level i is still backbone level i's grid; the head decodes on the grid of its first feature stride
        fs = int(model['decode_head']['feature_strides'][0])
    if fs % loss_stride != 0:
        raise NotImplementedError(f'feature {feature!r} (stride {fs}) is finer than the loss grid (stride {loss_stride})')
    u = fs // loss_stride
    if dilation % u != 0:
        raise NotImplementedError(f'dilation {dilation} not divisible by the feature up-sampling factor {u}')
    return dilation // u


def settings_from_config(cfg):
    """The defaults of tools/sim_statistics.py -> dict(feature, kernel_size, dilation, sim_type, sigma): what the config's own `uda`
    section trains with (use_decoded_feats and the first PFGSTLoss's feat_level, kernel_size, sim_type, sigma; its dilation in feature-grid
    pixels).  Without a `uda` section: decoded features, K = 3, d = 2, cosine."""
    uda = cfg.get('uda') or {}
    loss = next((a for a in uda.get('aux_losses') or [] if a.get('type') == 'PFGSTLoss'), None)
    if loss is None:
        return dict(feature='decoded', kernel_size=3, dilation=2, sim_type='cosine', sigma=30.0)
    feature = 'decoded' if uda.get('use_decoded_feats', False) else loss.get('feat_level', 2)      # 2: PFGSTLoss's own default
    if feature is None:
        raise ValueError('the config trains on backbone features (use_decoded_feats=False) but its PFGSTLoss has feat_level=None')
    return dict(feature=feature, kernel_size=int(loss['kernel_size']),
                dilation=feature_dilation(cfg, feature, int(loss['dilation']), loss.get('downscale')),
                sim_type=loss.get('sim_type', 'gaussian'), sigma=float(loss.get('sigma', 30)))


def select_feature(out, feature):
    """the map of EncoderDecoder.eval_features' dict that `feature` ('decoded' or a backbone level 0..3) names"""
    return out['decoded_feats'] if feature == 'decoded' else out['feats'][int(feature)]


@torch.no_grad()
def collect_sim_statistics(seg, dataset, specs, feature='decoded', max_images=None):
    """One pass over a labelled TileFolder (built with test_mode=True: items without annotations, `gt_seg_map(i)` for the ground truth, which
    already has reduce_zero_label applied): per image ONE EncoderDecoder.eval_features forward, the arg-max of its low-resolution logits
    as the prediction, and every accumulator of `specs` updated from that forward.
    specs: SimStatistics, or (feature, SimStatistics) pairs to read several feature maps; `feature` names the map of the bare ones.
    -> the number of images"""
    specs = [s if isinstance(s, (tuple, list)) else (feature, s) for s in specs]
    dev = next(seg.parameters()).device
    n = len(dataset) if max_images is None else min(len(dataset), max_images)
    for i in range(n):
        item = dataset[i]
        if isinstance(item['img'], list):
            raise ValueError('collect_sim_statistics reads single-view items; the pipeline makes several views (test-time augmentation)')
        out = seg.eval_features(item['img'][None].to(dev))
        pred = ops.argmax_nchw(out['seg_logits'])
        gt = torch.from_numpy(np.ascontiguousarray(dataset.gt_seg_map(i), dtype=np.uint8))[None].to(dev)
        for feat_name, stat in specs:
            stat.update(select_feature(out, feat_name).contiguous(), pred, gt)
    return n


class SyntheticTiles:
    """`n` seeded synthetic labelled tiles with the item layout of a TileFolder built with test_mode=True: N(0, 1) images and label maps
    of constant `block` x `block` squares (so that same-class pairs exist) with a 255 patch, from pfst_amd.synthetic.synth_batch"""

    def __init__(self, n, size=128, num_classes=6, in_channels=3, seed=1234, block=32):
        from .synthetic import synth_batch
        self.items = [synth_batch(1, size, num_classes, in_channels, seed=seed + i, block=min(block, size)) for i in range(n)]

    def __len__(self):
        return len(self.items)

    def gt_seg_map(self, idx):
        return self.items[idx]['gt_semantic_seg'][0, 0].numpy().astype(np.uint8)

    def __getitem__(self, idx):
        b = self.items[idx]
        return dict(img=b['img'][0], img_metas=dict(filename=f'synthetic{idx}', ori_shape=tuple(b['img'].shape[2:]) + (3,)))


def purity_table(results):
    """the per-rank purity of every result as a text table, one row per setting"""
    width = max((len(r['rank_purity']) for r in results), default=0)
    fmt = lambda v: '    -' if v is None else f'{v:5.3f}'
    lines = ['feature  K  d  sim       centres  | purity of the top-r neighbours, r = 1 .. ' + str(width)]
    for r in results:
        lines.append(f"{str(r.get('feature', '?')):>7s}  {r['kernel_size']}  {r['dilation']}  {r['sim_type']:8s} {r['n_centres']:8d}  | "
                     + ' '.join(fmt(v) for v in r['rank_purity']))
    return '\n'.join(lines)
