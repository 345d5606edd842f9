"""Pseudo-feature statistics on the GPU: pfst_sim_pair_stats against a NumPy / torch-CPU restatement of its definition, fed the
very similarity tensor the kernel reads -- every counter must be EQUAL --, then the path above it: SimStatistics, EncoderDecoder.eval_features,
collect_sim_statistics and tools/sim_statistics.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the oracle
def oracle(sim, pred, gt, K, d, edges):
    """sim [N, K^2, h, w] float32, pred [N, hp, wp] / gt [N, hg, wg] uint8 (NumPy), edges float32 [bins + 1] ->
    (counters int64 in the kernel's layout, number of ignored taps of correct centres)"""
    sim = np.asarray(sim, np.float32)
    N, KK, h, w = sim.shape
    R, c, bins = K // 2, KK // 2, len(edges) - 1
    near = lambda m: F.interpolate(torch.from_numpy(np.asarray(m)).float()[:, None], size=(h, w), mode='nearest')
    unf = lambda m: F.unfold(m, K, dilation=d, padding=R * d).view(N, KK, h, w).numpy()
    p, g = near(pred), near(gt)
    inside = unf(torch.ones(N, 1, h, w)).min(axis=1) == 1                    # explicit: every tap inside the map
    up, ug = unf(p), unf(g)                                                 # [N, KK, h, w]; the padding's zeros never count (inside mask)
    pc, gc = p[:, 0].numpy(), g[:, 0].numpy()
    counted = inside & (gc != 255)
    correct = counted & (pc == gc)
    nc = [k for k in range(KK) if k != c]                                   # the centre leaves by index
    s, ug_nc, up_nc = sim[:, nc], ug[:, nc], up[:, nc]
    order = np.argsort(-s, axis=1, kind='stable')                           # descending, the lower tap first on ties
    g_sorted = np.take_along_axis(ug_nc, order, axis=1)
    rank = np.zeros((KK - 1, 2), np.int64)
    for r in range(KK - 1):
        live = counted & (g_sorted[:, r] != 255)
        rank[r, 0] = np.sum(live & (g_sorted[:, r] == gc))
        rank[r, 1] = np.sum(live & (g_sorted[:, r] != gc))
    hist = np.zeros((4, bins + 2), np.int64)
    live = correct[:, None] & (ug_nc != 255)
    psame, gsame = up_nc == pc[:, None], ug_nc == gc[:, None]
    case = np.where(psame, np.where(gsame, 0, 1), np.where(gsame, 3, 2))
    b = np.searchsorted(edges, s.ravel(), side='right').reshape(s.shape) - 1
    slot = np.where(s < edges[0], bins, np.where(s > edges[-1], bins + 1, np.minimum(b, bins - 1)))      # v == hi: the last bin
    np.add.at(hist, (case[live], slot[live]), 1)
    ignored = int(np.sum(correct[:, None] & (ug_nc == 255)))
    counters = np.concatenate([hist.ravel(), rank.ravel(), [counted.sum(), correct.sum()]]).astype(np.int64)
    return counters, ignored


def split(counters, K, bins):
    hs, KK = bins + 2, K * K
    return counters[:4 * hs].reshape(4, hs), counters[4 * hs:4 * hs + 2 * (KK - 1)].reshape(KK - 1, 2), int(counters[-2]), int(counters[-1])


# ---------------------------------------------------------------------------------------------------------------- inputs
def edges_of(bins, lo=0.0, hi=1.0):
    from pfst_amd.statistics import bin_edges
    return bin_edges(bins, lo, hi)


def make_inputs(N, h, w, K, bins, seed, pred_factor=2, gt_factor=4, ignore=True):
    """similarities quantised to eighths in [-0.25, 1.125] (frequent ties, values below lo and above hi) with a sprinkling of exact edge
    values, of 1 + 2^-23 and 1.5, and of copies of the neighbouring tap; blocky labels with a 255 block and scattered 255 pixels; a
    prediction that agrees with the annotation on about half of the pixels"""
    g = torch.Generator().manual_seed(seed)
    KK = K * K
    sim = torch.randint(-2, 10, (N, KK, h, w), generator=g).float() / 8
    e = torch.from_numpy(edges_of(bins))
    pick = torch.rand(sim.shape, generator=g)
    sim = torch.where(pick < 0.15, e[torch.randint(0, bins + 1, sim.shape, generator=g)], sim)       # exactly on bin edges
    sim = torch.where((pick >= 0.15) & (pick < 0.18), torch.tensor(1.0 + 2.0 ** -23), sim)
    sim = torch.where((pick >= 0.18) & (pick < 0.20), torch.tensor(1.5), sim)
    copy = torch.rand(N, KK - 1, h, w, generator=g) < 0.1
    sim[:, 1:] = torch.where(copy, sim[:, :-1], sim[:, 1:])                                           # exact copies of the tap before
    hg, wg = h * gt_factor, w * gt_factor
    blocks = torch.randint(0, 4, (N, 1, (hg + 15) // 16, (wg + 15) // 16), generator=g)
    gt = blocks.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, 0, :hg, :wg].clone()
    noise = torch.rand(N, hg, wg, generator=g) < 0.1
    gt = torch.where(noise, torch.randint(0, 4, gt.shape, generator=g), gt)
    hp, wp = h * pred_factor, w * pred_factor
    pred = F.interpolate(gt[:, None].float(), size=(hp, wp), mode='nearest')[:, 0].long()
    flip = torch.rand(N, hp, wp, generator=g) < 0.5
    pred = torch.where(flip, torch.randint(0, 4, pred.shape, generator=g), pred)
    if ignore:
        gt[:, hg // 8:hg // 8 + 5 * gt_factor, wg // 4:wg // 4 + 6 * gt_factor] = 255
        gt = torch.where(torch.rand(N, hg, wg, generator=g) < 0.03, torch.tensor(255), gt)
    return sim.contiguous(), pred.to(torch.uint8).contiguous(), gt.to(torch.uint8).contiguous()


def run_kernel(sim, pred, gt, K, d, edges, counters=None):
    from pfst_amd import hip_ops as ops
    dev = torch.device('cuda')
    e = torch.from_numpy(edges).to(dev)
    if counters is None:
        counters = torch.zeros(ops.sim_pair_stats_counters(K, len(edges) - 1), dtype=torch.int64, device=dev)
    return ops.sim_pair_stats(sim.to(dev), pred.to(dev), gt.to(dev), d, K, e, counters)


# ---------------------------------------------------------------------------------------------------------------- kernel level
SHAPES = [(2, 24, 20, 3, 2), (2, 24, 20, 5, 2), (2, 24, 20, 7, 3), (2, 24, 20, 7, 4), (3, 72, 64, 3, 2), (3, 72, 64, 5, 2), (3, 72, 64, 7, 3)]


@pytest.mark.parametrize('bins', [25, 256])
@pytest.mark.parametrize('N,h,w,K,d', SHAPES)
def test_counters_equal_the_oracle(N, h, w, K, d, bins):
    edges = edges_of(bins)
    sim, pred, gt = make_inputs(N, h, w, K, bins, seed=100 * K + d + h)
    assert pred.shape[1:] == (2 * h, 2 * w) and gt.shape[1:] == (4 * h, 4 * w)
    got = run_kernel(sim, pred, gt, K, d, edges).cpu().numpy()
    want, ignored = oracle(sim.numpy(), pred.numpy(), gt.numpy(), K, d, edges)
    hist, rank, n, nc = split(got, K, bins)
    whist, wrank, wn, wnc = split(want, K, bins)
    print(f'K {K} d {d} {N}x{h}x{w} bins {bins}: centres {n} / {wn}, correct {nc} / {wnc}, pairs {hist.sum()} / {whist.sum()}, '
          f'below {hist[:, bins].sum()}, above {hist[:, bins + 1].sum()}')
    assert np.array_equal(got, want)
    # the identities of the tables
    assert np.all(rank.sum(axis=1) <= n)
    assert hist.sum() == (K * K - 1) * nc - ignored
    if (K // 2) * d * 2 >= min(h, w):                 # (7, 4) on 24 x 20: no centre has all its taps inside
        assert not got.any()
    elif wn >= 100:                                   # enough centres for every kind of pair to occur (the inputs are seeded)
        assert nc > 0 and ignored > 0 and hist[:, bins].sum() > 0 and hist[:, bins + 1].sum() > 0
        assert (hist[:, :bins] > 0).any(axis=1).all()                    # all four cases
    else:
        assert wn > 0
    if (K, d, h) == (7, 3, 24):
        assert wn <= N * 6 * 2                                           # 6 x 2 centres per image before the 255 ones leave


def test_grid_stride_and_many_blocks_per_counter():
    """300 images share the launch's block budget (6 blocks each), so a block walks its 48 x 44 image in two strides, the second partial,
    and 1800 blocks add to every counter"""
    K, d, bins = 3, 2, 25
    edges = edges_of(bins)
    sim, pred, gt = make_inputs(300, 48, 44, K, bins, seed=21, pred_factor=1, gt_factor=2)
    got = run_kernel(sim, pred, gt, K, d, edges).cpu().numpy()
    want, _ = oracle(sim.numpy(), pred.numpy(), gt.numpy(), K, d, edges)
    assert np.array_equal(got, want) and want[-2] > 300 * 1000


def test_every_rank_sums_to_the_centres_without_ignored_labels():
    K, d, bins = 5, 2, 25
    edges = edges_of(bins)
    sim, pred, gt = make_inputs(2, 24, 20, K, bins, seed=7, ignore=False)
    assert not (gt == 255).any()
    got = run_kernel(sim, pred, gt, K, d, edges).cpu().numpy()
    want, ignored = oracle(sim.numpy(), pred.numpy(), gt.numpy(), K, d, edges)
    assert np.array_equal(got, want) and ignored == 0
    hist, rank, n, nc = split(got, K, bins)
    assert n == 2 * (24 - 8) * (20 - 8) and np.all(rank.sum(axis=1) == n) and hist.sum() == (K * K - 1) * nc


def test_ties_follow_the_tap_index():
    """every similarity equal: the order is the tap order, so rank r is non-centre tap r and its column is decided by that tap's label"""
    K, d, bins = 3, 1, 25
    edges = edges_of(bins)
    _, pred, gt = make_inputs(1, 24, 20, K, bins, seed=3, pred_factor=1, gt_factor=1)
    sim = torch.full((1, 9, 24, 20), 0.5)
    got = run_kernel(sim, pred, gt, K, d, edges).cpu().numpy()
    want, _ = oracle(sim.numpy(), pred.numpy(), gt.numpy(), K, d, edges)
    assert np.array_equal(got, want)
    g = gt[0].numpy().astype(np.int64)
    ctr = g[1:-1, 1:-1]
    _, rank, _, _ = split(got, K, bins)
    for r, k in enumerate([0, 1, 2, 3, 5, 6, 7, 8]):
        nb = g[k // 3:k // 3 + 22, k % 3:k % 3 + 18]
        live = (ctr != 255) & (nb != 255)
        assert rank[r, 0] == np.sum(live & (nb == ctr)) and rank[r, 1] == np.sum(live & (nb != ctr))


def test_launches_add_and_merge_combines():
    from pfst_amd import hip_ops as ops
    from pfst_amd.statistics import SimStatistics
    K, d, bins = 3, 2, 25
    edges = edges_of(bins)
    a = make_inputs(2, 24, 20, K, bins, seed=11)
    b = make_inputs(2, 24, 20, K, bins, seed=12)
    ca, cb = run_kernel(*a, K, d, edges), run_kernel(*b, K, d, edges)
    both = run_kernel(*b, K, d, edges, counters=run_kernel(*a, K, d, edges))
    assert torch.equal(both, ca + cb) and bool((ca != cb).any())
    # the accumulator: update = similarity map + pair statistics; merge adds
    g = torch.Generator().manual_seed(5)
    fa, fb = torch.randn(2, 8, 24, 20, generator=g).cuda(), torch.randn(2, 8, 24, 20, generator=g).cuda()
    one, two, ref = (SimStatistics(K, d, bins=bins, lo=-1.0, hi=1.0) for _ in range(3))
    one.update(fa, a[1].cuda(), a[2].cuda())
    two.update(fb, b[1].cuda(), b[2].cuda())
    ref.update(fa, a[1].cuda(), a[2].cuda()).update(fb, b[1].cuda(), b[2].cuda())
    assert one.merge(two).result() == ref.result() and ref.result()['n_centres'] > 0
    sim, _ = ops.sim_map(fa, d, 'cosine', 30.0, ksize=K)
    want, _ = oracle(sim.cpu().numpy(), a[1].numpy(), a[2].numpy(), K, d, one.edges_host)
    solo = SimStatistics(K, d, bins=bins, lo=-1.0, hi=1.0).update(fa, a[1].cuda(), a[2].cuda())
    assert np.array_equal(solo.counters.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import sim_statistics
    return sim_statistics


@pytest.fixture(scope='module')
def synthetic_run():
    """the seeded random EncoderDecoder of the Potsdam -> Vaihingen config and two synthetic 128 x 128 labelled tiles, built the way
    tools/sim_statistics.py --synthetic 2 builds them"""
    tool = _tool()
    args = tool.parse_args(['--synthetic', '2'])
    cfg = tool.load_config(args)
    model, data = tool.build_model_and_data(args, cfg, torch.device('cuda'))
    return tool, cfg, model, data


def test_collect_matches_the_oracle_on_the_models_own_features(synthetic_run):
    from pfst_amd import hip_ops as ops
    from pfst_amd.statistics import SimStatistics, collect_sim_statistics
    _, _, model, data = synthetic_run
    assert len(data) == 2 and data.gt_seg_map(0).shape == (128, 128)
    combos = [(f, K) for f in ('decoded', 2) for K in (3, 5)]
    specs = [(f, SimStatistics(K, 2, bins=25)) for f, K in combos]
    assert collect_sim_statistics(model, data, specs) == 2
    want = [np.zeros(s.counters.numel(), np.int64) for _, s in specs]
    for i in range(2):
        img = data[i]['img'][None].cuda()
        with torch.no_grad():
            out = model.eval_features(img)
            lab, logits = model.inference(img, None, rescale=False)
        assert sorted(out) == ['decoded_feats', 'feats', 'seg_logits'] and len(out['feats']) == 4
        assert out['decoded_feats'].shape == (1, 512, 16, 16) and out['feats'][2].shape == (1, 1024, 16, 16)
        assert torch.equal(out['seg_logits'], logits)                       # bit for bit the logits of `inference`
        pred = ops.argmax_nchw(out['seg_logits'])
        assert pred.shape == (1, 32, 32)
        for j, (f, K) in enumerate(combos):
            feat = out['decoded_feats'] if f == 'decoded' else out['feats'][f]
            sim, _ = ops.sim_map(feat.contiguous(), 2, 'cosine', 30.0, ksize=K)
            c, _ = oracle(sim.cpu().numpy(), pred.cpu().numpy(), data.gt_seg_map(i)[None], K, 2, specs[j][1].edges_host)
            want[j] += c
    for (f, s), w, (_, K) in zip(specs, want, combos):
        got = s.counters.cpu().numpy()
        print(f'{f} K {K}: centres {got[-2]}, correct {got[-1]}')
        assert np.array_equal(got, w)
        assert got[-2] == w[-2] > 0
        r = s.result()
        assert r['n_centres'] == int(w[-2]) and len(r['rank_purity']) == K * K - 1


def test_cli_synthetic_sweep_equals_collect_in_process(synthetic_run, tmp_path):
    from pfst_amd.statistics import SimStatistics, collect_sim_statistics
    tool, cfg, model, data = synthetic_run
    cmd = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'tools', 'sim_statistics.py'), '--synthetic', '2',
           '--kernel-size', '3', '5', '--dilation', '1', '2', '--out-dir', str(tmp_path)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    out = json.load(open(tmp_path / 'sim_statistics.json'))
    assert out['images'] == 2 and out['synthetic'] == 2 and len(out['results']) == 4
    assert 'purity' in done.stdout
    specs = [SimStatistics(K, d, bins=25) for K in (3, 5) for d in (1, 2)]
    collect_sim_statistics(model, data, specs, feature='decoded')
    for entry, s in zip(out['results'], specs):
        r = s.result()
        assert (entry['feature'], entry['kernel_size'], entry['dilation']) == ('decoded', s.ksize, s.dilation)
        for key in ('hist', 'rank', 'n_centres', 'n_correct_centres', 'hist_norm', 'rank_same', 'rank_purity', 'edges'):
            assert entry[key] == r[key], key
        assert entry['n_centres'] > 0
