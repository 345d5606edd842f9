"""Pseudo-feature statistics, the parts that need no GPU: the tables SimStatistics.result() derives from its integer counters, the defaults
read from the shipped configs, the bin-edge table, the command line's cross product of settings, and the C ABI of the two new entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import sim_statistics
    return sim_statistics


def test_result_tables_from_hand_written_counters():
    import torch
    from pfst_amd.statistics import CASES, SimStatistics
    st = SimStatistics(ksize=3, dilation=1, bins=4, lo=0.0, hi=1.0, device='cpu')
    assert st.counters.numel() == 4 * 6 + 2 * 8 + 2 and st.counters.dtype == torch.int64
    hist = [[1, 3, 0, 4, 7, 9],            # 1a: 8 in range, 7 below, 9 above
            [0, 0, 0, 0, 5, 0],            # 1b: nothing in range -> no normalised histogram
            [2, 0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0, 0]]
    rank = [[3, 1], [0, 0], [1, 3], [0, 4], [0, 0], [0, 0], [2, 2], [1, 0]]
    st.counters.copy_(torch.tensor(sum(hist, []) + sum(rank, []) + [11, 6]))
    r = st.result()
    assert r['kernel_size'] == 3 and r['dilation'] == 1 and r['bins'] == 4 and r['range'] == [0.0, 1.0] and r['sim_type'] == 'cosine'
    assert r['cases'] == list(CASES) == ['1a', '1b', '2b', '2a']
    assert r['hist'] == hist and r['rank'] == rank and r['n_centres'] == 11 and r['n_correct_centres'] == 6
    assert all(type(v) is int for row in r['hist'] + r['rank'] for v in row)
    assert r['edges'] == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert r['hist_norm'][0] == [1 / 8, 3 / 8, 0.0, 4 / 8]                       # out-of-range counts stay out of the normalisation
    assert r['hist_norm'][1] == [None] * 4 and r['hist_norm'][3] == [None] * 4     # empty denominator: None, not NaN
    assert r['hist_norm'][2] == [1.0, 0.0, 0.0, 0.0]
    assert r['rank_same'] == [3 / 4, None, 1 / 4, 0.0, None, None, 2 / 4, 1.0]
    assert r['rank_purity'] == [3 / 4, 3 / 4, 4 / 8, 4 / 12, 4 / 12, 4 / 12, 6 / 16, 7 / 17]
    import json
    assert json.loads(json.dumps(r)) == r                                         # plain Python all the way down
    empty = SimStatistics(ksize=5, dilation=2, bins=25, device='cpu').result()
    assert empty['rank_purity'] == [None] * 24 and empty['rank_same'] == [None] * 24 and empty['hist_norm'] == [[None] * 25] * 4


def test_merge_adds_counters_and_refuses_another_setting():
    import torch
    from pfst_amd.statistics import SimStatistics
    a, b = SimStatistics(3, 2, bins=5, device='cpu'), SimStatistics(3, 2, bins=5, device='cpu')
    a.counters += torch.arange(a.counters.numel())
    b.counters += 2
    a.merge(b)
    assert torch.equal(a.counters, torch.arange(a.counters.numel()) + 2)
    with pytest.raises(ValueError):
        a.merge(SimStatistics(3, 1, bins=5, device='cpu'))
    for bad in (dict(ksize=4), dict(dilation=0), dict(bins=0), dict(bins=257), dict(lo=1.0, hi=1.0), dict(sim_type='dot')):
        with pytest.raises(ValueError):
            SimStatistics(device='cpu', **bad)


@pytest.mark.parametrize('name,dilation', [('pfst_pots_irrg2vaih_irrg', 2), ('pfst_vaih_irrg2pots_irrg', 2), ('pfst_inria_da', 2),
                                           ('pfst_season_net_sp2fa', 1)])
def test_settings_from_the_shipped_configs(name, dilation, golden_dir):
    """use_decoded_feats=True, kernel 3, cosine everywhere; dilation 2 on the loss grid is 2 on the 1/8 decoded grid with downscale 0.5
    and 1 with SeasonNet's downscale 1 (the 1/4 loss grid holds the 1/8 features replicated 2 x 2): PFGSTLoss.forward's fd"""
    from test_config_dropin import reference_config
    from pfst_amd.statistics import settings_from_config
    cfg = reference_config(name, golden_dir)
    assert settings_from_config(cfg) == dict(feature='decoded', kernel_size=3, dilation=dilation, sim_type='cosine', sigma=30.0)


def test_settings_of_other_configs(golden_dir):
    from test_config_dropin import reference_config
    from pfst_amd.config import Config
    from pfst_amd.statistics import feature_dilation, settings_from_config
    assert settings_from_config(Config(dict(model=dict()))) == dict(feature='decoded', kernel_size=3, dilation=2, sim_type='cosine', sigma=30.0)
    cfg = reference_config('pfst_pots_irrg2vaih_irrg', golden_dir)
    cfg.merge_from_dict({'uda.use_decoded_feats': False})
    cfg.uda.aux_losses[0].update(feat_level=2, kernel_size=5, sim_type='gaussian', sigma=12, dilation=4)
    assert settings_from_config(cfg) == dict(feature=2, kernel_size=5, dilation=4, sim_type='gaussian', sigma=12.0)
    # level 0 is the 1/4 grid: finer than the 1/8 loss grid of downscale 0.5 (PFGSTLoss refuses it too); with downscale 1 it is the loss grid
    with pytest.raises(NotImplementedError):
        feature_dilation(cfg, 0, 2, 0.5)
    assert feature_dilation(cfg, 0, 2, 1) == 2 and feature_dilation(cfg, 3, 2, 1) == 1 and feature_dilation(cfg, 'decoded', 4, None) == 2
    with pytest.raises(NotImplementedError):
        feature_dilation(cfg, 'decoded', 3, 1)


@pytest.mark.parametrize('bins,lo,hi', [(25, 0.0, 1.0), (256, 0.0, 1.0), (25, -1.0, 1.0), (10, 0.5, 1.0), (7, 0.0, 0.3)])
def test_edges_are_linspace_rounded_to_float32(bins, lo, hi):
    from pfst_amd.statistics import SimStatistics, bin_edges
    e = bin_edges(bins, lo, hi)
    assert e.dtype == np.float32 and e.shape == (bins + 1,)
    assert np.array_equal(e, np.linspace(lo, hi, bins + 1).astype(np.float32))
    assert e[0] == np.float32(lo) and e[-1] == np.float32(hi) and np.all(np.diff(e) > 0)
    st = SimStatistics(3, 1, bins=bins, lo=lo, hi=hi, device='cpu')
    assert np.array_equal(st.edges.numpy(), e)


def test_cli_builds_the_cross_product_of_settings():
    tool = _tool()
    args = tool.parse_args(['--synthetic', '2', '--kernel-size', '3', '5', '--dilation', '1', '2'])
    cfg = tool.load_config(args)
    specs = tool.spec_settings(args, cfg)
    assert [(s['kernel_size'], s['dilation']) for s in specs] == [(3, 1), (3, 2), (5, 1), (5, 2)]
    assert all(s['feature'] == 'decoded' and s['sim_type'] == 'cosine' and s['bins'] == 25 and (s['lo'], s['hi']) == (0.0, 1.0) for s in specs)
    # nothing given: the config's own setting, once
    one = tool.spec_settings(tool.parse_args(['--synthetic', '1']), cfg)
    assert one == [dict(feature='decoded', kernel_size=3, dilation=2, sim_type='cosine', sigma=30.0, bins=25, lo=0.0, hi=1.0)]
    args = tool.parse_args(['cfg.py', 'ck.pth', '--feature', '2', '--kernel-size', '7', '--sim-type', 'gaussian', '--sigma', '5', '--bins', '50',
                            '--range', '-1', '1', '--split', 'val', '--revise-checkpoint-key', '--max-images', '3', '--plot'])
    assert args.split == 'val' and args.revise_checkpoint_key and args.max_images == 3 and args.plot
    assert tool.spec_settings(args, cfg) == [dict(feature=2, kernel_size=7, dilation=2, sim_type='gaussian', sigma=5.0, bins=50, lo=-1.0, hi=1.0)]
    for bad in ([], ['cfg.py'], ['--synthetic', '0'], ['--synthetic', '1', '--kernel-size', '4'], ['--synthetic', '1', '--bins', '300'],
                ['--synthetic', '1', '--range', '1', '0'], ['--synthetic', '1', '--dilation', '0']):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_header_declares_and_library_exports_the_entry_points():
    from pfst_amd import _lib
    decls = _lib.parse_header()
    assert [a[1] for a in decls['pfst_sim_pair_stats'][1]] == ['sim', 'pred', 'gt', 'N', 'H', 'W', 'Hp', 'Wp', 'Hg', 'Wg', 'ksize', 'dil', 'edges',
                                                               'bins', 'counters', 'stream']
    assert [a[0] for a in decls['pfst_sim_pair_stats'][1]] == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 9 + [ctypes.c_void_p, ctypes.c_int,
                                                                                                          ctypes.c_void_p, ctypes.c_void_p]
    assert [a[1] for a in decls['pfst_sim_pair_stats_counters'][1]] == ['ksize', 'bins']
    assert os.path.exists(_lib.LIB_PATH), 'run python -m pfst_amd.build'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'pfst_sim_pair_stats') and hasattr(raw, 'pfst_sim_pair_stats_counters')
    L = _lib.lib()
    # hist[4][bins + 2] + rank[K^2 - 1][2] + the two centre counts; bad sizes are refused
    assert L.pfst_sim_pair_stats_counters(3, 25) == 4 * 27 + 16 + 2 and L.pfst_sim_pair_stats_counters(7, 256) == 4 * 258 + 96 + 2
    assert L.pfst_sim_pair_stats_counters(4, 25) == -1 and L.pfst_sim_pair_stats_counters(3, 0) == -1
    assert L.pfst_sim_pair_stats_counters(3, 257) == -1
    # arguments are checked on the host before any launch
    assert L.pfst_sim_pair_stats(None, None, None, 1, 8, 8, 8, 8, 8, 8, 3, 1, None, 25, None, None) == -1
    assert b'pfgst_loss.hip' in L.pfst_last_error()
    from pfst_amd import hip_ops as ops
    assert ops.sim_pair_stats_counters(5, 10) == 4 * 12 + 48 + 2
    with pytest.raises(ValueError):
        ops.sim_pair_stats_counters(3, 1000)
