#!/usr/bin/env python3
"""Pseudo-feature statistics of a checkpoint over a labelled split: the similarity histograms (cases 1a / 1b / 2a / 2b) and the local-rank
table the reference's PlotStatisticsHook collects (rsiseg/core/hook/plot_statistics_hook.py, `sim_feat_cfg` in configs/pfst/*.py:73-81) --
the evidence for choosing PFGSTLoss's feat_level, sim_type, kernel_size, dilation and top_k for a pair of domains.

  python tools/sim_statistics.py CONFIG CHECKPOINT [--split test|val] [--revise-checkpoint-key] [--feature decoded|0|1|2|3]
      [--kernel-size K [K ...]] [--dilation D [D ...]] [--sim-type cosine|gaussian] [--sigma S] [--bins 25] [--range LO HI]
      [--max-images N] [--out-dir DIR] [--plot] [--gpu-id 0] [--cfg-options ...]

Defaults come from the config's own `uda` section (pfst_amd.statistics.settings_from_config): the feature map, kernel size, similarity type
and dilation the config trains with; --dilation is in pixels of the feature grid.  Several --kernel-size / --dilation values give every
combination from ONE pass over the data (one forward per image).  Writes `<out-dir>/sim_statistics.json`, one entry per combination (integer
counters, the normalised histograms, the per-rank share of same-class neighbours and its cumulative form: the purity of a top_k positive
set), and prints the purity table.  --plot adds the reference's three bar charts per entry when matplotlib is installed.

`--synthetic N` needs neither a checkpoint nor data (nor a config: the Potsdam -> Vaihingen one is built in): a seeded random model on N seeded
synthetic labelled tiles of --synthetic-size pixels."""
import argparse
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SYNTHETIC_WORKLOAD = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='pfst_amd: similarity histograms and local-rank tables of pseudo-features')
    p.add_argument('config', nargs='?')
    p.add_argument('checkpoint', nargs='?')
    p.add_argument('--split', default='test', choices=['test', 'val'])
    p.add_argument('--revise-checkpoint-key', action='store_true')
    p.add_argument('--feature', default=None, choices=['decoded', '0', '1', '2', '3'], help='the decoded features or a backbone level')
    p.add_argument('--kernel-size', type=int, nargs='+', default=None, choices=[3, 5, 7])
    p.add_argument('--dilation', type=int, nargs='+', default=None, help='in pixels of the feature grid')
    p.add_argument('--sim-type', default=None, choices=['cosine', 'gaussian'])
    p.add_argument('--sigma', type=float, default=None)
    p.add_argument('--bins', type=int, default=25)
    p.add_argument('--range', type=float, nargs=2, default=[0.0, 1.0], metavar=('LO', 'HI'))
    p.add_argument('--max-images', type=int, default=None)
    p.add_argument('--out-dir', default='.')
    p.add_argument('--plot', action='store_true', help='also write the bar charts (needs matplotlib)')
    p.add_argument('--synthetic', type=int, default=None, metavar='N', help='a seeded random model on N seeded synthetic labelled tiles')
    p.add_argument('--synthetic-size', type=int, default=128)
    p.add_argument('--gpu-id', type=int, default=0)
    p.add_argument('--cfg-options', nargs='+')
    args = p.parse_args(argv)
    if args.synthetic is None and (args.config is None or args.checkpoint is None):
        p.error('CONFIG and CHECKPOINT are required without --synthetic')
    if args.synthetic is not None and args.synthetic < 1:
        p.error('--synthetic needs at least one tile')
    if not 1 <= args.bins <= 256:
        p.error('--bins must lie in 1 .. 256')
    if not args.range[0] < args.range[1]:
        p.error('--range LO HI needs LO < HI')
    if args.dilation is not None and min(args.dilation) < 1:
        p.error('--dilation must be at least 1')
    if args.sigma is not None and args.sigma <= 0:
        p.error('--sigma must be positive')
    return args


def load_config(args):
    """the config file with --cfg-options merged; without a file (--synthetic) the built-in Potsdam -> Vaihingen workload"""
    from pfst_amd.config import Config, parse_cfg_options
    if args.config is not None:
        cfg = Config.fromfile(args.config)
    else:
        from pfst_amd.presets import workload_cfg
        uda, _ = workload_cfg(SYNTHETIC_WORKLOAD)
        cfg = Config(dict(model=uda.pop('model'), uda=uda))
    if args.cfg_options:
        cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    return cfg


def spec_settings(args, cfg):
    """-> the list of settings dicts (feature, kernel_size, dilation, sim_type, sigma, bins, lo, hi), one per --kernel-size x --dilation
    combination (kernel sizes outermost), every value not given on the command line from the config"""
    from pfst_amd.statistics import settings_from_config
    d = settings_from_config(cfg)
    feature = d['feature'] if args.feature is None else ('decoded' if args.feature == 'decoded' else int(args.feature))
    ksizes = args.kernel_size or [d['kernel_size']]
    dils = args.dilation or [d['dilation']]
    common = dict(sim_type=args.sim_type or d['sim_type'], sigma=d['sigma'] if args.sigma is None else args.sigma, bins=args.bins,
                  lo=args.range[0], hi=args.range[1])
    return [dict(feature=feature, kernel_size=k, dilation=dl, **common) for k, dl in itertools.product(ksizes, dils)]


def build_model_and_data(args, cfg, dev):
    from pfst_amd.apis import init_segmentor
    if args.synthetic is not None:
        import torch
        from pfst_amd.statistics import SyntheticTiles
        from pfst_amd.synthetic import fill_state_dict
        torch.manual_seed(0)
        model = init_segmentor(cfg, None, device='cpu')
        fill_state_dict(model.state_dict(), 0)
        model.to(dev)
        data = SyntheticTiles(args.synthetic, args.synthetic_size, cfg.model.decode_head.num_classes, cfg.model.backbone.get('in_channels', 3))
        return model, data
    from pfst_amd.data import TileFolder
    model = init_segmentor(cfg, args.checkpoint, device=dev, revise_checkpoint_key=args.revise_checkpoint_key)
    return model, TileFolder(cfg.data[args.split], test_mode=True)


def write_plots(results, out_dir):
    """the three bar charts of the reference per entry: the histograms of cases 1a / 1b, of cases 2a / 2b, and the local-rank table with
    each column normalised to 1.  -> the files written, or None when matplotlib is not installed"""
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    red, blue = (228 / 255.0, 26 / 255.0, 28 / 255.0, 0.8), (55 / 255.0, 126 / 255.0, 184 / 255.0, 0.8)
    nz = lambda row: [0.0 if v is None else v for v in row]
    written = []
    for r in results:
        tag = f"{r['feature']}_k{r['kernel_size']}_d{r['dilation']}_{r['sim_type']}"
        mids = [(a + b) / 2 for a, b in zip(r['edges'][:-1], r['edges'][1:])]
        width = (r['edges'][-1] - r['edges'][0]) / r['bins']
        for name, (ia, la), (ib, lb) in (('sim_hist_true', (0, 'Case 1a'), (1, 'Case 1b')), ('sim_hist_false', (3, 'Case 2a'), (2, 'Case 2b'))):
            fig, ax = plt.subplots(figsize=(6, 3))
            ax.bar(mids, nz(r['hist_norm'][ia]), width, color=red, label=la)
            ax.bar(mids, nz(r['hist_norm'][ib]), width, color=blue, label=lb)
            ax.set(xlabel='Similarity', ylabel='Frequency')
            ax.legend()
            fig.tight_layout()
            written.append(os.path.join(out_dir, f'{name}_{tag}.pdf'))
            fig.savefig(written[-1])
            plt.close(fig)
        cols = [[row[c] for row in r['rank']] for c in (0, 1)]
        cols = [[v / sum(col) if sum(col) else 0.0 for v in col] for col in cols]
        xs = list(range(1, len(r['rank']) + 1))
        fig, ax = plt.subplots(figsize=(6, 3))
        ax.bar([x - 0.2 for x in xs], cols[0], 0.4, color=red, label='Case 1a & 2a')
        ax.bar([x + 0.2 for x in xs], cols[1], 0.4, color=blue, label='Case 1b & 2b')
        ax.set(xlabel='Local Rank', ylabel='Frequency')
        ax.legend()
        fig.tight_layout()
        written.append(os.path.join(out_dir, f'local_rank_{tag}.pdf'))
        fig.savefig(written[-1])
        plt.close(fig)
    return written


def main(argv=None):
    args = parse_args(argv)
    import torch
    import pfst_amd  # noqa: F401
    from pfst_amd.statistics import SimStatistics, collect_sim_statistics, purity_table
    cfg = load_config(args)
    settings = spec_settings(args, cfg)
    torch.cuda.set_device(args.gpu_id)
    dev = torch.device('cuda', args.gpu_id)
    model, data = build_model_and_data(args, cfg, dev)
    specs = [(s['feature'], SimStatistics(s['kernel_size'], s['dilation'], s['sim_type'], s['sigma'], s['bins'], s['lo'], s['hi'], dev))
             for s in settings]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    images = collect_sim_statistics(model, data, specs, max_images=args.max_images)
    results = [dict(feature=f, **st.result()) for f, st in specs]                # the reads end the queued work
    seconds = time.perf_counter() - t0
    os.makedirs(args.out_dir, exist_ok=True)
    out = dict(config=args.config, checkpoint=args.checkpoint, split=None if args.synthetic is not None else args.split,
               synthetic=args.synthetic, images=images, seconds=seconds, seconds_per_image=seconds / max(images, 1), results=results)
    with open(os.path.join(args.out_dir, 'sim_statistics.json'), 'w') as f:
        json.dump(out, f, indent=1)
    print(purity_table(results))
    print(f'{images} images, {seconds / max(images, 1):.3f} s per image -> {os.path.join(args.out_dir, "sim_statistics.json")}')
    if args.plot:
        files = write_plots(results, args.out_dir)
        print('matplotlib is not installed: no charts written' if files is None else f'{len(files)} charts written')
    return out


if __name__ == '__main__':
    main()
