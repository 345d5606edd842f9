#!/usr/bin/env python3
"""What the pseudo-feature statistics cost, in one process on one box:
  1. at the product shape, 1 x 512 x 128 x 128 decoded features of a 1024^2 tile: one EncoderDecoder.eval_features forward, and per kernel
     size 3 / 5 / 7 (dilation 2) one similarity-map launch and one pfst_sim_pair_stats launch -- the yardstick of the statistics pass is the
     similarity map it follows (it reads the K^2 floats per pixel that launch wrote and writes counters only);
  2. per image at 1024^2: collect_sim_statistics (the work of tools/sim_statistics.py) with the config's setting and with the 3 x 2 sweep,
     against the evaluation loop of tools/test.py (inference + confusion statistics) on the same tiles.
Seeded random model, seeded synthetic tiles; device events around warmed-up launches, minimum and median of the repeats."""
import argparse
import os
import statistics as pystat
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--tiles', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    import torch
    import sim_statistics as tool
    from pfst_amd import hip_ops as ops
    from pfst_amd.evaluation import AreaAccumulator
    from pfst_amd.statistics import SimStatistics, collect_sim_statistics
    assert torch.cuda.is_available(), 'a measurement needs the GPU'
    dev = torch.device('cuda')
    args = tool.parse_args(['--synthetic', str(a.tiles), '--synthetic-size', str(a.size)])
    cfg = tool.load_config(args)
    model, data = tool.build_model_and_data(args, cfg, dev)

    def timed(fn, reps=a.reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            ts.append(s.elapsed_time(e) * 1e3)
        return min(ts), pystat.median(ts)

    img = data[0]['img'][None].to(dev)
    with torch.no_grad():
        out = model.eval_features(img)
        lo, md = timed(lambda: model.eval_features(img), reps=10)
    feat = out['decoded_feats'].contiguous()
    print(f'eval_features forward, 1 x 3 x {a.size}^2: {lo:9.1f} us min {md:9.1f} us median', flush=True)
    pred = ops.argmax_nchw(out['seg_logits'])
    gt = torch.from_numpy(data.gt_seg_map(0))[None].to(dev)
    print(f'features {tuple(feat.shape)}, pred {tuple(pred.shape)}, gt {tuple(gt.shape)}')
    for K in (3, 5, 7):
        st = SimStatistics(K, 2, bins=25, device=dev)
        sim, _ = ops.sim_map(feat, 2, 'cosine', 30.0, ksize=K)
        m_lo, m_md = timed(lambda: ops.sim_map(feat, 2, 'cosine', 30.0, ksize=K))
        s_lo, s_md = timed(lambda: ops.sim_pair_stats(sim, pred, gt, 2, K, st.edges, st.counters))
        r = st.result()
        print(f'K {K} d 2: sim_map {m_lo:8.1f} us min {m_md:8.1f} median | sim_pair_stats {s_lo:8.1f} us min {s_md:8.1f} median '
              f'({sim.numel() * 4 / s_lo / 1e3:6.1f} GB/s of similarities; centres per launch {r["n_centres"] // (a.reps + 3)})', flush=True)

    def wall(fn, reps=3):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / len(data))
        return min(ts)

    def evaluate():                                   # the loop of pfst_amd.evaluation.build_eval_fn (tools/test.py) on these tiles
        acc = AreaAccumulator(cfg.model.decode_head.num_classes, 255, dev)
        with torch.no_grad():
            for i in range(len(data)):
                p8, _ = model.inference(data[i]['img'][None].to(dev), [data[i]['img_metas']], rescale=True)
                g = torch.from_numpy(data.gt_seg_map(i)).to(dev)
                acc.update(p8.reshape(g.shape), g)
        return acc.areas()

    def collect(combos):
        specs = [SimStatistics(K, d, bins=25, device=dev) for K, d in combos]
        collect_sim_statistics(model, data, specs, feature='decoded')
        return [s.result() for s in specs]

    t_eval = wall(evaluate)
    t_one = wall(lambda: collect([(3, 2)]))
    t_sweep = wall(lambda: collect([(K, d) for K in (3, 5, 7) for d in (1, 2)]))
    print(f'per image at {a.size}^2 ({len(data)} tiles, host clock around a synchronise): evaluation loop {t_eval * 1e3:7.2f} ms | statistics, '
          f'K 3 d 2 {t_one * 1e3:7.2f} ms | statistics, sweep of 6 settings {t_sweep * 1e3:7.2f} ms')


if __name__ == '__main__':
    main()
