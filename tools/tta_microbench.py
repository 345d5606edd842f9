"""Multi-scale + flip test-time augmentation at b = 1, a 1024^2 tile, C = 6, the reference's six ratios with flip (12 views), timed on
device events (median of --reps):
  - the whole aug_test per image (paired-flip forwards: one batch-2 forward per scale), and the per-view path (12 batch-1 forwards);
  - the share of the forwards in it;
  - per view at each scale, the fused pfst_tta_accumulate against the chain it replaces (resize, resize, softmax, flip, axpy),
    with the bytes of acc's read-modify-write.

    python tools/tta_microbench.py [--reps N]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        t.append(s.elapsed_time(e))
    t.sort()
    return t[len(t) // 2]                       # median, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    import torch.nn.functional as F
    import pfst_amd  # noqa: F401
    from helpers import seeded_pfgst_state, uda_cfg
    from oracle import pfst_oracle as O
    from pfst_amd import hip_ops as ops
    from pfst_amd.registry import UDA
    model = UDA.build(uda_cfg())
    both, _, _ = seeded_pfgst_state(O, 9)
    model.load_state_dict(both, strict=False)
    model.cuda()
    seg = model.get_model()
    S, C = 1024, 6
    ratios = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]
    g = torch.Generator(device='cuda').manual_seed(0)
    base = torch.randn(1, 3, S, S, device='cuda', generator=g)
    imgs, metas = [], []
    for si, r in enumerate(ratios):
        s = int(S * r)
        plain = base if s == S else F.interpolate(base, size=(s, s), mode='bilinear', align_corners=False).contiguous()
        for flip in (False, True):
            imgs.append(plain.flip(3).contiguous() if flip else plain)
            metas.append([dict(ori_shape=(S, S, 3), flip=flip, flip_direction='horizontal', scale_index=si, flip_permutes=True)])
    per_view = [[dict(m[0], flip_permutes=False)] for m in metas]
    res = dict(b=1, size=S, classes=C, ratios=ratios, views=len(imgs))
    with torch.no_grad():
        res['aug_test_ms'] = timeit(lambda: seg.aug_test_labels(imgs, metas), args.reps)
        res['aug_test_per_view_ms'] = timeit(lambda: seg.aug_test_labels(imgs, per_view), args.reps)
        pairs = [torch.cat([imgs[2 * i], imgs[2 * i + 1]], 0) for i in range(len(ratios))]
        res['forwards_ms'] = timeit(lambda: [seg._tta_forward(p) for p in pairs], args.reps)
        res['forward_share'] = res['forwards_ms'] / res['aug_test_ms']
        acc = torch.zeros(1, C, S, S, device='cuda')
        views = []
        for i, r in enumerate(ratios):
            src, mid = seg._tta_forward(imgs[2 * i])
            src = src.contiguous()

            def chain():
                p = ops.resize_bilinear(src, mid)
                if tuple(mid) != (S, S):
                    p = ops.resize_bilinear(p, (S, S))
                ops.axpy_(acc, ops.flip_planes(ops.softmax_nchw(p), horizontal=True))
            fused_ms = timeit(lambda: ops.tta_accumulate_(acc, src, mid, True, False), args.reps)
            chain_ms = timeit(chain, args.reps)
            rmw = 2 * acc.numel() * 4
            views.append(dict(ratio=r, input=list(mid), src=list(src.shape[2:]), fused_us=1e3 * fused_ms, chain_us=1e3 * chain_ms,
                              fused_rmw_TBps=rmw / (fused_ms * 1e-3) / 1e12))
        res['per_view'] = views
    print(json.dumps(res))


if __name__ == '__main__':
    main()
