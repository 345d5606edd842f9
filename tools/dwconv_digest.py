"""Depthwise 3x3 family (csrc/dwconv.hip) on seeded inputs: one line per output -- case, output, SHA-256 of its bytes.  Two builds of the library
compute the same thing exactly when their outputs are identical line for line:
    PFST_HIP_LIB=<other libpfst_hip.so> python tools/dwconv_digest.py > a.txt;  python tools/dwconv_digest.py > b.txt;  diff a.txt b.txt
Weight gradients are printed in deterministic mode only (the order of the atomic adds is free otherwise); every backward runs in both modes."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pfst_amd import hip_ops as ops

DEV = 'cuda'
NC = [(1, 1), (1, 7), (3, 6)]
# (dil, H, W): whole planes (row_taps_d1, aligned, unaligned taps, 8 x 512 quads), strips (two, clamped to one row, scalar, several, more quads than the
# weight-gradient kernel keeps in registers), W % 4 != 0
SHAPES = [(1, 16, 20), (12, 32, 32), (3, 24, 32), (12, 128, 128), (1, 136, 128), (12, 40, 512), (16, 40, 510), (3, 130, 132), (1, 2, 16400), (9, 7, 9)]
MULTI = [(32, 32, (12, 24, 36)), (24, 40, (4, 8)), (16, 16, (36,))]


def rnd(seed, *shape, shift=0.0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(DEV)


def emit(case, name, t):
    torch.cuda.synchronize()
    print(case, name, hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest(), flush=True)


def bn_of(pre, seed):
    """gamma, beta, and in deterministic mode (fixed-order sums) the statistics of pre"""
    c = pre.shape[1]
    gamma, beta = rnd(seed, c).abs() + 0.5, rnd(seed + 1, c, scale=0.3)
    ops.set_deterministic(True)
    mean, invstd, coef = ops.bn_stats(pre, gamma=gamma, beta=beta)
    return gamma, beta, mean, invstd, coef


def bn_rec(dyo, pre, seed):
    gamma, beta, mean, invstd, _ = bn_of(pre, seed)
    return ops.bn_backward_sums(dyo, pre, mean, invstd, gamma, beta, None, None)


def single(n, c, dil, h, w):
    case = f'n{n}c{c}d{dil}h{h}w{w}'
    x, wt, dy = rnd(1, n, c, h, w, shift=1.0), rnd(2, c, 1, 3, 3, shift=0.25), rnd(3, n, c, h, w)
    y, st, slots = ops.dwconv(x, wt, dil, want_stats=True, want_minmax=True)
    emit(case, 'fwd.y', y)
    emit(case, 'fwd.partials', st[:4 * c * slots])
    pre = rnd(11, n, c, h, w, scale=2.0)
    coef = bn_of(pre, 12)[4]
    emit(case, 'fwd.bnl.y', ops.dwconv(pre, wt, dil, bnl=coef))
    emit(case, 'dgrad', ops.dwconv(dy, wt, dil, flip=True))
    emit(case, 'dgrad.acc', ops.dwconv(dy, wt, dil, flip=True, out=x.clone(), accumulate=True))
    dyo = rnd(16, n, c, h, w)
    rec = bn_rec(dyo, y, 14)
    for det in (False, True):
        ops.set_deterministic(det)
        for name, xin, g, kw in (('bwd', x, dy, {}), ('bwd.acc', x, dy, dict(accumulate=True)), ('bwd.bnl', pre, dy, dict(bnl=coef)),
                                 ('bwd.bnb', x, dyo, dict(bnb=(y, rec)))):
            dw, dx = torch.zeros_like(wt), x.clone()
            ops.dwconv_bwd_(dw, xin, g, wt, dil, dx, **kw)
            emit(case, f'{name}.det{int(det)}.dx', dx)
            if det:
                emit(case, f'{name}.det1.dw', dw)
        dw = ops.dwconv_wgrad_(torch.zeros_like(wt), x, dy, dil)
        if det:
            emit(case, 'wgrad.det1.dw', dw)
    ops.set_deterministic(False)


def multi(n, c, h, w, dils):
    case = f'multi.n{n}c{c}h{h}w{w}d' + '-'.join(map(str, dils))
    k = len(dils)
    x, mg = rnd(1, n, c, h, w, shift=1.0), rnd(20, n, c)
    ws, dys = [rnd(2 + i, c, 1, 3, 3, shift=0.25) for i in range(k)], [rnd(7 + i, n, c, h, w) for i in range(k)]
    for i, (y, _, _) in enumerate(ops.dwconv_multi(x, ws, list(dils))):
        emit(case, f'fwd.y{i}', y)
    res, mean = ops.dwconv_multi(x, ws, list(dils), want_stats=True, want_minmax=True, want_mean=True)
    emit(case, 'fwd.stats.mean', mean)
    for i, (y, st, slots) in enumerate(res):
        emit(case, f'fwd.stats.y{i}', y)
        emit(case, f'fwd.stats.partials{i}', st[:4 * c * slots])
    pres = [r[0] for r in res]
    recs = [bn_rec(dys[i], pres[i], 30 + 2 * i) for i in range(k)]
    for det in (False, True):
        ops.set_deterministic(det)
        for name, kw in (('bwd', {}), ('bwd.acc', dict(accumulate=True)), ('bwd.mean', dict(mean_grad=mg)),
                         ('bwd.bnb', dict(bnb=list(zip(pres, recs)))), ('bwd.bnb.mean', dict(bnb=list(zip(pres, recs)), mean_grad=mg))):
            dws, dx = [torch.zeros_like(t) for t in ws], x.clone()
            ops.dwconv_multi_bwd_(dws, x, dys, ws, list(dils), dx, **kw)
            emit(case, f'{name}.det{int(det)}.dx', dx)
            if det:
                for i in range(k):
                    emit(case, f'{name}.det1.dw{i}', dws[i])
    ops.set_deterministic(False)


if __name__ == '__main__':
    for n, c in NC:
        for dil, h, w in SHAPES:
            single(n, c, dil, h, w)
        for h, w, dils in MULTI:
            multi(n, c, h, w, dils)
