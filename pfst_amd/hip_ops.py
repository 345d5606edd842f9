"""Thin torch-tensor front end of the C ABI (include/pfst_hip.h).

Every function checks device / dtype / layout on the host (a wrong shape must never reach a kernel),
passes raw device pointers + the current HIP stream, and returns torch tensors it allocated.
There is NO fallback: a missing libpfst_hip.so or a CPU tensor raises.
Tensors may be channel slices of a bigger NCHW tensor (batch stride != C*H*W)."""
import ctypes
import os

import torch

from ._lib import call, lib

F32, U8, I64, F64, I32 = torch.float32, torch.uint8, torch.int64, torch.float64, torch.int32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk(t, dtype=F32, nd=None):
    if not t.is_cuda:
        raise RuntimeError('pfst_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'expected {dtype}, got {t.dtype}')
    if nd is not None and t.dim() != nd:
        raise ValueError(f'expected {nd}-d tensor, got shape {tuple(t.shape)}')
    return t


def _bs(t):
    """batch stride of an NCHW tensor whose (C,H,W) part is dense."""
    _chk(t, F32, 4)
    n, c, h, w = t.shape
    if w > 1 and t.stride(3) != 1 or (h > 1 and t.stride(2) != w) or (c > 1 and t.stride(1) != h * w):
        raise ValueError(f'tensor is not a dense-plane NCHW view: shape {tuple(t.shape)} strides {t.stride()}')
    return t.stride(0) if n > 1 else max(t.stride(0), c * h * w)


def _dense(t, dtype=F32):
    _chk(t, dtype)
    if not t.is_contiguous():
        raise ValueError('tensor must be contiguous')
    return t


def _p(t):
    return 0 if t is None else t.data_ptr()


# ---------------------------------------------------------------- utilities
def set_deterministic(on=True):
    """pfst_set_deterministic: sums that are normally completed by atomic adds of several workgroups (split-K weight gradients, BatchNorm-backward
    reductions, depthwise weight gradients, bias gradients, PFGSTLoss source statistics) are formed in a fixed order -- per-workgroup (per grid
    slice) partials in a scratch + an ordered reduction; same launch shapes.  The gradient arena of a step is then bit-identical run to run and for
    any stream schedule (tests/test_deterministic_gpu.py); the b = 8 x 1024^2 step is about 3 % slower (tools/det_cost.py).  What the reference's `--deterministic`
    (cudnn.deterministic = True, rsiseg/apis/train.py:63-66) asks for."""
    call('pfst_set_deterministic', int(bool(on)))


def is_deterministic():
    return bool(lib().pfst_get_deterministic())


_h2d_stage = {}
_h2d_const = {}


def h2d_small(t_cpu, dev, tag):
    """a small per-step host tensor (augmentation parameters, class choices) to the device WITHOUT the stream synchronisation a pageable
    copy implies (`.to(dev)` of pageable memory makes the host wait for everything queued on the stream -- the host then starts the next
    pass with no lead over the device): staged through a pinned buffer cached per (tag, shape, dtype, device), copied asynchronously.  An event
    recorded behind each copy guards the buffer: the next call with the same key rewrites it only once that copy has run.  In the train step
    a buffer is reused one step later at the earliest, with the step's blocking read of its log values in between -- the event has long
    completed, the query returns at once and nothing waits; only a caller that reuses a key while its stream is still busy blocks, for that
    one copy"""
    key = (tag, tuple(t_cpu.shape), t_cpu.dtype, str(dev))
    ent = _h2d_stage.get(key)
    if ent is None:
        ent = _h2d_stage[key] = (torch.empty(t_cpu.shape, dtype=t_cpu.dtype, pin_memory=True), torch.cuda.Event())
    st, evt = ent
    if not evt.query():                  # (an event never recorded counts as complete)
        evt.synchronize()
    st.copy_(t_cpu)
    out = st.to(dev, non_blocking=True)
    evt.record(torch.cuda.current_stream(dev))
    return out


def const_tensor(values, dev, dtype=F32):
    """a device tensor of a few host constants (normalisation mean / std ...), built once per (values, device)"""
    key = (tuple(float(v) for v in values), str(dev), dtype)
    t = _h2d_const.get(key)
    if t is None:
        t = _h2d_const[key] = torch.tensor(list(values), dtype=dtype, device=dev)
    return t


def fill_(t, value):
    _dense(t)
    call('pfst_fill_f32', t.data_ptr(), t.numel(), float(value), _stream())
    return t


def axpy_(y, x, alpha=1.0):
    _dense(y), _dense(x)
    assert y.numel() == x.numel()
    call('pfst_axpy_f32', y.data_ptr(), x.data_ptr(), float(alpha), y.numel(), _stream())
    return y


def to_u8(lab):
    if lab.dtype == U8:
        return _dense(lab, U8)
    _dense(lab, I64)
    out = torch.empty(lab.shape, dtype=U8, device=lab.device)
    call('pfst_i64_to_u8', lab.data_ptr(), out.data_ptr(), lab.numel(), _stream())
    return out


def to_i64(lab):
    _dense(lab, U8)
    out = torch.empty(lab.shape, dtype=I64, device=lab.device)
    call('pfst_u8_to_i64', lab.data_ptr(), out.data_ptr(), lab.numel(), _stream())
    return out


# ---------------------------------------------------------------- dense conv
def conv_out_size(hi, k, stride, dil, pad):
    return (hi + 2 * pad - (k - 1) * dil - 1) // stride + 1


def _pack_outs(w, want_fprop, want_dgrad, out_f, out_d, shape_f, shape_d=None, dtype=F32):
    """the (forward, data-gradient) images of a weight-packing call: None where the direction is not wanted, else the caller's buffer
    (checked: an image of another size or type must not reach the kernel) or a fresh one"""
    def image(want, out, shape):
        if not want:
            return None
        if out is None:
            return torch.empty(shape, dtype=dtype, device=w.device)
        n = 1
        for s in shape:
            n *= s
        assert _dense(out, dtype).numel() == n, (tuple(out.shape), shape)
        return out
    return image(want_fprop, out_f, shape_f), image(want_dgrad, out_d, shape_f if shape_d is None else shape_d)


def pack_weight(w, want_fprop=True, want_dgrad=True, out_f=None, out_d=None):
    """w [Cout][Cin][k][k] -> K-major packings used by the implicit GEMM."""
    _dense(w)
    co, ci, kh, kw = w.shape
    assert kh == kw and kh in (1, 3)
    wf, wd = _pack_outs(w, want_fprop, want_dgrad, out_f, out_d, (kh * kw * ci, co), (kh * kw * co, ci))
    call('pfst_conv_pack_weight', w.data_ptr(), _p(wf), _p(wd), co, ci, kh * kw, _stream())
    return wf, wd


_scratch_cache = {}


def _scratch(dev, tag, n, floor=0, dtype=F32):
    """per-(device, stream, tag) scratch of at least n elements, consumed on the same stream: kept while it is large enough, else
    replaced by one of max(n, floor) elements.  Tags: 'stats' the conv / depthwise / Winograd epilogues' BN partials (read by
    bn_finalize_partials), ('multi', i) the same per branch of a multi-branch launch (all alive until their statistics are finalised),
    'V' 'M' 'U' 'Pf' 'Pd' the transform-domain tensors, 'bn' the fp64 sums of the BatchNorm kernels"""
    key = (dev, torch.cuda.current_stream().cuda_stream, tag)
    t = _scratch_cache.get(key)
    if t is None or t.numel() < n:
        t = _scratch_cache[key] = torch.empty(max(n, floor), dtype=dtype, device=dev)
    return t


_STATS_FLOOR = 1 << 20       # floats of a 'stats' scratch at least: every shape of the network fits, one allocation per stream


def conv_stats_slots(n, cout, ho, wo):
    return n * lib().pfst_conv_stats_slots(cout, ho, wo)


def bn_finalize_partials(stats, slots, c, count, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, gamma=None, beta=None,
                         predict_amax=None, relu=True, coef_out=None):
    """gamma / beta given: also returns coef [C,4] = (mean, invstd, sc, sh), the record the fused BatchNorm-backward sums read.
    predict_amax: a zeroed slot group (amax_slots); `stats` then carries the producer's (minimum, maximum) partials behind the sums
    (conv_fprop_f16x3(want_minmax=True)) and the group receives max |[relu](bn(x))| -- what bn_apply(amax=...) would publish, known before
    (or without) the normalised tensor being written"""
    mean = torch.empty(c, device=stats.device)
    invstd = torch.empty(c, device=stats.device)
    coef = torch.empty(c, 4, device=stats.device) if gamma is not None else None
    if coef_out is not None:                 # rows of a concat buffer's coefficient table (engine.Var.coef_table)
        assert gamma is not None and tuple(coef_out.shape) == (c, 4) and coef_out.is_contiguous()
        coef = coef_out
    mm = 0
    if predict_amax is not None:
        assert gamma is not None and stats.numel() >= 4 * c * slots
        mm = stats.data_ptr() + 4 * 2 * c * slots
    call('pfst_bn_finalize_partials', stats.data_ptr(), slots, c, float(count), mean.data_ptr(), invstd.data_ptr(),
         _p(running_mean), _p(running_var), momentum, eps, _p(gamma), _p(beta), _p(coef), mm, int(relu), _p(predict_amax), _stream())
    return (mean, invstd, coef) if gamma is not None else (mean, invstd)


class _BnbFuseStruct(ctypes.Structure):           # pfst_bnb_fuse_t (include/pfst_hip.h)
    _fields_ = [('x', ctypes.c_void_p), ('x_bs', ctypes.c_longlong), ('y', ctypes.c_void_p), ('y_bs', ctypes.c_longlong),
                ('coef', ctypes.c_void_p), ('partials', ctypes.c_void_p), ('relu', ctypes.c_int), ('y_mask', ctypes.c_void_p)]


def bnb_tile_rows(m):
    return 128 if m > 64 else (64 if m > 32 else 32)


def _conv_fprop(entry, wbytes, x, wk, cout, ksize, stride, dil, pad, bias, out, want_stats, amax=(), minmax=None, bnl=None):
    """the forward launch of the three implicit-GEMM families.  entry / wbytes: the C entry and what its K-major image holds per weight
    (1 fp32, or 6 / 4 bytes of split pieces).  The f16x3 entry alone takes amax = (w_amax, x_amax) pointers in front of the bias, and,
    behind the common arguments, the want_minmax flag (minmax: None marks the other entries) and the normalise-on-load rows"""
    n, c, hi, wi = x.shape
    ho, wo = conv_out_size(hi, ksize, stride, dil, pad), conv_out_size(wi, ksize, stride, dil, pad)
    assert wk.numel() == wbytes * ksize * ksize * c * cout, (wk.shape, c, cout, ksize)
    if out is None:
        out = torch.empty(n, cout, ho, wo, device=x.device)
    assert tuple(out.shape) == (n, cout, ho, wo)          # (the C side sees a pointer and a batch stride)
    f16 = minmax is not None
    slots, st = 0, None
    if want_stats:
        # f16x3: two pixel-waves per 128-pixel tile at every tile height
        slots = n * ((ho * wo + 127) // 128) * 2 if f16 else conv_stats_slots(n, cout, ho, wo)
        st = _scratch(x.device, 'stats', (4 if minmax else 2) * cout * slots, _STATS_FLOOR)
    tail = (0, 0, 0, int(minmax), _p(None if bnl is None else _dense(bnl))) if f16 else ()
    call(entry, x.data_ptr(), _bs(x), _dense(wk, F32 if wbytes == 1 else U8).data_ptr(), *amax, _p(bias), out.data_ptr(), _bs(out),
         n, c, hi, wi, cout, ho, wo, ksize, stride, dil, pad, 0, 0, _p(st), 0, *tail, _stream())
    return (out, st, slots) if want_stats else out


def _conv_dgrad(entry, wbytes, dy, wk_d, cin, in_hw, ksize, stride, dil, pad, out, accumulate, bnb, amax=(), tail=()):
    """the data-gradient launch of the three families (as _conv_fprop; tail: the f16x3 entry's gate and its unused forward arguments)"""
    n, co, ho, wo = dy.shape
    hi, wi = in_hw
    assert wk_d.numel() == wbytes * ksize * ksize * co * cin
    if out is None:
        assert not accumulate
        out = torch.empty(n, cin, hi, wi, device=dy.device)
    assert tuple(out.shape) == (n, cin, hi, wi)
    fuse, part, slots, st = 0, None, 0, None
    if bnb is not None:
        st, part, slots = _bnb_struct(bnb, n, cin, hi, wi, co, dy.device)
        fuse = ctypes.addressof(st)
    call(entry, dy.data_ptr(), _bs(dy), _dense(wk_d, F32 if wbytes == 1 else U8).data_ptr(), *amax, 0, out.data_ptr(), _bs(out),
         n, co, ho, wo, cin, hi, wi, ksize, stride, dil, pad, 1, int(accumulate), 0, fuse, *tail, _stream())
    return (out, part, slots) if bnb is not None else out


def conv_fprop(x, wk, cout, ksize, stride=1, dil=1, pad=0, bias=None, out=None, want_stats=False):
    """want_stats: also return (stats_ws, slots), the epilogue's per-channel BN partial sums"""
    return _conv_fprop('pfst_conv_igemm', 1, x, wk, cout, ksize, stride, dil, pad, bias, out, want_stats)


def conv_dgrad(dy, wk_d, cin, in_hw, ksize, stride=1, dil=1, pad=0, out=None, accumulate=False, bnb=None):
    """bnb = (pre, y | None, coef, relu): `out` is the COMPLETE gradient of a conv -> BN layer's output and this launch also emits
    that layer's BatchNorm-backward sums (pfst_bnb_fuse_t); returns (out, partials, slots) then."""
    return _conv_dgrad('pfst_conv_igemm', 1, dy, wk_d, cin, in_hw, ksize, stride, dil, pad, out, accumulate, bnb)


def pack_weight_split(w, want_fprop=True, want_dgrad=True, out_f=None, out_d=None):
    """w [Cout][Cin][k][k] -> bf16x3-split K-major images (uint8 buffers of 6 bytes per weight)."""
    _dense(w)
    co, ci, kh, kw = w.shape
    wf, wd = _pack_outs(w, want_fprop, want_dgrad, out_f, out_d, (6 * co * ci * kh * kw,), dtype=U8)
    call('pfst_conv_pack_weight_split', w.data_ptr(), _p(wf), _p(wd), co, ci, kh * kw, _stream())
    return wf, wd


def conv_fprop_split(x, wk6, cout, ksize, stride=1, dil=1, pad=0, bias=None, out=None, want_stats=False):
    return _conv_fprop('pfst_conv_igemm_split', 6, x, wk6, cout, ksize, stride, dil, pad, bias, out, want_stats)


# ---------------------------------------------------------------- fp32-faithful two-piece fp16 split (csrc/conv_f16x3.hip)
AMAX_SUB = 1024        # floats per slot group (csrc/amax.h)
_amax_arena = {}


def amax_slots(dev, groups=1):
    """`groups` zeroed slot groups (groups x 1024 fp32) carved out of a zero-filled arena block: one memset per 4096 groups instead of one
    per tensor.  A block that is used up is replaced by a fresh one; the old one lives as long as views of it do."""
    need = groups * AMAX_SUB
    # one arena per (device, stream): a block is zero-filled on the stream that allocates it, and the first kernel to touch a group
    # (the producer publishing into it) runs on that same stream; consumers on other streams are ordered behind the producer anyway
    key = (dev, torch.cuda.current_stream().cuda_stream)
    blk = _amax_arena.get(key)
    if blk is None or blk[1] + need > blk[0].numel():
        blk = [torch.zeros(max(1 << 22, need), dtype=F32, device=dev), 0]
        _amax_arena[key] = blk
    out = blk[0][blk[1]:blk[1] + need]
    blk[1] += need
    return out


def absmax(x, planes=1, out=None):
    """max |x| -> device slot group(s) of 1024 fp32 (csrc/amax.h).  planes = 1: one group for the whole tensor (a dense tensor, or a dense-plane NCHW view such as a
    channel slice of a concat buffer); planes > 1: x is dense and viewed as `planes` equal contiguous parts, one slot each.
    out: slots to extend (already zeroed or holding an earlier maximum)"""
    if out is None:
        out = amax_slots(x.device, planes)
    if planes == 1 and x.dim() == 4 and not x.is_contiguous():
        n, c, h, w = x.shape
        call('pfst_absmax', x.data_ptr(), c * h * w, n, _bs(x), 0, out.data_ptr(), _stream())
        return out
    _dense(x)
    n = x.numel() // planes
    assert n * planes == x.numel()
    call('pfst_absmax', x.data_ptr(), n, planes, n, 1, out.data_ptr(), _stream())
    return out


def set_f16x3_slots(slots):
    """resident workgroup slots the f16x3 GEMMs size their tile-chain grid for (0: the device's two per CU) -- a test hook"""
    call('pfst_f16x3_set_slots', int(slots))


def f16x3_eligible(cin, cout, ksize=3):
    """the f16x3 implicit GEMM covers contractions over whole 32-channel blocks -- a 1x1 convolution also a last half block: the loads of
    the missing 16 channels fall outside their buffers' ranges and return zeros (the range check includes the scalar offset on gfx950:
    tools/probes/soffset_range_probe.hip) -- and more than 32 output rows (33 ... 64: the 64-row tile, one 32-row block per wave)"""
    return (cin % 32 == 0 or (ksize == 1 and cin % 16 == 0)) and cout > F16X3_MIN_ROWS


F16X3_MIN_ROWS = 32


def pack_weight_f16x2(w, want_fprop=True, want_dgrad=True, out_f=None, out_d=None, amax=None, sets=1):
    """w [Cout][Cin][k][k] (or `sets` plain [Cout][Cin] Winograd-domain filter sets) -> two-piece fp16 K-major images (uint8 buffers of
    4 bytes per weight per layout) + the slots with max |w| per set that fixed their scales"""
    _dense(w)
    if sets == 1:
        co, ci, kh, kw = w.shape
        t = kh * kw
    else:
        assert w.dim() == 3 and w.shape[0] == sets
        _, co, ci = w.shape
        t = 1
    wf, wd = _pack_outs(w, want_fprop, want_dgrad, out_f, out_d, (4 * sets * co * ci * t,), dtype=U8)
    if amax is None:
        amax = absmax(w, sets)
    call('pfst_conv_pack_weight_f16x2', w.data_ptr(), _p(wf), _p(wd), co, ci, t, sets, amax.data_ptr(), _stream())
    return wf, wd, amax


class _WeightJob(ctypes.Structure):             # pfst_weight_job_t (include/pfst_hip.h)
    _fields_ = [('src', ctypes.c_void_p), ('dst_f', ctypes.c_void_p), ('dst_d', ctypes.c_void_p), ('amax_f', ctypes.c_void_p),
                ('amax_d', ctypes.c_void_p), ('Cout', ctypes.c_int), ('Cin', ctypes.c_int), ('T', ctypes.c_int), ('sets', ctypes.c_int),
                ('m', ctypes.c_int), ('first_block', ctypes.c_int)]


class WeightJobTable:
    """a job table of the batched weight preparation: the host copy the library checks and its device copy the kernel reads.
    jobs: dicts with the fields of pfst_weight_job_t (tensors or None for the pointers); pack: 0 = prep table, 1 = pack table"""

    def __init__(self, jobs, pack, dev):
        self.n = len(jobs)
        self.host = (_WeightJob * self.n)()
        first = 0
        for j, d in zip(self.host, jobs):
            j.src, j.dst_f, j.dst_d, j.amax_f, j.amax_d = (_p(d.get(k)) or None for k in ('src', 'dst_f', 'dst_d', 'amax_f', 'amax_d'))
            j.Cout, j.Cin, j.T, j.sets, j.m, j.first_block = d['Cout'], d['Cin'], d['T'], d.get('sets', 1), d.get('m', 0), first
            first += lib().pfst_weight_job_blocks(ctypes.addressof(j), pack)
        self.blocks = first
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=U8).to(dev)
        self.keep = [t for d in jobs for t in d.values() if torch.is_tensor(t)]     # the buffers the table points into

    def run(self, name):
        call(name, ctypes.addressof(self.host), self.dev.data_ptr(), self.n, _stream())


BNL_MAX_C = 2048          # coefficient rows the normalising GEMM keeps in LDS (conv_f16x3.hip BNL_ROWS)


def conv_fprop_bnl_ok(cin, cout, ksize, stride=1, pad=0):
    """can conv_fprop_f16x3 normalise its input as it loads (bnl=...): the 256-row pixel-to-pixel tile, coefficient rows in LDS"""
    return ksize == 1 and stride == 1 and pad == 0 and cout % 256 == 0 and cin <= BNL_MAX_C and f16x3_eligible(cin, cout, 1)


def conv_fprop_f16x3(x, wk4, w_amax, x_amax, cout, ksize, stride=1, dil=1, pad=0, bias=None, out=None, want_stats=False, want_minmax=False,
                     bnl=None):
    """want_minmax (with want_stats): the statistics scratch also receives the per-channel (minimum, maximum) partials of the output behind
    the sums -- bn_finalize_partials(predict_amax=...) turns them into max |relu(bn(out))|.
    bnl: coef [C, 4] of the conv -> BN -> ReLU layer feeding this one: x is that layer's PRE-normalisation output, normalised between load and
    split (x_amax = the predicted max of the normalised tensor)"""
    c = x.shape[1]
    assert bnl is None or (tuple(bnl.shape) == (c, 4) and bias is None and conv_fprop_bnl_ok(c, cout, ksize, stride, pad))
    assert f16x3_eligible(c, cout, ksize)
    return _conv_fprop('pfst_conv_igemm_f16x3', 4, x, wk4, cout, ksize, stride, dil, pad, bias, out, want_stats,
                       amax=(w_amax.data_ptr(), x_amax.data_ptr()), minmax=bool(want_minmax and want_stats and bias is None), bnl=bnl)


def conv_wgrad_f16x3_(dw, x, dy, x_amax, dy_amax, bnl=None):
    """dw += dL/dw of a stride-1 1x1 convolution with the f16x3 split (fp32 atomics); bnl: as conv_fprop_f16x3 (x is the pre-normalisation
    tensor, x_amax the predicted maximum of the normalised one)"""
    n, ci, h, w = x.shape
    co = dy.shape[1]
    assert dy.shape == (n, co, h, w) and dw.numel() == co * ci and (bnl is None or tuple(bnl.shape) == (ci, 4))
    call('pfst_conv_wgrad_f16x3', x.data_ptr(), _bs(x), dy.data_ptr(), _bs(dy), _dense(dw).data_ptr(), n, ci, co, h * w,
         x_amax.data_ptr(), dy_amax.data_ptr(), _p(None if bnl is None else _dense(bnl)), _stream())
    return dw


def dgrad_gate_ok(cin, in_hw):
    """can conv_dgrad_f16x3 add a ReLU-gated tensor in its epilogue (gate=...): whole 128-row tiles, whole 256-element mask groups"""
    return cin % 128 == 0 and (in_hw[0] * in_hw[1]) % 256 == 0


def conv_dgrad_f16x3(dy, wk4_d, w_amax, dy_amax, cin, in_hw, ksize, stride=1, dil=1, pad=0, out=None, accumulate=False, bnb=None, gate=None):
    """bnb: as conv_dgrad (returns (out, partials, slots) then);
    gate = (g, mask): out = data gradient + (mask bit ? g : 0) -- g an [N, cin, H, W] tensor, mask the ReLU bitmask bn_apply(want_mask=True)
    returned for a tensor of that shape (the identity branch of a residual block; `out` has no earlier writer: accumulate = False)"""
    n, co, ho, wo = dy.shape
    hi, wi = in_hw
    g_ptr, g_bs, m_ptr = 0, 0, 0
    if gate is not None:
        g, mask = gate
        assert not accumulate and dgrad_gate_ok(cin, in_hw) and tuple(g.shape) == (n, cin, hi, wi)
        assert mask.dtype == torch.int64 and mask.numel() == n * cin * hi * wi // 64
        g_ptr, g_bs, m_ptr = g.data_ptr(), _bs(g), mask.data_ptr()
    assert f16x3_eligible(co, cin, ksize)
    return _conv_dgrad('pfst_conv_igemm_f16x3', 4, dy, wk4_d, cin, in_hw, ksize, stride, dil, pad, out, accumulate, bnb,
                       amax=(w_amax.data_ptr(), dy_amax.data_ptr()), tail=(g_ptr, g_bs, m_ptr, 0, 0))


def _bnb_struct(bnb, n, cin, hi, wi, co, dev):
    """-> (ctypes struct kept alive by the caller, partials tensor, slots) for a fused BatchNorm-backward data-gradient launch"""
    pre, y, coef, relu = bnb[:4]
    mask = bnb[4] if len(bnb) > 4 else None            # bn_apply's ReLU bitmask of y: the f16x3 epilogue reads the gate bits instead of y
    assert tuple(pre.shape) == (n, cin, hi, wi) and (y is None or tuple(y.shape) == tuple(pre.shape))
    assert mask is None or (y is not None and relu and (hi * wi) % 256 == 0 and mask.dtype == torch.int64 and mask.numel() == n * cin * hi * wi // 64)
    assert co % 16 == 0 and cin % bnb_tile_rows(cin) == 0 and tuple(coef.shape) == (cin, 4)
    slots = conv_stats_slots(n, cin, hi, wi)
    part = torch.empty(2 * cin * slots, dtype=F32, device=dev)     # owned by the consumer layer's context until its bn_backward ran
    st = _BnbFuseStruct(pre.data_ptr(), _bs(pre), _p(y), 0 if y is None else _bs(y), _dense(coef).data_ptr(), part.data_ptr(), int(relu), _p(mask))
    return st, part, slots


def conv_dgrad_split(dy, wk6_d, cin, in_hw, ksize, stride=1, dil=1, pad=0, out=None, accumulate=False, bnb=None):
    """bnb: as conv_dgrad (returns (out, partials, slots) then)"""
    return _conv_dgrad('pfst_conv_igemm_split', 6, dy, wk6_d, cin, in_hw, ksize, stride, dil, pad, out, accumulate, bnb)


def conv_wgrad_(dw, x, dy, ksize, stride=1, dil=1, pad=0):
    """dw += dL/dw (fp32 atomics)."""
    n, ci, hi, wi = x.shape
    _, co, ho, wo = dy.shape
    assert dy.shape[0] == n and dw.numel() == co * ci * ksize * ksize
    call('pfst_conv_wgrad', x.data_ptr(), _bs(x), dy.data_ptr(), _bs(dy), _dense(dw).data_ptr(), n, ci, hi, wi, co, ho, wo,
         ksize, stride, dil, pad, _stream())
    return dw


def conv_wgrad_split_(dw, x, dy, ksize, stride=1, dil=1, pad=0):
    """dw += dL/dw with the fp32-faithful bf16x6 split (fp32 atomics)."""
    n, ci, hi, wi = x.shape
    _, co, ho, wo = dy.shape
    assert dy.shape[0] == n and dw.numel() == co * ci * ksize * ksize
    call('pfst_conv_wgrad_split', x.data_ptr(), _bs(x), dy.data_ptr(), _bs(dy), _dense(dw).data_ptr(), n, ci, hi, wi, co, ho, wo,
         ksize, stride, dil, pad, _stream())
    return dw


def wgrad_q_operands_ok(x, dy):
    """the operand layout the K-quad weight-gradient kernels need beyond the layer's shape (pfst_wgrad_q_eligible, csrc/conv_wgrad_q.hip):
    16-byte aligned planes, batch strides in whole float4s.  A caller that fails this takes the generic kernel instead of an error."""
    return x.data_ptr() % 16 == 0 and dy.data_ptr() % 16 == 0 and _bs(x) % 4 == 0 and _bs(dy) % 4 == 0


def conv_wgrad_f16q_(dw, x, dy, x_amax, dy_amax, ksize, dil=1):
    """dw += dL/dw of a stride-1 'same' convolution (1x1, or 3x3 with pad == dil) with the f16x3 split on the K-quad kernel (fp32 atomics):
    the direct 3x3 layers of the stems / layer1 and the 1x1 layers with <= 64 output channels"""
    n, ci, h, w = x.shape
    co = dy.shape[1]
    assert tuple(dy.shape) == (n, co, h, w) and dw.numel() == co * ci * ksize * ksize
    call('pfst_conv_wgrad_f16x3_q', x.data_ptr(), _bs(x), dy.data_ptr(), _bs(dy), _dense(dw).data_ptr(), n, ci, h, w, co, ksize, dil,
         x_amax.data_ptr(), dy_amax.data_ptr(), _stream())
    return dw


def bias_grad_(db, dy):
    n, c, h, w = dy.shape
    call('pfst_bias_grad', dy.data_ptr(), _bs(dy), _dense(db).data_ptr(), n, c, h * w, _stream())
    return db


# ---------------------------------------------------------------- Winograd F(2x2,3x3) (wide stride-1 3x3 convolutions)
_wino_ws, _wino_cache = _scratch, _scratch_cache        # the transform-domain scratch (tags 'V' 'M' 'U' 'Pf' 'Pd', exact sizes) under its older names


# output tile edge m of the Winograd F(m x m, 3x3) transforms: 4 (4x fewer MACs, 36 transform indices) or 2 (2.25x, 16 indices)
WINO_TILE = 4


def _wino_m(m):
    m = WINO_TILE if m is None else int(m)
    assert m in (2, 4)
    return m, (m + 2) * (m + 2)


def set_wgrad_lds_pad(nbytes):
    """occupancy cap of the K-quad weight-gradient kernels (pfst_conv_wgrad_set_lds_pad)"""
    call('pfst_conv_wgrad_set_lds_pad', int(nbytes))


def wgrad_split_k(work, p, slots=0, k_step=0, chunk_cap=0, doubling=False):
    """(chunks, chunk_len) of a weight-gradient launch of `work` workgroups over `p` pixels: the library's own split-K planner
    (pfst_wgrad_split_k; host arithmetic, no device)"""
    chunks, chunk_len = ctypes.c_int(0), ctypes.c_int(0)
    call('pfst_wgrad_split_k', int(work), int(p), int(slots), int(k_step), int(chunk_cap), int(bool(doubling)), ctypes.addressof(chunks),
         ctypes.addressof(chunk_len))
    return chunks.value, chunk_len.value


def wino_tiles(h, w, dil, m=None):
    return lib().pfst_wino_tiles(h, w, dil, _wino_m(m)[0])


def _wino_filter_dims(w, m):
    _dense(w)
    m, nx = _wino_m(m)
    co, ci, kh, kw = w.shape
    assert kh == 3 and kw == 3
    return m, nx, co, ci


def wino_pack_weight(w, want_fprop=True, want_dgrad=True, out_f=None, out_d=None, m=None):
    """w [Cout][Cin][3][3] -> transform-domain filters U[X][K/4][M][4], X = (m+2)^2, for fprop (K = Cin) and dgrad (K = Cout, flipped)."""
    m, nx, co, ci = _wino_filter_dims(w, m)
    uf, ud = _pack_outs(w, want_fprop, want_dgrad, out_f, out_d, (nx * co * ci,))
    call('pfst_wino_pack_weight', w.data_ptr(), _p(uf), _p(ud), co, ci, m, _stream())
    return uf, ud


def _wino_filter_plain(w, want_fprop, want_dgrad, m):
    """the plain fp32 transform-domain filter sets [X][Cout][Cin] (data gradient: [X][Cin][Cout], flipped) in per-stream scratch: what the
    split packings of both arithmetics start from; -> (m, X, Cout, Cin, sets_f | None, sets_d | None)"""
    m, nx, co, ci = _wino_filter_dims(w, m)
    pf = _scratch(w.device, 'Pf', nx * co * ci) if want_fprop else None
    pd = _scratch(w.device, 'Pd', nx * co * ci) if want_dgrad else None
    call('pfst_wino_filter_plain', w.data_ptr(), _p(pf), _p(pd), co, ci, m, _stream())
    return m, nx, co, ci, pf, pd


def wino_pack_weight_split(w, want_fprop=True, want_dgrad=True, out_f=None, out_d=None, m=None):
    """transform-domain filters for the bf16x6 GEMM: X split-packed sets (uint8 buffers of X * 6 * Cout * Cin bytes)"""
    m, nx, co, ci, pf, pd = _wino_filter_plain(w, want_fprop, want_dgrad, m)
    uf, ud = _pack_outs(w, want_fprop, want_dgrad, out_f, out_d, (nx * 6 * co * ci,), dtype=U8)
    call('pfst_wino_pack_weight_split', _p(pf), _p(pd), _p(uf), _p(ud), co, ci, m, _stream())
    return uf, ud


def wino_pack_weight_f16(w, want_fprop=True, want_dgrad=True, out_f=None, out_d=None, m=None, shared_dy=False):
    """transform-domain filters for the f16x3 GEMM: X two-piece fp16 sets (uint8 buffers of X * 4 * Cout * Cin bytes) + the X slots with
    each set's absolute maximum; -> (uf, ud, amax_f, amax_d).
    shared_dy: the data-gradient image is the one wino_dgrad_shared reads -- the UNFLIPPED forward sets in the data-gradient layout
    (K = Cout, rows = Cin), scaled by the forward sets' maxima (amax_d is amax_f) -- instead of the flipped sets wino_conv reads"""
    if shared_dy and want_dgrad:
        m, nx, co, ci, pf, _ = _wino_filter_plain(w, True, False, m)
        uf, ud, af = pack_weight_f16x2(pf[:nx * co * ci].view(nx, co, ci), want_fprop, True, out_f=out_f, out_d=out_d, sets=nx)
        return uf, ud, (af if want_fprop else None), af
    m, nx, co, ci, pf, pd = _wino_filter_plain(w, want_fprop, want_dgrad, m)
    uf = ud = af = ad = None
    if want_fprop:
        uf, _, af = pack_weight_f16x2(pf[:nx * co * ci].view(nx, co, ci), True, False, out_f=out_f, sets=nx)
    if want_dgrad:
        _, ud, ad = pack_weight_f16x2(pd[:nx * co * ci].view(nx, co, ci), False, True, out_d=out_d, sets=nx)
    return uf, ud, af, ad


def wino_conv(x, u, cout, dil, out=None, accumulate=False, keep_v=False, want_stats=False, m=None, u_amax=None, x_amax=None, bnl=None,
              want_minmax=False, bnb=None):
    """'same' 3x3 stride-1 convolution (or its data gradient, with the dgrad filter) through the transform domain.
    keep_v: the transformed input goes to a tensor of its own and is returned as (out, V) for the weight gradient
    (288 GB of HBM: keeping it resident beats re-transforming the input in backward).
    bnl: coef [C, 4] of the conv -> BN -> ReLU layer feeding this one: x is that layer's PRE-normalisation output, normalised by the input
    transform as it loads (x_amax then = the predicted max of the normalised tensor, bn_finalize_partials(predict_amax=...)).
    bnb = (pre, coef, relu): `pre` needs 16-byte aligned planes and a batch stride in whole float4s (a channel slice of an aligned buffer
    with HW % 4 == 0); pfst_wino_output refuses any other, before it writes `out`"""
    n, c, h, w = x.shape
    assert bnl is None or (tuple(bnl.shape) == (c, 4) and (u_amax is None or x_amax is not None))
    m, nx = _wino_m(m)
    t = wino_tiles(h, w, dil, m)
    assert u.numel() == nx * c * cout * ((4 if u_amax is not None else 6) if u.dtype == U8 else 1), 'filter set was packed for another tile size'
    v = torch.empty(nx * n * c * t, dtype=F32, device=x.device) if keep_v else _scratch(x.device, 'V', nx * n * c * t)
    mb = _scratch(x.device, 'M', nx * n * cout * t)
    if out is None:
        assert not accumulate
        out = torch.empty(n, cout, h, w, device=x.device)
    assert tuple(out.shape) == (n, cout, h, w)
    # f16x3 (u_amax given): the input transform writes V PRE-SPLIT -- two fp16 pieces per element, scaled from max |x| (x_amax: the slot
    # group the producer of x published, else computed here) through the transform's norm bound -- and v_amax receives that bound
    v_amax = amax_slots(x.device) if u_amax is not None else None
    if u_amax is not None and x_amax is None:
        x_amax = absmax(x)
    call('pfst_wino_input', x.data_ptr(), _bs(x), v.data_ptr(), n, c, h, w, dil, m, _p(v_amax), _p(x_amax) if u_amax is not None else 0,
         _p(None if bnl is None else _dense(bnl)), _stream())
    if u_amax is not None:              # two-piece fp16 filter sets -> f16x3 GEMM
        call('pfst_wino_gemm_f16x3', v.data_ptr(), u.data_ptr(), u_amax.data_ptr(), v_amax.data_ptr(), mb.data_ptr(), n, c, cout, t, m, 1, _stream())
    else:
        gemm = 'pfst_wino_gemm_split' if u.dtype == U8 else 'pfst_wino_gemm'        # split-packed filters -> bf16x6 GEMM
        call(gemm, v.data_ptr(), _dense(u, u.dtype).data_ptr(), mb.data_ptr(), n, c, cout, t, m, _stream())
    slots, st = 0, None
    if want_stats:                      # BN partial sums of the output come out of the output transform
        slots = n * lib().pfst_wino_stats_slots(h, w, dil, m)
        st = _scratch(x.device, 'stats', (4 if want_minmax else 2) * cout * slots, _STATS_FLOOR)
    bx, bx_bs, bcoef, brelu = 0, 0, 0, 0
    if bnb is not None:
        # a data-gradient launch that completes the gradient of a conv -> BN [-> ReLU] layer's output (no residual): bnb = (pre, coef, relu) of
        # that layer -> returns (out, partials, slots) with its BatchNorm-backward sums for bn_backward(partials=...), no reduction pass
        assert not want_stats
        pre, coef, relu = bnb
        assert tuple(pre.shape) == (n, cout, h, w) and tuple(coef.shape) == (cout, 4)
        slots = n * lib().pfst_wino_stats_slots(h, w, dil, m)
        st = torch.empty(2 * cout * slots, dtype=F32, device=x.device)        # owned by the layer's context until its bn_backward ran
        bx, bx_bs, bcoef, brelu = pre.data_ptr(), _bs(pre), _dense(coef).data_ptr(), int(relu)
    call('pfst_wino_output', mb.data_ptr(), out.data_ptr(), _bs(out), n, cout, h, w, dil, int(accumulate), _p(st),
         int(bool(want_minmax and want_stats)), bx, bx_bs, bcoef, brelu, m, _stream())
    res = (out, st, slots) if (want_stats or bnb is not None) else (out,)
    if keep_v:
        res = res + ((v, v_amax),)          # the transformed input and the slot group with its absolute maximum (None unless f16x3)
    return res if len(res) > 1 else res[0]


def wino_dy(dy, dil, dy_amax=None, m=None):
    """dM = A dY A^T of an f16x3 Winograd layer, PRE-SPLIT, in a tensor of its own (not the 'M' scratch: the data-gradient GEMM's result
    lives there while the weight gradient still reads dM on its side stream) -> (dM, dm_amax), for wino_dgrad_shared and
    wino_wgrad_(dm=...); dy_amax: the slot group with max |dy| (computed here otherwise)"""
    n, co, h, w = dy.shape
    m, nx = _wino_m(m)
    t = wino_tiles(h, w, dil, m)
    dm = torch.empty(nx * n * co * t, dtype=F32, device=dy.device)
    dm_amax = amax_slots(dy.device)
    if dy_amax is None:
        dy_amax = absmax(dy)
    call('pfst_wino_dy', dy.data_ptr(), _bs(dy), dm.data_ptr(), n, co, h, w, dil, m, dm_amax.data_ptr(), dy_amax.data_ptr(), _stream())
    return dm, dm_amax


def wino_dx_slots(h, w, dil, m=None):
    return lib().pfst_wino_dx_slots(h, w, dil, _wino_m(m)[0])


def wino_dx(p, cin, hw, dil, n, out=None, accumulate=False, m=None, bnb=None):
    """dx [n, cin, h, w] from the transform-domain product P [X][n][cin][T] of dM with the transposed forward filter sets: the patches
    B P B^T overlap-added at stride m (pfst_wino_dx: a gather in a fixed order, bitwise reproducible); out / accumulate / bnb as wino_conv"""
    h, w = hw
    m, nx = _wino_m(m)
    assert p.numel() >= nx * n * cin * wino_tiles(h, w, dil, m)
    if out is None:
        assert not accumulate
        out = torch.empty(n, cin, h, w, device=p.device)
    assert tuple(out.shape) == (n, cin, h, w)
    st, slots, bx, bx_bs, bcoef, brelu = None, 0, 0, 0, 0, 0
    if bnb is not None:
        pre, coef, relu = bnb
        assert tuple(pre.shape) == (n, cin, h, w) and tuple(coef.shape) == (cin, 4)
        slots = n * wino_dx_slots(h, w, dil, m)
        st = torch.empty(2 * cin * slots, dtype=F32, device=p.device)         # owned by the layer's context until its bn_backward ran
        bx, bx_bs, bcoef, brelu = pre.data_ptr(), _bs(pre), _dense(coef).data_ptr(), int(relu)
    call('pfst_wino_dx', p.data_ptr(), out.data_ptr(), _bs(out), n, cin, h, w, dil, int(accumulate), _p(st), bx, bx_bs, bcoef, brelu, m, _stream())
    return (out, st, slots) if bnb is not None else out


def wino_dgrad_shared(dm, dm_amax, ut, ut_amax, n, cout, cin, hw, dil, out=None, accumulate=False, m=None, bnb=None):
    """the data gradient of an f16x3 Winograd layer from the weight gradient's transform dM (wino_dy): the f16x3 GEMM of dM with the
    transposed forward filter sets (wino_pack_weight_f16(shared_dy=True): ut, ut_amax) into the 'M' scratch, then wino_dx"""
    h, w = hw
    m, nx = _wino_m(m)
    t = wino_tiles(h, w, dil, m)
    assert dm.numel() >= nx * n * cout * t and ut.dtype == U8 and ut.numel() == nx * 4 * cin * cout, 'filter set was packed for another tile size'
    pb = _scratch(dm.device, 'M', nx * n * cin * t)
    call('pfst_wino_gemm_f16x3', dm.data_ptr(), ut.data_ptr(), ut_amax.data_ptr(), dm_amax.data_ptr(), pb.data_ptr(), n, cout, cin, t, m, 1, _stream())
    return wino_dx(pb, cin, hw, dil, n, out=out, accumulate=accumulate, m=m, bnb=bnb)


def wino_wgrad_(dw, x, dy, dil, v=None, m=None, split=False, v_amax=None, x_amax=None, dy_amax=None, dm=None, dm_amax=None):
    """dw += dL/dw of the 'same' 3x3 stride-1 convolution; v: the transformed input kept from the forward pass (same m);
    split: the transform-domain products with the fp32-faithful bf16x6 split instead of the fp32-input MFMA;
    dm, dm_amax: the packed transform of dy the data gradient already made (wino_dy; f16x3 only) -- no pfst_wino_dy here"""
    n, ci, h, w = x.shape
    co = dy.shape[1]
    m, nx = _wino_m(m)
    assert dy.shape == (n, co, h, w) and dw.numel() == co * ci * 9
    t = wino_tiles(h, w, dil, m)
    du = _scratch(x.device, 'U', nx * co * ci)
    # split: False / 0 fp32-input MFMA, True / 1 bf16x6, 2 f16x3 (falls back to bf16x6 for <= 64 rows).  f16x3: both operands PRE-SPLIT by
    # their transforms (v given: the packed V and its bound group kept from the f16x3 forward pass)
    f16 = split == 2 and co > 64
    assert not (f16 and v is not None and v_amax is None), 'a kept V must come with the slot group of its scale bound'
    assert f16 or v_amax is None, 'a packed V kept from an f16x3 forward pass needs the f16x3 weight gradient'
    if v is None:
        v = _scratch(x.device, 'V', nx * n * ci * t)
        v_amax = amax_slots(x.device) if f16 else None
        if f16 and x_amax is None:
            x_amax = absmax(x)
        call('pfst_wino_input', x.data_ptr(), _bs(x), v.data_ptr(), n, ci, h, w, dil, m, _p(v_amax), _p(x_amax) if f16 else 0, 0, _stream())
    assert v.numel() >= nx * n * ci * t
    if dm is not None:
        assert f16 and dm_amax is not None and dm.numel() >= nx * n * co * t, 'a supplied dM is the packed transform of the f16x3 route'
    else:
        dm = _scratch(x.device, 'M', nx * n * co * t)
        dm_amax = amax_slots(x.device) if f16 else None
        if f16 and dy_amax is None:
            dy_amax = absmax(dy)
        call('pfst_wino_dy', dy.data_ptr(), _bs(dy), dm.data_ptr(), n, co, h, w, dil, m, _p(dm_amax), _p(dy_amax) if f16 else 0, _stream())
    call('pfst_wino_wgrad', v.data_ptr(), dm.data_ptr(), du.data_ptr(), _dense(dw).data_ptr(), n, ci, co, t, m,
         2 if f16 else int(bool(split)), _p(v_amax), _p(dm_amax), int(f16), _stream())
    return dw


# ---------------------------------------------------------------- depthwise
def dwconv(x, w, dil, flip=False, out=None, accumulate=False, want_stats=False, bnl=None, want_minmax=False):
    """want_stats: also return (stats_ws, slots), per-channel BN partial sums of the output (as conv_fprop); want_minmax: followed by the
    (minimum, maximum) partials (as conv_fprop_f16x3);
    bnl: coef [C, 4] of the conv -> BN -> ReLU layer feeding this one: x is that layer's PRE-normalisation output, normalised on load"""
    n, c, h, wd = x.shape
    assert w.numel() == c * 9
    if out is None:
        assert not accumulate
        out = torch.empty(n, c, h, wd, device=x.device)
    slots, st = 0, None
    if want_stats:
        slots = n * lib().pfst_dwconv_stats_slots(h, wd, dil)
        st = _scratch(x.device, 'stats', (4 if want_minmax else 2) * c * slots, _STATS_FLOOR)
    call('pfst_dwconv3x3', x.data_ptr(), _bs(x), _dense(w).data_ptr(), out.data_ptr(), _bs(out), n, c, h, wd, dil,
         int(flip), int(accumulate), _p(st), int(bool(want_minmax and want_stats)), _p(bnl), _stream())
    return (out, st, slots) if want_stats else out


def dwconv_wgrad_(dw, x, dy, dil):
    n, c, h, w = x.shape
    assert dy.shape == x.shape and dw.numel() == c * 9
    call('pfst_dwconv3x3_wgrad', x.data_ptr(), _bs(x), dy.data_ptr(), _bs(dy), _dense(dw).data_ptr(), n, c, h, w, dil, _stream())
    return dw


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def dwconv_multi_ok(x, dils):
    """the fused multi-branch depthwise kernels cover this input (whole planes <= 16384 elements, W % 4 == 0, dilations % 4 == 0, dense
    16-byte aligned planes)"""
    n, c, h, w = x.shape
    if not (x.stride(3) == 1 and x.stride(2) == w and x.stride(1) == h * w):
        return False
    return (1 <= len(dils) <= 3 and _bs(x) % 4 == 0 and x.data_ptr() % 16 == 0
            and bool(lib().pfst_dwconv3x3_multi_ok(h, w, len(dils), (ctypes.c_int * len(dils))(*dils))))


def dwconv_multi(x, ws, dils, want_stats=False, want_mean=False, want_minmax=False):
    """y_i = depthwise 3x3 conv of x with filters ws[i] at dilation dils[i], every input plane staged ONCE for all branches
    -> [(y_i, stats_i, slots_i)] (stats as dwconv(want_stats=True): per-channel BN partials, one slot per image);
    want_mean: -> (that list, [N, C, 1, 1] plane means of x = global_avgpool(x)) from the same pass"""
    n, c, h, w = x.shape
    k = len(ws)
    ys = [torch.empty(n, c, h, w, device=x.device) for _ in range(k)]
    want_minmax = bool(want_minmax and want_stats)          # the (minimum, maximum) partials behind each branch's sums
    sts = [(_scratch(x.device, ('multi', i), (4 if want_minmax else 2) * c * n, 1 << 16) if want_stats else None) for i in range(k)]
    mean = torch.empty(n, c, 1, 1, device=x.device) if want_mean else None
    call('pfst_dwconv3x3_multi_fwd', x.data_ptr(), _bs(x), k, _ptr_array([_dense(t) for t in ws]), _ptr_array(ys),
         (ctypes.c_longlong * k)(*[_bs(y) for y in ys]), _ptr_array(sts), int(want_minmax), (ctypes.c_int * k)(*dils), _p(mean), n, c, h, w,
         _stream())
    res = [(ys[i], sts[i], n if want_stats else 0) for i in range(k)]
    return (res, mean) if want_mean else res


def dwconv_multi_bwd_(dws, x, dys, ws, dils, dx, accumulate=False, mean_grad=None, bnb=None):
    """dws[i] += weight gradients, dx (+)= sum_i mirrored stencil of dys[i]: x read once, every dy once, dx written once;
    mean_grad: [N, C] gradient of the plane means dwconv_multi(want_mean=True) returned: dx += mean_grad / (H W);
    bnb = [(pre_i, rec_i)]: dys[i] are the gradients of the branches' BatchNorm + ReLU outputs (see dwconv_bwd_)"""
    n, c, h, w = x.shape
    k = len(ws)
    assert all(tuple(d.shape) == tuple(x.shape) and _bs(d) % 4 == 0 and d.data_ptr() % 16 == 0 for d in dys) and tuple(dx.shape) == tuple(x.shape)
    assert bnb is None or all(_bs(b[0]) == _bs(d) and tuple(b[0].shape) == tuple(d.shape) for b, d in zip(bnb, dys))
    call('pfst_dwconv3x3_multi_bwd', x.data_ptr(), _bs(x), k, _ptr_array([_dense(t) for t in ws]), _ptr_array(dys),
         (ctypes.c_longlong * k)(*[_bs(d) for d in dys]), _ptr_array([_dense(t) for t in dws]), (ctypes.c_int * k)(*dils),
         _p(None if mean_grad is None else _dense(mean_grad)), dx.data_ptr(), _bs(dx), int(accumulate),
         None if bnb is None else _ptr_array([b[0] for b in bnb]), None if bnb is None else _ptr_array([b[1] for b in bnb]),
         n, c, h, w, _stream())
    return dx


def dwconv_bwd_(dw, x, dy, w, dil, dx, accumulate=False, bnl=None, bnb=None):
    """both gradients of the depthwise convolution in one pass: dx (+)= the mirrored stencil of dy, dw += the weight gradient.
    bnb = (pre, rec): dy is the gradient of the layer's BatchNorm + ReLU OUTPUT, pre the convolution's own output, rec from
    bn_backward_sums: the gradient of the convolution output is formed while the rows are staged"""
    n, c, h, wd = x.shape
    assert dy.shape == x.shape and tuple(dx.shape) == tuple(x.shape) and dw.numel() == c * 9 and w.numel() == c * 9
    call('pfst_dwconv3x3_bwd', dy.data_ptr(), _bs(dy), x.data_ptr(), _bs(x), _dense(w).data_ptr(), dx.data_ptr(), _bs(dx),
         _dense(dw).data_ptr(), n, c, h, wd, dil, int(accumulate), _p(bnl), _p(None if bnb is None else bnb[0]),
         0 if bnb is None else _bs(bnb[0]), _p(None if bnb is None else bnb[1]), _stream())
    return dx


# ---------------------------------------------------------------- batch norm
def bn_stats(x, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, gamma=None, beta=None):
    n, c, h, w = x.shape
    mean = torch.empty(c, device=x.device)
    invstd = torch.empty(c, device=x.device)
    coef = torch.empty(c, 4, device=x.device) if gamma is not None else None
    call('pfst_bn_stats', x.data_ptr(), _bs(x), n, c, h * w, mean.data_ptr(), invstd.data_ptr(), _p(running_mean),
         _p(running_var), float(momentum), float(eps), _scratch(x.device, 'bn', 2 * c, 8192, F64).data_ptr(), _p(gamma), _p(beta), _p(coef), _stream())
    return (mean, invstd, coef) if gamma is not None else (mean, invstd)


def bn_apply(x, mean, invstd, gamma, beta, relu=True, residual=None, out=None, want_mask=False, amax=None, post=None, residual_coef=None):
    """want_mask: also return the ReLU gate as a bitmask (int64 words) for bn_backward, or None where the kernel cannot
    produce it (plane size not a multiple of 256, unaligned slices) -- the caller then keeps using y.
    post: [N, C] factors applied after the ReLU (the Dropout2d mask of the layer feeding conv_seg, folded into this pass)"""
    n, c, h, w = x.shape
    assert post is None or (residual is None and post.numel() == n * c)
    assert residual_coef is None or (residual is not None and tuple(residual_coef.shape) == (c, 4))      # the residual is normalised on load
    if out is None:
        out = torch.empty(n, c, h, w, device=x.device)
    assert out.shape == x.shape
    mask = None
    if want_mask and relu and (h * w) % 256 == 0 and all(
            t is None or (_bs(t) % 4 == 0 and t.data_ptr() % 16 == 0) for t in (x, out, residual)):
        mask = torch.empty(n * c * h * w // 64, dtype=torch.int64, device=x.device)
    call('pfst_bn_apply', x.data_ptr(), _bs(x), _p(residual), 0 if residual is None else _bs(residual), out.data_ptr(), _bs(out),
         mean.data_ptr(), invstd.data_ptr(), _dense(gamma).data_ptr(), _dense(beta).data_ptr(), n, c, h * w, int(relu), _p(mask),
         _p(amax), _p(None if post is None else _dense(post)), _p(None if residual_coef is None else _dense(residual_coef)), _stream())
    return (out, mask) if want_mask else out


def bn_backward(dy, y, x, mean, invstd, gamma, dgamma, dbeta, relu=True, dres=None, dres_accumulate=False, dx=None, beta=None,
                mask=None, partials=None, slots=0, amax=None, post=None):
    """mask: the bitmask bn_apply(..., want_mask=True) returned; replaces y as the source of the ReLU gate.
    partials / slots: the (sum dz, sum dz*x) partials the launch that wrote dy emitted (conv_dgrad(bnb=...)): no reduction pass"""
    n, c, h, w = x.shape
    assert dy.shape == x.shape
    assert mask is None or (mask.dtype == torch.int64 and mask.numel() == n * c * h * w // 64 and (h * w) % 256 == 0)
    if dx is None:
        dx = torch.empty(n, c, h, w, device=x.device)
    call('pfst_bn_backward', dy.data_ptr(), _bs(dy), _p(y), 0 if y is None else _bs(y), x.data_ptr(), _bs(x),
         mean.data_ptr(), invstd.data_ptr(), _dense(gamma).data_ptr(), _p(beta), dx.data_ptr(), _bs(dx),
         _p(dres), 0 if dres is None else _bs(dres), int(dres_accumulate), _p(dgamma), _p(dbeta),
         n, c, h * w, int(relu), _p(mask), _scratch(x.device, 'bn', 2 * c, 8192, F64).data_ptr(), _p(partials), int(slots), _p(amax), _p(None if post is None else _dense(post)), _stream())
    return dx


def bn_backward_dual(dy, mask, a, b):
    """the BatchNorm backward of TWO layers that receive the same gated gradient g = (mask bit ? dy : 0) -- bn3 and the downsample branch's BN of
    a stage's first Bottleneck -- in one reduction and one apply pass (pfst_bn_backward_dual).  a / b: dicts x (pre-BN tensor), mean, invstd,
    gamma, dgamma, dbeta, amax (slot group or None); a may carry partials / slots (its sums from the launch that wrote dy).  Returns
    (dxa, dxb), or None when the entry point does not take the case (deterministic mode, unaligned planes, planes that are no multiple of 256
    elements): the caller runs the layers one by one"""
    n, c, h, w = a['x'].shape
    assert dy.shape == a['x'].shape == b['x'].shape
    # the conditions under which pfst_bn_backward_dual answers PFST_ERR_UNSUPPORTED, repeated here (dxa / dxb are allocated below)
    if is_deterministic() or (h * w) % 256 != 0 or any(_bs(t) % 4 or t.data_ptr() % 16 for t in (dy, a["x"], b["x"])):
        return None
    assert mask.dtype == torch.int64 and mask.numel() == n * c * h * w // 64
    dxa, dxb = torch.empty(n, c, h, w, device=dy.device), torch.empty(n, c, h, w, device=dy.device)
    ws = torch.empty(4 * c, dtype=torch.float64, device=dy.device)
    call('pfst_bn_backward_dual', dy.data_ptr(), _bs(dy), mask.data_ptr(),
         a['x'].data_ptr(), _bs(a['x']), a['mean'].data_ptr(), a['invstd'].data_ptr(), _dense(a['gamma']).data_ptr(), dxa.data_ptr(), _bs(dxa),
         _p(a['dgamma']), _p(a['dbeta']), ws.data_ptr(), _p(a.get('partials')), int(a.get('slots', 0)), _p(a.get('amax')),
         b['x'].data_ptr(), _bs(b['x']), b['mean'].data_ptr(), b['invstd'].data_ptr(), _dense(b['gamma']).data_ptr(), dxb.data_ptr(), _bs(dxb),
         _p(b['dgamma']), _p(b['dbeta']), ws[2 * c:].data_ptr(), _p(b.get('amax')), n, c, h * w, _stream())
    return dxa, dxb


def relu_gate_(out, g, mask, accumulate=False):
    """out (+)= g where bn_apply's ReLU bitmask `mask` has the element's bit"""
    n, c, h, w = g.shape
    assert tuple(out.shape) == tuple(g.shape) and mask.dtype == torch.int64 and mask.numel() == n * c * h * w // 64 and (h * w) % 256 == 0
    call('pfst_relu_gate', g.data_ptr(), _bs(g), mask.data_ptr(), out.data_ptr(), _bs(out), n, c, h * w, int(accumulate), _stream())
    return out


BN_BWD_REC_BYTES = 40          # sizeof(pfst_bn_bwd_rec_t): three doubles + four floats


def bn_backward_sums(dy, x, mean, invstd, gamma, beta, dgamma, dbeta, partials=None, slots=0):
    """the first half of bn_backward for a depthwise conv -> BN -> ReLU layer: the two sums (from `partials` or by the reduction pass),
    dgamma / dbeta += ..., and the per-channel record (uint8 [C * 40]) with which the layer's fused depthwise backward applies the second
    half itself while it stages dy and x (dwconv_bwd_(bnb=...), dwconv_multi_bwd_(bnb=...)): dL/dpre is never written"""
    n, c, h, w = x.shape
    assert dy.shape == x.shape
    rec = torch.empty(c * BN_BWD_REC_BYTES, dtype=U8, device=x.device)
    ws = torch.empty(2 * c, dtype=torch.float64, device=x.device)        # its own scratch: the record is read later, by another launch
    call('pfst_bn_backward_sums', dy.data_ptr(), _bs(dy), x.data_ptr(), _bs(x), mean.data_ptr(), invstd.data_ptr(),
         _dense(gamma).data_ptr(), _dense(beta).data_ptr(), _p(dgamma), _p(dbeta), n, c, h * w, ws.data_ptr(), _p(partials), int(slots),
         rec.data_ptr(), _stream())
    return rec


# ---------------------------------------------------------------- pooling / resize
def maxpool(x, bnl=None, amax=None):
    _dense(x)
    n, c, h, w = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty(n, c, ho, wo, device=x.device)
    idx = torch.empty(n, c, ho, wo, dtype=U8, device=x.device)
    call('pfst_maxpool3x3s2', x.data_ptr(), y.data_ptr(), idx.data_ptr(), n * c, h, w, ho, wo, _p(bnl), c, _p(amax), _stream())
    return y, idx


def maxpool_bwd(dy, idx, in_hw):
    _dense(dy)
    n, c, ho, wo = dy.shape
    dx = torch.empty(n, c, in_hw[0], in_hw[1], device=dy.device)
    call('pfst_maxpool3x3s2_bwd', dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), n * c, in_hw[0], in_hw[1], ho, wo, _stream())
    return dx


def resize_bilinear(x, size, out=None):
    n, c, hi, wi = x.shape
    if out is None:
        out = torch.empty(n, c, size[0], size[1], device=x.device)
    call('pfst_resize_bilinear', x.data_ptr(), _bs(x), out.data_ptr(), _bs(out), n, c, hi, wi, size[0], size[1], _stream())
    return out


def resize_bilinear_bwd(dy, in_hw, out=None, accumulate=False):
    n, c, ho, wo = dy.shape
    if out is None:
        assert not accumulate
        out = torch.empty(n, c, in_hw[0], in_hw[1], device=dy.device)
    call('pfst_resize_bilinear_bwd', dy.data_ptr(), _bs(dy), out.data_ptr(), _bs(out), n, c, in_hw[0], in_hw[1], ho, wo,
         int(accumulate), _stream())
    return out


def global_avgpool(x):
    n, c, h, w = x.shape
    y = torch.empty(n, c, 1, 1, device=x.device)
    call('pfst_global_avgpool', x.data_ptr(), _bs(x), y.data_ptr(), n, c, h * w, _stream())
    return y


def reduce_hw(dy):
    n, c, h, w = dy.shape
    v = torch.empty(n, c, 1, 1, device=dy.device)
    call('pfst_reduce_hw', dy.data_ptr(), _bs(dy), v.data_ptr(), n, c, h * w, _stream())
    return v


def broadcast_hw(v, out, scale=1.0, accumulate=False, amax=None):
    n, c, h, w = out.shape
    assert v.numel() == n * c
    call('pfst_broadcast_hw', _dense(v).data_ptr(), out.data_ptr(), _bs(out), n, c, h * w, float(scale), int(accumulate), _p(amax), _stream())
    return out


# ---------------------------------------------------------------- plane <-> pyramid of small grids (csrc/pyramid.hip)
PYR_MAX_SCALES, PYR_MAX_SCALE = 6, 8          # PFST_PYR_MAX_SCALES / PFST_PYR_MAX_SCALE
_pyramid_tables = {}


def check_pool_scales(scales):
    """the scales the pyramid kernels take: one to six grids of 1 .. 8 cells per side"""
    scales = tuple(int(s) for s in scales)
    if not 1 <= len(scales) <= PYR_MAX_SCALES or any(not 1 <= s <= PYR_MAX_SCALE for s in scales):
        raise NotImplementedError(f'pyramid kernels: 1 to {PYR_MAX_SCALES} scales of 1 .. {PYR_MAX_SCALE} cells per side, got {scales}')
    return scales


def pyramid_operator(kind, n, scales):
    """The per-axis operator of the pyramid kernels for an axis of `n` pixels, on the host in fp64 (no device needed):
    -> (D [sum(scales), n], span int32 [sum(scales), 2], tspan int32 [len(scales), n, 2]).  Rows off1[k] .. off1[k] + s_k of D belong to scale k.
    kind 'pool':     row i of scale s is 1 / (b - a) on [a, b) = [floor(i n / s), ceil((i + 1) n / s)): nn.AdaptiveAvgPool2d(s) is Dh X Dw^T;
    kind 'bilinear': D = A^T, A [n, s] the bilinear resize from s to n cells (align_corners=False, torch's
                     area_pixel_compute_source_index: src = max(0, s / n (dst + 0.5) - 0.5)): F.interpolate is Dh^T G Dw.
    span: the [begin, end) of each row's non-zeros; tspan[k, p]: the [begin, end) of the cells of scale k that pixel p touches."""
    import numpy as np
    scales = check_pool_scales(scales)
    if kind not in ('pool', 'bilinear'):
        raise ValueError(kind)
    rows = []
    for s in scales:
        d = np.zeros((s, n), np.float64)
        if kind == 'pool':
            for i in range(s):
                a, b = (i * n) // s, -((-(i + 1) * n) // s)
                d[i, a:b] = 1.0 / (b - a)
        else:
            src = np.maximum(0.0, (s / n) * (np.arange(n, dtype=np.float64) + 0.5) - 0.5)
            i0 = np.minimum(src.astype(np.int64), s - 1)
            i1 = i0 + (i0 < s - 1)
            l1 = src - i0
            np.add.at(d, (i0, np.arange(n)), 1.0 - l1)
            np.add.at(d, (i1, np.arange(n)), l1)
        rows.append(d)
    dense = np.concatenate(rows, 0)

    def spans(m):            # per row of m: [first non-zero, last non-zero + 1); the non-zeros of a row are one run, possibly with exact zeros inside
        nz = m != 0
        some = nz.any(1)                      # (a grid finer than the plane it is resized to has cells that no pixel reads: an empty span)
        lo = np.where(some, nz.argmax(1), 0)
        hi = np.where(some, m.shape[1] - nz[:, ::-1].argmax(1), 0)
        return np.stack([lo, hi], 1).astype(np.int32)
    span = spans(dense)
    tspan = np.stack([spans(d.T) for d in rows], 0)
    return dense, span, tspan


def _pyramid_dev_tables(kind, h, w, scales, dev):
    key = (kind, h, w, scales, str(dev))
    t = _pyramid_tables.get(key)
    if t is None:
        import numpy as np
        if len(_pyramid_tables) >= 64:
            _pyramid_tables.clear()
        t = []
        for axis, n in (('h', h), ('w', w)):
            dense, span, tspan = pyramid_operator(kind, n, scales)
            for name, arr in (('op', dense.astype(np.float32)), ('span', span), ('tspan', tspan)):
                t.append(h2d_small(torch.from_numpy(np.ascontiguousarray(arr)), dev, ('pyramid', name, axis)))
        t = _pyramid_tables[key] = tuple(t)           # (op_h, span_h, tspan_h, op_w, span_w, tspan_w)
    return t


def _pyr_ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _pyramid_reduce(kind, x, c, scales, chan_off, shared, out=None):
    scales = check_pool_scales(scales)
    n, _, h, w = x.shape
    bs = _bs(x)
    op_h, span_h, _, op_w, span_w, _ = _pyramid_dev_tables(kind, h, w, scales, x.device)
    cells = n * c * sum(s * s for s in scales)
    flat = torch.empty(cells, device=x.device) if out is None else _dense(out)
    if flat.dim() != 1 or flat.numel() != cells:
        raise ValueError(f'out must be a flat tensor of {cells} floats, got {tuple(flat.shape)}')
    outs, o = [], 0
    for s in scales:
        outs.append(flat[o:o + n * c * s * s].view(n, c, s, s))
        o += n * c * s * s
    call('pfst_pyramid_reduce', x.data_ptr(), bs, n, c, h, w, len(scales), _pyr_ints(scales), _pyr_ints(chan_off), int(shared), op_h.data_ptr(),
         op_w.data_ptr(), span_h.data_ptr(), span_w.data_ptr(), _ptr_array(outs), _stream())
    return outs


def _pyramid_expand(kind, grids, scales, chan_off, sliced, out, c, add, accumulate, amax):
    scales = check_pool_scales(scales)
    n, _, h, w = out.shape
    if len(grids) != len(scales) or any(tuple(g.shape) != (n, c, s, s) for g, s in zip(grids, scales)):
        raise ValueError(f'pyramid grids {[tuple(g.shape) for g in grids]} for scales {scales}, N = {n}, C = {c}')
    _, _, tspan_h, _, _, tspan_w = t = _pyramid_dev_tables(kind, h, w, scales, out.device)
    call('pfst_pyramid_expand', _ptr_array([_dense(g) for g in grids]), n, c, h, w, len(scales), _pyr_ints(scales), _pyr_ints(chan_off), int(sliced),
         out.data_ptr(), _bs(out), _p(add), 0 if add is None else _bs(add), int(accumulate), t[0].data_ptr(), t[3].data_ptr(), tspan_h.data_ptr(),
         tspan_w.data_ptr(), _p(amax), _stream())
    return out


def pyramid_pool(x, scales, out=None):
    """[F.adaptive_avg_pool2d(x, s) for s in scales] in ONE launch that reads x once: -> list of dense [N, C, s, s] (views of one allocation,
    or of the flat tensor `out` of N C sum(s^2) floats).  x may be a channel slice of a wider NCHW buffer."""
    return _pyramid_reduce('pool', x, x.shape[1], scales, [0] * len(scales), True, out)


def pyramid_pool_bwd(grads, scales, out, accumulate=False, add=None):
    """the adjoint of pyramid_pool, all scales in one pass: out = (accumulate ? out : 0) + (add if given) + sum_k pool_k^T(grads[k]).
    `add`: a tensor shaped like out (a slice of a concat gradient: the identity branch beside the pyramid) -- dL/dx is written once"""
    if add is not None and tuple(add.shape) != tuple(out.shape):
        raise ValueError(f'add {tuple(add.shape)} for out {tuple(out.shape)}')
    return _pyramid_expand('pool', grads, scales, [0] * len(scales), False, out, out.shape[1], add, accumulate, None)


def pyramid_upsample(grids, scales, out, amax=None):
    """out[:, k C:(k + 1) C] = F.interpolate(grids[k], out.shape[2:], mode='bilinear', align_corners=False) for every k in one launch; out: a
    [N, K C, H, W] dense-plane view (the pyramid's slices of the concat buffer).  amax: the slot group that receives max |out|"""
    c = grids[0].shape[1]
    if out.shape[1] != c * len(grids):
        raise ValueError(f'{len(grids)} grids of {c} channels into {out.shape[1]} channels')
    return _pyramid_expand('bilinear', grids, scales, [k * c for k in range(len(grids))], True, out, c, None, False, amax)


def pyramid_upsample_bwd(dy, scales, out=None):
    """the adjoint of pyramid_upsample: dy [N, K C, H, W] (dense planes) -> list of dense [N, C, s, s] (out: as for pyramid_pool), one launch"""
    k = len(scales)
    if dy.shape[1] % k:
        raise ValueError(f'{dy.shape[1]} channels for {k} scales')
    c = dy.shape[1] // k
    return _pyramid_reduce('bilinear', dy, c, scales, [i * c for i in range(k)], False, out)


def copy_planes(x, out, accumulate=False, amax=None):
    """out[...] = (accumulate ? out : 0) + x between two dense-plane NCHW views of equal shape (a tensor into its slice of a concat buffer); amax: the slot group that
    receives max |x|"""
    if tuple(x.shape) != tuple(out.shape):
        raise ValueError(f'copy_planes: {tuple(x.shape)} into {tuple(out.shape)}')
    n, c, h, w = x.shape
    call('pfst_copy_planes', x.data_ptr(), _bs(x), out.data_ptr(), _bs(out), n, c * h * w, int(accumulate), _p(amax), _stream())
    return out


# ---------------------------------------------------------------- feature-pyramid top-down path (csrc/fpn.hip)
FPN_MAX_LEVELS = 3          # PFST_FPN_MAX_LEVELS
MERGE_ROUTES = ('pixel', 'quad', 'half')          # pfst_topdown_merge_route: one pixel per thread, four with 16-byte accesses, the exact-1/2 walk


def _i64s(vals):
    return (ctypes.c_longlong * len(vals))(*[int(v) for v in vals])


def _merge_shapes(lat, coarse):
    n, c, hf, wf = lat.shape
    if coarse.dim() != 4 or tuple(coarse.shape[:2]) != (n, c) or coarse.shape[2] > hf or coarse.shape[3] > wf:
        raise ValueError(f'topdown_merge: coarse {tuple(coarse.shape)} under lateral {tuple(lat.shape)} (same N, C; a grid no finer)')
    return n, c, coarse.shape[2], coarse.shape[3], hf, wf


def topdown_merge(lat, coarse, out=None, amax=None):
    """out = lat + F.interpolate(coarse, lat.shape[2:], mode='bilinear', align_corners=False) in one pass: the value of resize_bilinear and one
    fp32 add, bit for bit.  lat, coarse, out: dense-plane NCHW views; out (default: a new tensor) must not be lat -- the lateral layer's backward
    still reads it.  amax: the slot group that receives max |out|.  Adjoint: d_lat = d_out, d_coarse (+)= resize_bilinear_bwd(d_out)."""
    n, c, hc, wc, hf, wf = _merge_shapes(lat, coarse)
    if out is None:
        out = torch.empty(n, c, hf, wf, device=lat.device)
    if tuple(out.shape) != tuple(lat.shape):
        raise ValueError(f'topdown_merge: out {tuple(out.shape)} for lateral {tuple(lat.shape)}')
    call('pfst_topdown_merge', lat.data_ptr(), _bs(lat), coarse.data_ptr(), _bs(coarse), out.data_ptr(), _bs(out), n, c, hc, wc, hf, wf, _p(amax),
         _stream())
    return out


def topdown_merge_route(lat, coarse, out):
    """the form pfst_topdown_merge takes for these operands, one of MERGE_ROUTES (no launch)"""
    _, _, hc, wc, hf, wf = _merge_shapes(lat, coarse)
    return MERGE_ROUTES[lib().pfst_topdown_merge_route(lat.data_ptr(), _bs(lat), coarse.data_ptr(), _bs(coarse), out.data_ptr(), _bs(out), hc, wc, hf, wf)]


def _fpn_levels(name, wide, levels, chan_off):
    """checks of the K level tensors against the wide buffer -> (N, C, Hf, Wf, chan_off)"""
    n, cw, hf, wf = wide.shape
    k = len(levels)
    if not 1 <= k <= FPN_MAX_LEVELS:
        raise NotImplementedError(f'{name}: 1 to {FPN_MAX_LEVELS} levels per launch, got {k}')
    c = levels[0].shape[1]
    chan_off = [i * c for i in range(k)] if chan_off is None else [int(o) for o in chan_off]
    if len(chan_off) != k or any(o < 0 or o + c > cw for o in chan_off):
        raise ValueError(f'{name}: channel offsets {chan_off} of {c}-channel slices in {cw} channels')
    for t in levels:
        if t.dim() != 4 or tuple(t.shape[:2]) != (n, c) or t.shape[2] > hf or t.shape[3] > wf:
            raise ValueError(f'{name}: level {tuple(t.shape)} for a buffer {tuple(wide.shape)} (N = {n}, C = {c}; grids no finer than the buffer)')
    return n, c, hf, wf, chan_off


def fpn_resize_concat(srcs, out, chan_off=None, amax=None):
    """out[:, chan_off[k]:chan_off[k] + C] = F.interpolate(srcs[k], out.shape[2:], mode='bilinear', align_corners=False) for up to three maps in
    ONE launch, each bit-identical to resize_bilinear(srcs[k], out=that slice).  out: a dense-plane NCHW view (the concat buffer, or its tail);
    chan_off: default k C.  amax: the slot group that receives max |.| over everything written."""
    n, c, hf, wf, chan_off = _fpn_levels('fpn_resize_concat', out, srcs, chan_off)
    call('pfst_fpn_resize_concat', _ptr_array(srcs), _i64s([_bs(s) for s in srcs]), _pyr_ints([s.shape[2] for s in srcs]),
         _pyr_ints([s.shape[3] for s in srcs]), _pyr_ints(chan_off), len(srcs), out.data_ptr(), _bs(out), n, c, hf, wf, _p(amax), _stream())
    return out


def fpn_resize_concat_route(out):
    """1: the concat launch moves `out` in 16-byte accesses, 0: pixel by pixel"""
    return lib().pfst_fpn_resize_concat_route(out.data_ptr(), _bs(out), out.shape[2], out.shape[3])


def fpn_resize_concat_bwd(dy, outs, chan_off=None, accumulate=False):
    """the adjoint of fpn_resize_concat in one launch: outs[k] = (accumulate[k] ? outs[k] : 0) + resize_bilinear_bwd(dy[:, chan_off[k]:chan_off[k] + C]),
    each bit-identical to resize_bilinear_bwd on that slice.  accumulate: one flag, or one per level"""
    n, c, hf, wf, chan_off = _fpn_levels('fpn_resize_concat_bwd', dy, outs, chan_off)
    acc = [bool(accumulate)] * len(outs) if isinstance(accumulate, (bool, int)) else [bool(a) for a in accumulate]
    if len(acc) != len(outs):
        raise ValueError(f'fpn_resize_concat_bwd: {len(acc)} accumulate flags for {len(outs)} levels')
    call('pfst_fpn_resize_concat_bwd', dy.data_ptr(), _bs(dy), _ptr_array(outs), _i64s([_bs(o) for o in outs]), _pyr_ints([o.shape[2] for o in outs]),
         _pyr_ints([o.shape[3] for o in outs]), _pyr_ints(chan_off), _pyr_ints(acc), len(outs), n, c, hf, wf, _stream())
    return outs


def fpn_resize_concat_bwd_routes(dy, outs, chan_off=None):
    """per level: 1 the x2 gather on 2 x 2 blocks, 0 the generic gather"""
    _, c, hf, wf, chan_off = _fpn_levels('fpn_resize_concat_bwd', dy, outs, chan_off)
    return [lib().pfst_fpn_resize_concat_bwd_route(dy[:, o:o + c].data_ptr(), _bs(dy), t.data_ptr(), _bs(t), t.shape[2], t.shape[3], hf, wf)
            for o, t in zip(chan_off, outs)]


# ---------------------------------------------------------------- Semantic FPN: nearest top-down merge, level sum (csrc/fpn.hip)
MERGE_NEAREST_ROUTES = ('pixel', 'quad', 'double')   # pfst_topdown_merge_nearest_route: one pixel per thread, four with 16-byte accesses, the exact x2 form
NEAREST_BWD_ROUTES = ('gather', 'double')            # pfst_nearest_resize_bwd_route: the generic gather, x2 on 2 x 2 blocks
UPSAMPLE2X_ROUTES = ('pixel', 'walk')                # pfst_upsample2x_norm_route
LEVEL_SUM_ROUTES = ('pixel', 'quad')                 # pfst_fpn_level_sum_route: quad = the x2 walk (K >= 1) or a flat pass (K = 0), 16-byte accesses


def nearest_src_index(n_out, n_in):
    """the source index of every output index under torch's legacy 'nearest' for a given output size, as pfst_topdown_merge_nearest forms it:
    min((int)floorf(dst * scale), n_in - 1) with scale = (float)n_in / (float)n_out, every step in fp32.  NumPy int64 [n_out], no device."""
    import numpy as np
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1)


def topdown_merge_nearest(lat, coarse, out=None, amax=None):
    """out = lat + F.interpolate(coarse, lat.shape[2:], mode='nearest') in one pass, bit for bit (one rounded fp32 add).  Operands as for
    topdown_merge.  Adjoint: d_lat = d_out, d_coarse (+)= nearest_resize_bwd(d_out)."""
    n, c, hc, wc, hf, wf = _merge_shapes(lat, coarse)
    if out is None:
        out = torch.empty(n, c, hf, wf, device=lat.device)
    if tuple(out.shape) != tuple(lat.shape):
        raise ValueError(f'topdown_merge_nearest: out {tuple(out.shape)} for lateral {tuple(lat.shape)}')
    call('pfst_topdown_merge_nearest', lat.data_ptr(), _bs(lat), coarse.data_ptr(), _bs(coarse), out.data_ptr(), _bs(out), n, c, hc, wc, hf, wf,
         _p(amax), _stream())
    return out


def topdown_merge_nearest_route(lat, coarse, out):
    """the form pfst_topdown_merge_nearest takes for these operands, one of MERGE_NEAREST_ROUTES (no launch)"""
    _, _, hc, wc, hf, wf = _merge_shapes(lat, coarse)
    return MERGE_NEAREST_ROUTES[lib().pfst_topdown_merge_nearest_route(lat.data_ptr(), _bs(lat), coarse.data_ptr(), _bs(coarse), out.data_ptr(),
                                                                        _bs(out), hc, wc, hf, wf)]


def _nearest_bwd_shapes(dy, in_hw, out):
    n, c, hf, wf = dy.shape
    hc, wc = int(in_hw[0]), int(in_hw[1])
    if not (1 <= hc <= hf and 1 <= wc <= wf):
        raise ValueError(f'nearest_resize_bwd: a source grid {(hc, wc)} under dy {tuple(dy.shape)} (no finer than it)')
    if out is not None and tuple(out.shape) != (n, c, hc, wc):
        raise ValueError(f'nearest_resize_bwd: out {tuple(out.shape)}, expected {(n, c, hc, wc)}')
    return n, c, hc, wc, hf, wf


def nearest_resize_bwd(dy, in_hw, out=None, accumulate=False):
    """the adjoint of F.interpolate(x [N, C, *in_hw], dy.shape[2:], mode='nearest'): out[s] = (accumulate ? out[s] : 0) + sum of dy over the
    pre-image of s, a plain fp32 sum in ascending row, then column order (deterministic, no atomics)"""
    n, c, hc, wc, hf, wf = _nearest_bwd_shapes(dy, in_hw, out)
    if out is None:
        if accumulate:
            raise ValueError('nearest_resize_bwd: accumulate needs out')
        out = torch.empty(n, c, hc, wc, device=dy.device)
    call('pfst_nearest_resize_bwd', dy.data_ptr(), _bs(dy), out.data_ptr(), _bs(out), n, c, hc, wc, hf, wf, int(bool(accumulate)), _stream())
    return out


def nearest_resize_bwd_route(dy, out):
    n, c, hc, wc, hf, wf = _nearest_bwd_shapes(dy, out.shape[2:], out)
    return NEAREST_BWD_ROUTES[lib().pfst_nearest_resize_bwd_route(dy.data_ptr(), _bs(dy), out.data_ptr(), _bs(out), hc, wc, hf, wf)]


def _coef_ptr(coef, c, name):
    if coef is None:
        return 0
    _chk(coef, F32, 2)
    if tuple(coef.shape) != (c, 4) or not coef.is_contiguous():
        raise ValueError(f'{name}: a coefficient table is a contiguous [C, 4] tensor (mean, invstd, sc, sh), got {tuple(coef.shape)} for C = {c}')
    return coef.data_ptr()


def upsample2x_norm(pre, coef=None, out=None, amax=None):
    """out = F.interpolate(relu(pre * sc + sh), scale 2, mode='bilinear', align_corners=False) with (sc, sh) = coef[:, 2], coef[:, 3] (the lazy
    record of conv_bn_act; None: pre holds final values), bit-identical to bn_apply + resize_bilinear.  amax: the slot group that receives
    max |out|.  Adjoint: resize_bilinear_bwd."""
    n, c, hc, wc = pre.shape
    if out is None:
        out = torch.empty(n, c, 2 * hc, 2 * wc, device=pre.device)
    if tuple(out.shape) != (n, c, 2 * hc, 2 * wc):
        raise ValueError(f'upsample2x_norm: out {tuple(out.shape)} for a source {tuple(pre.shape)}')
    call('pfst_upsample2x_norm', pre.data_ptr(), _bs(pre), _coef_ptr(coef, c, 'upsample2x_norm'), out.data_ptr(), _bs(out), n, c, hc, wc, _p(amax),
         _stream())
    return out


def upsample2x_norm_route(pre, out):
    return UPSAMPLE2X_ROUTES[lib().pfst_upsample2x_norm_route(pre.data_ptr(), _bs(pre), out.data_ptr(), _bs(out), pre.shape[2], pre.shape[3])]


def _level_sum_args(pre0, members, coefs, addend, out):
    n, c, h0, w0 = pre0.shape
    k = len(members)
    if k > FPN_MAX_LEVELS:
        raise NotImplementedError(f'fpn_level_sum: up to {FPN_MAX_LEVELS} half-grid members per launch, got {k}')
    coefs = [None] * k if coefs is None else list(coefs)
    if len(coefs) != k:
        raise ValueError(f'fpn_level_sum: {len(coefs)} tables for {k} members')
    for m in members:
        if m.dim() != 4 or tuple(m.shape) != (n, c, h0 // 2, w0 // 2) or h0 % 2 or w0 % 2:
            raise ValueError(f'fpn_level_sum: member {tuple(m.shape)} is not on exactly half of level 0 {tuple(pre0.shape)}')
    for t, what in ((addend, 'addend'), (out, 'out')):
        if t is not None and tuple(t.shape) != tuple(pre0.shape):
            raise ValueError(f'fpn_level_sum: {what} {tuple(t.shape)} for level 0 {tuple(pre0.shape)}')
    return n, c, h0, w0, k, coefs


def fpn_level_sum(pre0, coef0, members=(), coefs=None, addend=None, out=None, amax=None):
    """out = act0(pre0) + resize_x2((act1(members[0]) + act2(members[1])) + act3(members[2])) [+ addend] in ONE launch, summed in that order:
    bit-identical to bn_apply per operand, the fp32 adds on the half grid, resize_bilinear, one add, one more for the addend.  act_k normalises
    on load from the [C, 4] table coef0 / coefs[k] (None: final values).  members: 0 to 3 maps on exactly half of pre0's grid.  amax: the slot
    group that receives max |out|."""
    members = list(members)
    n, c, h0, w0, k, coefs = _level_sum_args(pre0, members, coefs, addend, out)
    if out is None:
        out = torch.empty(n, c, h0, w0, device=pre0.device)
    call('pfst_fpn_level_sum', pre0.data_ptr(), _bs(pre0), _coef_ptr(coef0, c, 'fpn_level_sum'), _ptr_array(members),
         _i64s([_bs(m) for m in members]), (ctypes.c_void_p * k)(*[_coef_ptr(t, c, 'fpn_level_sum') for t in coefs]), k, _p(addend),
         0 if addend is None else _bs(addend), out.data_ptr(), _bs(out), n, c, h0, w0, _p(amax), _stream())
    return out


def fpn_level_sum_route(pre0, members, addend, out):
    members = list(members)
    n, c, h0, w0, k, _ = _level_sum_args(pre0, members, None, addend, out)
    return LEVEL_SUM_ROUTES[lib().pfst_fpn_level_sum_route(pre0.data_ptr(), _bs(pre0), _ptr_array(members), _i64s([_bs(m) for m in members]), k,
                                                           _p(addend), 0 if addend is None else _bs(addend), out.data_ptr(), _bs(out), h0, w0)]


# ---------------------------------------------------------------- HRNet's exchange unit (csrc/hrnet.hip)
HR_MAX_BRANCHES = 4         # PFST_HR_MAX_BRANCHES
HR_FUSE_ROUTES = ('pixel', 'quad')                   # pfst_hr_fuse_route: one pixel per thread, four with 16-byte accesses
HR_RATIOS = (2, 4, 8)


def hr_fuse_exact(out_hw, op_hw):
    """an operand on grid op_hw can enter the fused exchange for an output on out_hw: the same grid, or out_hw / r exactly, r in HR_RATIOS"""
    return any(op_hw[0] * r == out_hw[0] and op_hw[1] * r == out_hw[1] for r in (1,) + HR_RATIOS)


def _hr_fuse_args(ops, coefs, out):
    n, c, hf, wf = out.shape
    ops = list(ops)
    coefs = [None] * len(ops) if coefs is None else list(coefs)
    if not 1 <= len(ops) <= HR_MAX_BRANCHES or len(coefs) != len(ops):
        raise ValueError(f'hr_fuse: 1 to {HR_MAX_BRANCHES} operands with one table (or None) each, got {len(ops)} and {len(coefs)}')
    for t in ops:
        if t.dim() != 4 or tuple(t.shape[:2]) != (n, c) or not hr_fuse_exact((hf, wf), t.shape[2:]):
            raise ValueError(f'hr_fuse: operand {tuple(t.shape)} for an output {tuple(out.shape)} (same N, C; the same grid or exactly 1/2, 1/4, 1/8 of it)')
    if sum(tuple(t.shape[2:]) != (hf, wf) for t in ops) > FPN_MAX_LEVELS:
        raise NotImplementedError(f'hr_fuse: up to {FPN_MAX_LEVELS} coarser operands per launch')
    return n, c, hf, wf, ops, coefs


def hr_fuse(ops, coefs=None, out=None, out_hw=None, amax=None):
    """out = relu(((t_0 + t_1) + t_2) + t_3) in ONE launch, the operands in the order given (hrnet.py:199-213).  ops[j] on out's grid: its values,
    or pre * sc + sh under a [C, 4] table coefs[j] (no ReLU); ops[j] on exactly 1/2, 1/4 or 1/8 of it: the bilinear (align_corners=False)
    interpolation of its (normalised) values.  Bit-identical to bn_apply(relu=False) per tabled operand, resize_bilinear per coarser one, the fp32
    adds in that order and a ReLU.  out: default a new tensor on out_hw (default: ops[0]'s grid).  amax: the slot group that receives max |out|."""
    if out is None:
        hw = tuple(ops[0].shape[2:]) if out_hw is None else tuple(out_hw)
        out = torch.empty(ops[0].shape[0], ops[0].shape[1], hw[0], hw[1], device=ops[0].device)
    n, c, hf, wf, ops, coefs = _hr_fuse_args(ops, coefs, out)
    call('pfst_hr_fuse', _ptr_array(ops), _i64s([_bs(t) for t in ops]), (ctypes.c_void_p * len(ops))(*[_coef_ptr(t, c, 'hr_fuse') for t in coefs]),
         _pyr_ints([t.shape[2] for t in ops]), _pyr_ints([t.shape[3] for t in ops]), len(ops), out.data_ptr(), _bs(out), n, c, hf, wf, _p(amax),
         _stream())
    return out


def hr_fuse_route(ops, out):
    """the form pfst_hr_fuse takes for these operands, one of HR_FUSE_ROUTES (no launch)"""
    n, c, hf, wf, ops, _ = _hr_fuse_args(ops, None, out)
    return HR_FUSE_ROUTES[lib().pfst_hr_fuse_route(_ptr_array(ops), _i64s([_bs(t) for t in ops]), _pyr_ints([t.shape[2] for t in ops]),
                                                   _pyr_ints([t.shape[3] for t in ops]), len(ops), out.data_ptr(), _bs(out), hf, wf)]


def hr_fuse_bwd(d_out, out, coarse=(), accumulate=False, gy=None):
    """the adjoint of hr_fuse in at most two launches.  Returns gy = d_out where out > 0, else 0 -- the upstream gradient of every operand on the
    output grid (gy: the buffer to write, default a new tensor; d_out itself is allowed) -- after coarse[k] = (accumulate[k] ? coarse[k] : 0) +
    resize_bilinear_bwd(gy) for the coarser operands' gradient buffers, all in one gather launch, each bit-identical to resize_bilinear_bwd.
    accumulate: one flag, or one per coarse buffer"""
    n, c, hf, wf = out.shape
    coarse = list(coarse)
    if tuple(d_out.shape) != tuple(out.shape) or (gy is not None and tuple(gy.shape) != tuple(out.shape)):
        raise ValueError(f'hr_fuse_bwd: d_out {tuple(d_out.shape)} / gy for an output {tuple(out.shape)}')
    if len(coarse) > FPN_MAX_LEVELS:
        raise NotImplementedError(f'hr_fuse_bwd: up to {FPN_MAX_LEVELS} coarser operands per launch')
    for t in coarse:
        if t.dim() != 4 or tuple(t.shape[:2]) != (n, c) or tuple(t.shape[2:]) == (hf, wf) or not hr_fuse_exact((hf, wf), t.shape[2:]):
            raise ValueError(f'hr_fuse_bwd: gradient buffer {tuple(t.shape)} under an output {tuple(out.shape)} (exactly 1/2, 1/4, 1/8 of its grid)')
    acc = [bool(accumulate)] * len(coarse) if isinstance(accumulate, (bool, int)) else [bool(a) for a in accumulate]
    if len(acc) != len(coarse):
        raise ValueError(f'hr_fuse_bwd: {len(acc)} accumulate flags for {len(coarse)} buffers')
    if gy is None:
        gy = torch.empty(n, c, hf, wf, device=out.device)
    call('pfst_hr_fuse_bwd', d_out.data_ptr(), _bs(d_out), out.data_ptr(), _bs(out), gy.data_ptr(), _bs(gy), _ptr_array(coarse),
         _i64s([_bs(t) for t in coarse]), _pyr_ints([t.shape[2] for t in coarse]), _pyr_ints([t.shape[3] for t in coarse]), _pyr_ints(acc),
         len(coarse), n, c, hf, wf, _stream())
    return gy


def upsample_nearest(x, factor):
    _dense(x)
    n, c, h, w = x.shape
    y = torch.empty(n, c, h * factor, w * factor, device=x.device)
    call('pfst_upsample_nearest', x.data_ptr(), y.data_ptr(), n * c, h, w, factor, _stream())
    return y


def upsample_nearest_bwd(dy, factor):
    _dense(dy)
    n, c, H, W = dy.shape
    dx = torch.empty(n, c, H // factor, W // factor, device=dy.device)
    call('pfst_upsample_nearest_bwd', dy.data_ptr(), dx.data_ptr(), n * c, H // factor, W // factor, factor, _stream())
    return dx


def channel_scale(x, mask):
    _dense(x)
    n, c, h, w = x.shape
    assert mask.numel() == n * c
    y = torch.empty_like(x)
    call('pfst_channel_scale', x.data_ptr(), _dense(mask).data_ptr(), y.data_ptr(), n, c, h * w, _stream())
    return y


# ---------------------------------------------------------------- test-time inference (sliding windows, flips, averaging)
def softmax_nchw(x, out=None):
    """F.softmax(x, dim=1) of an NCHW tensor (dense planes)"""
    n, c, h, w = x.shape
    if out is None:
        out = torch.empty(n, c, h, w, device=x.device)
    call('pfst_softmax_nchw', x.data_ptr(), _bs(x), out.data_ptr(), _bs(out), n, c, h * w, _stream())
    return out


def window_accumulate_(preds, count, crop, y1, x1):
    """preds[:, :, y1:y1+hc, x1:x1+wc] += crop; count[:, :, y1:.., x1:..] += 1 (encoder_decoder.py:246-250)"""
    _dense(preds), _dense(count), _dense(crop)
    n, c, h, w = preds.shape
    hc, wc = crop.shape[-2:]
    assert crop.shape[:2] == (n, c) and count.numel() == n * h * w
    call('pfst_window_accumulate', crop.data_ptr(), preds.data_ptr(), count.data_ptr(), n, c, hc, wc, h, w, int(y1), int(x1), _stream())


def window_normalize_(preds, count):
    _dense(preds), _dense(count)
    n, c, h, w = preds.shape
    call('pfst_window_normalize', preds.data_ptr(), count.data_ptr(), n, c, h * w, _stream())
    return preds


def argmax_nchw(x):
    """x.argmax(dim=1) as uint8 [N, H, W] (first maximal class; the first NaN class where a pixel holds one, as torch.argmax)"""
    n, c, h, w = x.shape
    lab = torch.empty(n, h, w, dtype=U8, device=x.device)
    call('pfst_argmax_nchw', x.data_ptr(), _bs(x), lab.data_ptr(), n, c, h * w, _stream())
    return lab


def flip_planes(x, horizontal=False, vertical=False):
    """x.flip(dims=(3,)) / (2,) of a dense NCHW tensor, out of place"""
    _dense(x)
    n, c, h, w = x.shape
    y = torch.empty_like(x)
    call('pfst_flip_planes', x.data_ptr(), y.data_ptr(), n * c, h, w, int(horizontal), int(vertical), _stream())
    return y


def div_scalar_(x, d):
    _dense(x)
    call('pfst_div_scalar', x.data_ptr(), x.numel(), float(d), _stream())
    return x


TTA_MAX_C = 32          # PFST_TTA_MAX_C: classes held in registers by pfst_tta_accumulate


def tta_accumulate_(acc, src, mid_hw, hflip=False, vflip=False, accumulate=True):
    """acc (dense [N, C, Ho, Wo]) = (acc if accumulate else 0) + flip(softmax(resize(resize(src, mid_hw), (Ho, Wo)))), bit for bit what
    resize_bilinear -> resize_bilinear -> softmax_nchw -> flip_planes -> axpy_ computes; a resize between equal sizes is skipped.
    src: [N, C, Hs, Ws] (dense planes); C <= TTA_MAX_C"""
    _dense(acc)
    n, c, hs, ws = src.shape
    assert acc.shape[:2] == (n, c), (tuple(acc.shape), tuple(src.shape))
    ho, wo = acc.shape[2:]
    call('pfst_tta_accumulate', src.data_ptr(), _bs(src), n, c, hs, ws, int(mid_hw[0]), int(mid_hw[1]), ho, wo, int(bool(hflip)),
         int(bool(vflip)), acc.data_ptr(), int(bool(accumulate)), _stream())
    return acc


def tta_finalize(acc, views):
    """(acc / views).argmax(dim=1) as uint8 [N, H, W]: labels equal to div_scalar_ + argmax_nchw's; acc is left as it is"""
    _dense(acc)
    n, c, h, w = acc.shape
    lab = torch.empty(n, h, w, dtype=U8, device=acc.device)
    call('pfst_tta_finalize', acc.data_ptr(), n, c, h * w, int(views), lab.data_ptr(), _stream())
    return lab


# ---------------------------------------------------------------- whole-scene prediction (pfst_amd/scene.py)
SCENE_MAX_WINDOWS = 16          # PFST_SCENE_MAX_WINDOWS: window offsets that travel by value with one launch


def _win_yx(windows):
    """[(y1, x1), ...] -> a host int array for the C ABI (copied into the kernel arguments by the entry point: no device copy)"""
    if not 1 <= len(windows) <= SCENE_MAX_WINDOWS:
        raise ValueError(f'1 .. {SCENE_MAX_WINDOWS} windows per launch, got {len(windows)}')
    flat = [int(v) for yx in windows for v in yx]
    return (ctypes.c_int * len(flat))(*flat)


def scene_windows(scene_u8, windows, size, mean, std, to_rgb, out=None):
    """the windows [(y1, x1), ...] of size (h, w) of a device uint8 [H, W, 3] scene (BGR as read), normalised as pipeline.normalize does
    ((BGR -> RGB,) subtract mean, divide by std, fp32) -> float32 [B, 3, h, w], bit for bit"""
    _dense(scene_u8, U8)
    if scene_u8.dim() != 3 or scene_u8.shape[2] != 3 or len(mean) != 3 or len(std) != 3:
        raise ValueError(f'scene must be [H, W, 3] with three means / stds, got {tuple(scene_u8.shape)}')
    H, W = scene_u8.shape[:2]
    h, w = int(size[0]), int(size[1])
    b = len(windows)
    if out is None:
        out = torch.empty(b, 3, h, w, device=scene_u8.device)
    assert tuple(_dense(out).shape) == (b, 3, h, w)
    call('pfst_scene_windows', scene_u8.data_ptr(), H, W, _win_yx(windows), b, h, w, float(mean[0]), float(mean[1]), float(mean[2]),
         float(std[0]), float(std[1]), float(std[2]), int(bool(to_rgb)), out.data_ptr(), _stream())
    return out


def scene_accumulate_(sums, logits, windows, size):
    """sums (dense [C, H, W]) += the low-resolution logits [B, C, hl, wl] of the windows [(y1, x1), ...] of size (h, w), each resized to
    (h, w) and added in place, window by window in index order: bit for bit resize_bilinear + window_accumulate_ per window"""
    _dense(sums)
    b, c, hl, wl = logits.shape
    if sums.dim() != 3 or sums.shape[0] != c or b != len(windows):
        raise ValueError(f'sums {tuple(sums.shape)} / logits {tuple(logits.shape)} / {len(windows)} windows do not match')
    call('pfst_scene_accumulate', logits.data_ptr(), _bs(logits), b, c, hl, wl, _win_yx(windows), int(size[0]), int(size[1]),
         sums.data_ptr(), sums.shape[1], sums.shape[2], _stream())
    return sums


def scene_finalize(sums, row_count, col_count, confidence=False, return_probs=False):
    """sums [C, H, W] / (row_count[y] * col_count[x]) -> softmax -> first maximal class: (labels uint8 [H, W], confidence uint8 [H, W] =
    rint(p_max * 255) or None, probabilities [C, H, W] or None), bit for bit window_normalize_ -> softmax_nchw -> argmax_nchw"""
    _dense(sums)
    c, h, w = sums.shape
    I32 = torch.int32
    if _dense(row_count, I32).numel() != h or _dense(col_count, I32).numel() != w:
        raise ValueError('row_count / col_count must hold H / W entries')
    dev = sums.device
    lab = torch.empty(h, w, dtype=U8, device=dev)
    conf = torch.empty(h, w, dtype=U8, device=dev) if confidence else None
    probs = torch.empty(c, h, w, device=dev) if return_probs else None
    call('pfst_scene_finalize', sums.data_ptr(), c, h, w, row_count.data_ptr(), col_count.data_ptr(), lab.data_ptr(), _p(conf), _p(probs),
         _stream())
    return lab, conf, probs


_resize_tables = {}


def _src_tables(n_out, n_in, dev):
    """pipeline._src_index of one axis on the device, uploaded once per (sizes, device): (int32 [2, n_out] lower / upper source index,
    float32 [n_out] weight of the upper one)"""
    import numpy as np
    from .pipeline import _src_index
    key = (n_out, n_in, str(dev))
    t = _resize_tables.get(key)
    if t is None:
        if len(_resize_tables) >= 32:
            _resize_tables.clear()
        lo, hi, f = _src_index(n_out, n_in)
        # through pinned staging buffers of their own (h2d_small, one tag per table): the upload does not make the host wait for the stream
        t = _resize_tables[key] = (h2d_small(torch.from_numpy(np.stack([lo, hi]).astype(np.int32)), dev, ('src_index', 'i') + key),
                                   h2d_small(torch.from_numpy(np.ascontiguousarray(f)), dev, ('src_index', 'f') + key))
    return t


def scene_resize_u8(scene_u8, out_hw, hflip=False, vflip=False):
    """device uint8 [h, w, 3] -> uint8 [Hr, Wr, 3]: pipeline.resize_bilinear_u8(scene, out_hw), mirrored horizontally / vertically when asked
    (np.flip of it along axis 1 / 0), bit for bit; with equal sizes an exact (mirrored) copy"""
    _dense(scene_u8, U8)
    if scene_u8.dim() != 3 or scene_u8.shape[2] != 3:
        raise ValueError(f'scene must be [H, W, 3], got {tuple(scene_u8.shape)}')
    h, w = scene_u8.shape[:2]
    hr, wr = int(out_hw[0]), int(out_hw[1])
    if hr < 1 or wr < 1:
        raise ValueError(f'resize to {out_hw}')
    dev = scene_u8.device
    yi, fy = _src_tables(hr, h, dev)
    xi, fx = _src_tables(wr, w, dev)
    out = torch.empty(hr, wr, 3, dtype=U8, device=dev)
    call('pfst_scene_resize_u8', scene_u8.data_ptr(), h, w, yi.data_ptr(), fy.data_ptr(), xi.data_ptr(), fx.data_ptr(), hr, wr, int(bool(hflip)),
         int(bool(vflip)), out.data_ptr(), _stream())
    return out


def scene_tta_accumulate_(acc, sums, row_count, col_count, hflip=False, vflip=False, accumulate=True):
    """acc (dense [C, H, W]) = (acc if accumulate else 0) + flip(softmax(resize(sums / (row_count[y] * col_count[x]), (H, W)))), bit for bit
    what window_normalize_ -> resize_bilinear (skipped between equal sizes) -> softmax_nchw -> flip_planes -> axpy_ computes from the view's
    window sums [C, Hr, Wr]; C <= TTA_MAX_C"""
    _dense(acc), _dense(sums)
    if acc.dim() != 3 or sums.dim() != 3 or acc.shape[0] != sums.shape[0]:
        raise ValueError(f'acc {tuple(acc.shape)} / sums {tuple(sums.shape)} do not match')
    c, hr, wr = sums.shape
    I32 = torch.int32
    if _dense(row_count, I32).numel() != hr or _dense(col_count, I32).numel() != wr:
        raise ValueError('row_count / col_count must hold the view\'s Hr / Wr entries')
    call('pfst_scene_tta_accumulate', sums.data_ptr(), c, hr, wr, row_count.data_ptr(), col_count.data_ptr(), int(bool(hflip)), int(bool(vflip)),
         acc.data_ptr(), acc.shape[1], acc.shape[2], int(bool(accumulate)), _stream())
    return acc


def scene_tta_finalize(acc, views, confidence=False, return_probs=False):
    """acc [C, H, W] / views -> first maximal class: (labels uint8 [H, W], confidence uint8 [H, W] = rint(p_max * 255) or None, probabilities
    [C, H, W] or None), bit for bit div_scalar_ -> argmax_nchw; acc is left as it is"""
    _dense(acc)
    if acc.dim() != 3:
        raise ValueError(f'acc must be [C, H, W], got {tuple(acc.shape)}')
    c, h, w = acc.shape
    dev = acc.device
    lab = torch.empty(h, w, dtype=U8, device=dev)
    conf = torch.empty(h, w, dtype=U8, device=dev) if confidence else None
    probs = torch.empty(c, h, w, device=dev) if return_probs else None
    call('pfst_scene_tta_finalize', acc.data_ptr(), c, h, w, int(views), lab.data_ptr(), _p(conf), _p(probs), _stream())
    return lab, conf, probs


def paint_labels(labels, palette, scene_u8=None, opacity=None):
    """labels uint8 [H, W] through palette (uint8 [<= 256, 3], RGB) -> uint8 [H, W, 3] RGB; with a scene (uint8 [H, W, 3], BGR) and an opacity
    in [0, 1] the blend of show_result, uint8(img * (1 - opacity) + colour * opacity) in double arithmetic: NumPy's bytes"""
    _dense(labels, U8), _dense(palette, U8)
    h, w = labels.shape
    if palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= 256:
        raise ValueError(f'palette must be [<= 256, 3], got {tuple(palette.shape)}')
    if (scene_u8 is None) != (opacity is None):
        raise ValueError('an overlay needs both the scene and an opacity')
    keep = op = 0.0
    if scene_u8 is not None:
        if tuple(_dense(scene_u8, U8).shape) != (h, w, 3):
            raise ValueError(f'scene {tuple(scene_u8.shape)} does not match labels {(h, w)}')
        op = float(opacity)
        if not 0.0 <= op <= 1.0:
            raise ValueError(f'opacity must lie in [0, 1], got {opacity}')
        keep = 1 - op                      # in double, as Python forms it in show_result
    out = torch.empty(h, w, 3, dtype=U8, device=labels.device)
    call('pfst_paint_labels', labels.data_ptr(), h, w, palette.data_ptr(), palette.shape[0], _p(scene_u8), keep, op, out.data_ptr(), _stream())
    return out


# ---------------------------------------------------------------- losses
def ce_upsample_fwd(logits, label_u8, pix_weight=None, class_weight=None, ignore_index=255):
    """-> (lse [N,H,W], acc float64[4] = (weighted nll sum, #correct, #valid, #labels outside [0,C) that are not ignore_index))"""
    _dense(logits), _dense(label_u8, U8)
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    assert label_u8.numel() == n * H * W
    if pix_weight is not None:
        assert _dense(pix_weight).numel() == n * H * W
    if class_weight is not None:
        assert _dense(class_weight).numel() == c
    lse = torch.empty(n, H, W, device=logits.device)
    acc = torch.zeros(4, dtype=F64, device=logits.device)
    call('pfst_ce_upsample_fwd', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), _p(pix_weight), _p(class_weight), H, W,
         ignore_index, lse.data_ptr(), acc.data_ptr(), _stream())
    return lse, acc


def ce_upsample_bwd(logits, label_u8, lse, scale, pix_weight=None, class_weight=None, ignore_index=255, out=None, accumulate=False):
    _dense(logits), _dense(label_u8, U8)                       # as ce_upsample_fwd: a view would be read as if it were dense
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    assert label_u8.numel() == n * H * W and lse.numel() == n * H * W
    if pix_weight is not None:
        assert _dense(pix_weight).numel() == n * H * W
    if class_weight is not None:
        assert _dense(class_weight).numel() == c
    if out is None:
        assert not accumulate
        out = torch.empty_like(logits)
    assert out.shape == logits.shape
    call('pfst_ce_upsample_bwd', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), _p(pix_weight), _p(class_weight), H, W,
         ignore_index, _dense(lse).data_ptr(), float(scale), _dense(out).data_ptr(), int(accumulate), _stream())
    return out


def ce_finalize(acc, numel, loss_weight):
    """-> float32[3] = (loss, acc_seg %, #invalid labels)"""
    out = torch.empty(3, device=acc.device)
    call('pfst_ce_finalize', acc.data_ptr(), float(numel), float(loss_weight), out.data_ptr(), _stream())
    return out


def _blocks_form(logits, label_u8, aligned8, generic):
    """the form rule of the fused up-sampling losses: 4 / 8 = the inter-cell block kernels of that ratio (C <= 8, H == S h, W == S w, label
    2-byte aligned and `aligned8` -- the tensor the family reads in pixel pairs, or None -- 8-byte aligned), 0 = the generic ones.
    -> (form, rows of partials per image)"""
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    for s, tile_rows in ((4, 32), (8, 16)):
        if (not generic and c <= 8 and H == s * h and W == s * w and label_u8.data_ptr() % 2 == 0 and h < 65535 * 15
                and (aligned8 is None or aligned8.data_ptr() % 8 == 0)):
            return s, ((w + 16) // 16) * ((h + tile_rows) // tile_rows)
    return 0, (H * W + 1023) // 1024


def dice_form(logits, label_u8, lse=None, generic=False):
    """which kernels a Dice term runs on: 4 / 8 = the inter-cell block kernels of that ratio (C <= 8, H == S h, W == S w, lse 8-byte and
    label 2-byte aligned), 0 = the generic ones; generic=True forces 0 (tests compare the two forms on one shape).
    -> (form, rows of partials per image)"""
    return _blocks_form(logits, label_u8, lse, generic)


def dice_upsample_fwd(logits, label_u8, ignore_index=255, head_ignore_index=255, exponent=2.0, lse=None, generic=False):
    """Per-workgroup partials of the Dice sums of softmax(up(logits)) and the head's accuracy counts; no atomics, a fixed order.
    lse: the CE term's log-sum-exp of the same logits (then nothing is written per pixel), or None (formed here: the same bits).
    -> (slab float64 [N, blocks, C, 2] = (I, P), counts int64 [N, blocks, C + 3] = (T per class, #correct, #valid, #bad), lse, form)"""
    _dense(logits), _dense(label_u8, U8)
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    assert label_u8.numel() == n * H * W
    if not float(exponent) >= 1.0:
        raise ValueError(f'DiceLoss: exponent must be >= 1 (p^(e-1) at p -> 0 is not finite below), got {exponent}')
    own = lse is None
    if own:
        lse = torch.empty(n, H, W, device=logits.device)
    else:
        assert _dense(lse).numel() == n * H * W
    form, blocks = dice_form(logits, label_u8, lse, generic)
    slab = torch.empty(n, blocks, c, 2, dtype=F64, device=logits.device)
    counts = torch.empty(n, blocks, c + 3, dtype=I64, device=logits.device)
    call('pfst_dice_upsample_fwd', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), H, W, int(ignore_index), int(head_ignore_index),
         float(exponent), form, 0 if own else lse.data_ptr(), lse.data_ptr() if own else 0, slab.data_ptr(), counts.data_ptr(),
         blocks, _stream())
    return slab, counts, lse, form


def dice_finalize(slab, counts, class_weight=None, ignore_index=255, smooth=1.0, exponent=2.0, loss_weight=1.0):
    """adds the partials in a fixed order -> (out float32[3] = (loss, acc_seg %, #bad labels), coef float32 [N, C, 2] = the gradient's
    (a, b) table, sums float64 [N*C*3 + 3] = (I, P, T) per (n, c), then (#correct, #valid, #bad))"""
    n, blocks, c, _ = slab.shape
    assert tuple(counts.shape) == (n, blocks, c + 3)
    if class_weight is not None:
        assert _dense(class_weight).numel() == c
    sums = torch.empty(n * c * 3 + 3, dtype=F64, device=slab.device)
    coef = torch.empty(n, c, 2, device=slab.device)
    out = torch.empty(3, device=slab.device)
    call('pfst_dice_finalize', slab.data_ptr(), counts.data_ptr(), n, c, blocks, _p(class_weight), int(ignore_index), float(smooth),
         float(exponent), float(loss_weight), sums.data_ptr(), coef.data_ptr(), out.data_ptr(), _stream())
    return out, coef, sums


def dice_upsample_bwd(logits, label_u8, lse, coef, scale, ignore_index=255, exponent=2.0, out=None, accumulate=False, generic=False):
    """d logits of the Dice term (gather form, no atomics); `scale` carries loss_weight and the step's gradient scale"""
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    if out is None:
        assert not accumulate
        out = torch.empty_like(logits)
    assert tuple(coef.shape) == (n, c, 2) and _dense(lse).numel() == n * H * W
    form, _ = dice_form(logits, label_u8, lse, generic)
    work = torch.empty(n, H, W, device=logits.device) if form == 0 and c > 8 else None
    call('pfst_dice_upsample_bwd', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), H, W, int(ignore_index), float(exponent), form,
         lse.data_ptr(), _dense(coef).data_ptr(), float(scale), _p(work), _dense(out).data_ptr(), int(accumulate), _stream())
    return out


def sigloss_form(logits, label_u8, pix_weight=None, generic=False):
    """which kernels a sigmoid loss term (FocalLoss, CrossEntropyLoss(use_sigmoid)) runs on, by dice_form's rules: 4 / 8 = the inter-cell
    block kernels of that ratio (C <= 8, H == S h, W == S w, pixel weights 8-byte and label 2-byte aligned), 0 = the generic ones;
    generic=True forces 0.  -> (form, rows of partials per image)"""
    return _blocks_form(logits, label_u8, pix_weight, generic)


def _sigloss_args(logits, label_u8, pix_weight, coef):
    _dense(logits), _dense(label_u8, U8)
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    assert label_u8.numel() == n * H * W
    if pix_weight is not None:
        assert _dense(pix_weight).numel() == n * H * W
    if tuple(_dense(coef).shape) != (c, 2):
        raise ValueError(f'sigmoid loss: the (k_pos, k_neg) table must be float [{c}, 2], got {tuple(coef.shape)}')
    return n, c, h, w, H, W


def sigloss_upsample_fwd(logits, label_u8, coef, gamma=0.0, pix_weight=None, ignore_index=255, generic=False):
    """Per-workgroup partials of sum w_px valid k q^gamma b over sigmoid(up(logits)) and the head's accuracy counts; no atomics, a fixed order.
    coef float [C, 2] = (k_pos, k_neg) per class.
    -> (slab float64 [N, blocks, C], counts int64 [N, blocks, 3] = (#correct, #valid, #bad), form)"""
    n, c, h, w, H, W = _sigloss_args(logits, label_u8, pix_weight, coef)
    if not float(gamma) >= 0.0:
        raise ValueError(f'sigmoid loss: gamma must be >= 0, got {gamma}')
    form, blocks = sigloss_form(logits, label_u8, pix_weight, generic)
    slab = torch.empty(n, blocks, c, dtype=F64, device=logits.device)
    counts = torch.empty(n, blocks, 3, dtype=I64, device=logits.device)
    call('pfst_sigloss_upsample_fwd', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), _p(pix_weight), H, W, int(ignore_index),
         coef.data_ptr(), float(gamma), form, slab.data_ptr(), counts.data_ptr(), blocks, _stream())
    return slab, counts, form


def sigloss_finalize(slab, counts, divisor, loss_weight=1.0):
    """adds the partials in a fixed order -> (out float32[3] = (loss_weight / divisor * sum, acc_seg %, #bad labels),
    sums float64 [N*C + 3] = the loss sum per (n, c), then (#correct, #valid, #bad))"""
    n, blocks, c = slab.shape
    assert tuple(counts.shape) == (n, blocks, 3)
    sums = torch.empty(n * c + 3, dtype=F64, device=slab.device)
    out = torch.empty(3, device=slab.device)
    call('pfst_sigloss_finalize', slab.data_ptr(), counts.data_ptr(), n, c, blocks, float(divisor), float(loss_weight), sums.data_ptr(),
         out.data_ptr(), _stream())
    return out, sums


def sigloss_upsample_bwd(logits, label_u8, coef, scale, gamma=0.0, pix_weight=None, ignore_index=255, out=None, accumulate=False, generic=False):
    """d logits of a sigmoid loss term (gather form, no atomics); `scale` carries loss_weight / divisor and the step's gradient scale"""
    n, c, h, w, H, W = _sigloss_args(logits, label_u8, pix_weight, coef)
    if out is None:
        assert not accumulate
        out = torch.empty_like(logits)
    form, _ = sigloss_form(logits, label_u8, pix_weight, generic)
    call('pfst_sigloss_upsample_bwd', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), _p(pix_weight), H, W, int(ignore_index),
         coef.data_ptr(), float(gamma), form, float(scale), _dense(out).data_ptr(), int(accumulate), _stream())
    return out


def lovasz_form(logits, label_u8, lse=None, generic=False):
    """which kernels a Lovasz term's key and backward passes run on, by dice_form's rules -> 4 / 8 (block frames) or 0 (generic)"""
    return _blocks_form(logits, label_u8, lse, generic)[0]


def lovasz_workspace(segments, seg_stride, dev):
    """the workspace of `segments` segments of `seg_stride` elements: ping-pong (key, value) buffers, digit histograms, per-tile partials"""
    nbytes = ctypes.c_longlong(0)
    call('pfst_lovasz_workspace_bytes', int(segments), int(seg_stride), ctypes.addressof(nbytes))
    return torch.empty((nbytes.value + 15) // 16 * 2, dtype=I64, device=dev)


def lovasz_sort(keys, seg_len=None, vals=None, out=None):
    """pfst_lovasz_sort: the stable ascending radix sort of the 32-bit patterns in keys (int32 [S, stride], read as unsigned), segment by
    segment; seg_len: int32 [S] on the device (None: full segments); vals: int32 [S, stride] carried along (None: the index in the segment,
    so that the second result is the permutation).  out: (keys_out, vals_out) to write into.  Elements at and beyond a segment's length
    are not written.  -> (keys_out, vals_out)"""
    _dense(_chk(keys, I32, 2), I32)
    s, stride = keys.shape
    if seg_len is not None and tuple(_dense(seg_len, I32).shape) != (s,):
        raise ValueError(f'lovasz_sort: seg_len {tuple(seg_len.shape)} for {s} segments')
    if vals is not None and _dense(vals, I32).shape != keys.shape:
        raise ValueError('lovasz_sort: vals must have the shape of keys')
    ko, vo = out if out is not None else (torch.empty_like(keys), torch.empty_like(keys))
    if _dense(ko, I32).numel() < keys.numel() or _dense(vo, I32).numel() < keys.numel():
        raise ValueError('lovasz_sort: output buffers are smaller than the keys')
    ws = lovasz_workspace(s, stride, keys.device)
    call('pfst_lovasz_sort', keys.data_ptr(), _p(vals), s, stride, _p(seg_len), ws.data_ptr(), ko.data_ptr(), vo.data_ptr(), _stream())
    return ko, vo


def lovasz_class_tables(classes, num_classes, dev):
    """classes: 'all' | 'present' | a list of class indices -> (slot int32 [C]: the class's slot or -1, cls int32 [K]: the class of a slot)"""
    cls = list(range(num_classes)) if classes in ('all', 'present') else [int(c) for c in classes]
    if not cls or any(not 0 <= c < num_classes for c in cls) or len(set(cls)) != len(cls):
        raise ValueError(f'LovaszLoss: classes {classes!r} must be distinct class indices in [0, {num_classes})')
    slot = [-1] * num_classes
    for k, c in enumerate(cls):
        slot[c] = k
    return torch.tensor(slot, dtype=I32, device=dev), torch.tensor(cls, dtype=I32, device=dev)


def lovasz_upsample_fwd(logits, label_u8, slot, cls, slot_weight=None, ignore_index=255, per_image=False, present=True, reduction='mean',
                        loss_weight=1.0, lse=None, generic=False, want_sorted=False, stage_hook=None):
    """The Lovasz-Softmax loss of softmax(up(logits)) (csrc/lovasz_loss.hip): key pass, segmented radix sort, gradient pass, finalize -- four
    ABI calls on the current stream, nothing read on the host.  slot / cls: lovasz_class_tables; slot_weight: float [K] (the class weights
    by slot) or None; reduction ('mean' | 'sum') counts with per_image only.  lse: a CE / Dice term's log-sum-exp (None: formed here).
    stage_hook(name): called after each stage's launches (tools/lovasz_bench.py records events there).
    -> dict(out float32[3] = (loss, acc_seg %, #bad labels), map float [N, K, H, W] (unwritten where label == ignore_index), scale float
    [N, K], lse, sums float64 [segments], counters int64 [3 + N K], form[, keys, vals: int32 [segments, L], the sorted order])"""
    _dense(logits), _dense(label_u8, U8)
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    k = cls.numel()
    if label_u8.numel() != n * H * W or tuple(_dense(slot, I32).shape) != (c,) or not 1 <= _dense(cls, I32).numel() <= c:
        raise ValueError(f'lovasz_upsample_fwd: logits {tuple(logits.shape)}, labels {tuple(label_u8.shape)}, {k} slots')
    if slot_weight is not None and tuple(_dense(slot_weight).shape) != (k,):
        raise ValueError(f'lovasz_upsample_fwd: slot_weight {tuple(slot_weight.shape)} for {k} slots')
    if reduction not in ('mean', 'sum'):
        raise ValueError(f'lovasz_upsample_fwd: reduction {reduction!r}')
    dev = logits.device
    own = lse is None
    if own:
        lse = torch.empty(n, H, W, device=dev)
    else:
        assert _dense(lse).numel() == n * H * W
    form = lovasz_form(logits, label_u8, lse, generic)
    pi = int(bool(per_image))
    segs, seg_len = (n * k, H * W) if pi else (k, n * H * W)
    ws = lovasz_workspace(segs, seg_len, dev)
    counters = torch.empty(3 + n * k, dtype=I64, device=dev)
    cmap = torch.empty(n, k, H, W, device=dev)
    sums = torch.empty(segs, dtype=F64, device=dev)
    scale = torch.empty(n, k, device=dev)
    out = torch.empty(3, device=dev)
    hook = stage_hook if stage_hook is not None else (lambda name: None)
    call('pfst_lovasz_keys', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), H, W, int(ignore_index), form, slot.data_ptr(), k, pi,
         0 if own else lse.data_ptr(), lse.data_ptr() if own else 0, ws.data_ptr(), counters.data_ptr(), _stream())
    hook('keys')
    call('pfst_lovasz_sort_keys', n, H, W, k, pi, ws.data_ptr(), _stream())
    hook('sort')
    call('pfst_lovasz_grad', n, H, W, k, pi, counters.data_ptr(), _p(slot_weight), ws.data_ptr(), cmap.data_ptr(), _stream())
    hook('grad')
    call('pfst_lovasz_finalize', n, H, W, k, pi, int(bool(present)), int(reduction == 'sum'), counters.data_ptr(), _p(slot_weight),
         float(loss_weight), ws.data_ptr(), sums.data_ptr(), scale.data_ptr(), out.data_ptr(), _stream())
    hook('finalize')
    res = dict(out=out, map=cmap, scale=scale, lse=lse, sums=sums, counters=counters, form=form)
    if want_sorted:
        nel = segs * seg_len
        pad = (nel * 4 + 15) // 16 * 16 // 4                # the workspace's buffers are 16-byte aligned: keys A, then values A
        flat = ws.view(I32)
        res['keys'] = flat[:nel].view(segs, seg_len).clone()
        res['vals'] = flat[pad:pad + nel].view(segs, seg_len).clone()
    return res


def lovasz_upsample_bwd(logits, label_u8, slot, cls, lse, cmap, scale, grad_scale, ignore_index=255, out=None, accumulate=False, generic=False):
    """d logits of the Lovasz term (gather form, no atomics); `grad_scale` carries loss_weight and the step's gradient scale"""
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    k = cls.numel()
    if out is None:
        assert not accumulate
        out = torch.empty_like(logits)
    assert tuple(_dense(cmap).shape) == (n, k, H, W) and tuple(_dense(scale).shape) == (n, k) and _dense(lse).numel() == n * H * W
    assert tuple(_dense(slot, I32).shape) == (c,) and out.shape == logits.shape
    form = lovasz_form(logits, label_u8, lse, generic)
    work = torch.empty(n, H, W, device=logits.device) if form == 0 and c > 8 else None
    call('pfst_lovasz_upsample_bwd', _dense(logits).data_ptr(), n, c, h, w, _dense(label_u8, U8).data_ptr(), H, W, int(ignore_index), form,
         slot.data_ptr(), _dense(cls, I32).data_ptr(), k, lse.data_ptr(), cmap.data_ptr(), scale.data_ptr(), float(grad_scale), _p(work),
         _dense(out).data_ptr(), int(accumulate), _stream())
    return out


ENTROPY_KINDS = {'entropy': 0, 'max_square': 1}


def _entropy_args(logits, kind):
    """logits [N, C, h, w]: dense, at any offset of its storage (data_ptr carries it); a strided view is refused, as by the other loss wrappers"""
    _chk(logits, F32, 4)
    if not logits.is_contiguous():
        raise ValueError(f'softmax_entropy: logits must be dense NCHW (shape {tuple(logits.shape)}, strides {logits.stride()}); '
                         'pass .contiguous()')
    if kind not in ENTROPY_KINDS:
        raise ValueError(f'softmax_entropy: kind must be one of {tuple(ENTROPY_KINDS)}, got {kind!r}')
    n, c, h, w = logits.shape
    return n, c, h * w, ENTROPY_KINDS[kind]


def softmax_entropy(logits, kind, weight, generic=False):
    """EntropyLoss of low-resolution logits [N, C, h, w] (pfst_softmax_entropy_fwd): kind 'entropy' = weight * mean_px of the normalised
    entropy of softmax_c, 'max_square' = -weight * mean(p^2) / 2.  Per-workgroup fp64 partials + one ordered sum, no atomics: bit-identical
    run to run in every mode.  generic=True forces the class-loop kernels at C <= 8 (tests).  -> float32 [1] on the device"""
    n, c, hw, k = _entropy_args(logits, kind)
    nbytes = ctypes.c_longlong(0)
    call('pfst_softmax_entropy_workspace_bytes', n, hw, ctypes.addressof(nbytes))
    work = torch.empty(nbytes.value // 8, dtype=F64, device=logits.device)
    out = torch.empty(1, device=logits.device)
    call('pfst_softmax_entropy_fwd', logits.data_ptr(), n, c, hw, k, int(bool(generic)), float(weight), work.data_ptr(), out.data_ptr(),
         _stream())
    return out


def softmax_entropy_bwd_(dlogits, logits, kind, weight, grad_scale=1.0, accumulate=True, generic=False):
    """dlogits (+)= grad_scale * d softmax_entropy(logits, kind, weight) / d logits, the probabilities formed again from the logits.
    accumulate=False writes every element of dlogits.  Both tensors dense (an offset view is fine), same shape, not overlapping"""
    n, c, hw, k = _entropy_args(logits, kind)
    _chk(dlogits, F32, 4)
    if not dlogits.is_contiguous() or dlogits.shape != logits.shape:
        raise ValueError(f'softmax_entropy_bwd_: dlogits must be dense with the logits\' shape {tuple(logits.shape)}, got shape '
                         f'{tuple(dlogits.shape)} strides {dlogits.stride()}')
    call('pfst_softmax_entropy_bwd', logits.data_ptr(), n, c, hw, k, int(bool(generic)), float(weight), float(grad_scale), dlogits.data_ptr(),
         int(bool(accumulate)), _stream())
    return dlogits


# ---------------------------------------------------------------- adversarial baseline (ADVENT): entropy map, 4x4 / stride-2 convolutions, L1 tail
def _same_dense(name, t, like):
    _chk(t, F32, 4)
    if not t.is_contiguous() or t.shape != like.shape:
        raise ValueError(f'{name} must be dense with shape {tuple(like.shape)}, got shape {tuple(t.shape)} strides {t.stride()}')
    return t


def entropy_map(logits, generic=False, out=None):
    """pfst_entropy_map: logits [N, C, h, w] -> ent [N, C, h, w], ent_c = -p_c log2(p_c + 1e-30) / log2(C) with p = softmax_c(logits): the
    discriminator's input (adv_loss.py:47-50), not summed over the classes"""
    n, c, hw, _ = _entropy_args(logits, 'entropy')
    out = torch.empty_like(logits) if out is None else _same_dense('entropy_map: out', out, logits)
    call('pfst_entropy_map', logits.data_ptr(), n, c, hw, int(bool(generic)), out.data_ptr(), _stream())
    return out


def entropy_map_bwd_(dlogits, logits, grad_ent, accumulate=True, generic=False):
    """dlogits (+)= the gradient of entropy_map(logits) contracted with grad_ent, through the entropy term and the softmax; the probabilities
    are formed again from the logits.  accumulate=False writes every element"""
    n, c, hw, _ = _entropy_args(logits, 'entropy')
    _same_dense('entropy_map_bwd_: grad_ent', grad_ent, logits)
    _same_dense('entropy_map_bwd_: dlogits', dlogits, logits)
    call('pfst_entropy_map_bwd', logits.data_ptr(), grad_ent.data_ptr(), n, c, hw, int(bool(generic)), dlogits.data_ptr(), int(bool(accumulate)),
         _stream())
    return dlogits


def _adv_conv_shapes(name, x, w):
    _dense(x)
    _dense(w)
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (x.shape[1], 4, 4) or x.shape[2] < 2 or x.shape[3] < 2:
        raise ValueError(f'{name}: x [N, Cin, H >= 2, W >= 2] and w [Cout, Cin, 4, 4], got {tuple(x.shape)} and {tuple(w.shape)}')
    n, cin, h, wd = x.shape
    return n, cin, h, wd, w.shape[0]


def adv_conv(x, w, bias=None, slope=None, out=None):
    """pfst_adv_conv_fwd: Conv2d(kernel 4, stride 2, padding 1) of x [N, Cin, H, W] with w [Cout, Cin, 4, 4] (+ bias), then LeakyReLU(slope)
    in the epilogue unless slope is None -> y [N, Cout, H // 2, W // 2]"""
    n, cin, h, wd, cout = _adv_conv_shapes('adv_conv', x, w)
    if bias is not None and (_dense(bias).dim() != 1 or bias.numel() != cout):
        raise ValueError(f'adv_conv: bias {tuple(bias.shape)} for {cout} output channels')
    shape = (n, cout, h // 2, wd // 2)
    if out is None:
        out = torch.empty(shape, device=x.device)
    elif tuple(_dense(out).shape) != shape:
        raise ValueError(f'adv_conv: out {tuple(out.shape)}, expected {shape}')
    call('pfst_adv_conv_fwd', x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), n, cin, h, wd, cout, int(slope is not None),
         float(slope or 0.0), _stream())
    return out


def adv_conv_dgrad_(dx, dy, w, x_gate=None, slope=0.0, accumulate=False):
    """pfst_adv_conv_dgrad: dx [N, Cin, H, W] (+)= the data gradient of adv_conv for dy [N, Cout, H // 2, W // 2]; x_gate (the layer's input x
    where x is a LeakyReLU output): multiplied by x > 0 ? 1 : slope, i.e. dx is the gradient of the pre-activation below"""
    n, cin, h, wd, cout = _adv_conv_shapes('adv_conv_dgrad_', dx, w)
    if tuple(_dense(dy).shape) != (n, cout, h // 2, wd // 2):
        raise ValueError(f'adv_conv_dgrad_: dy {tuple(dy.shape)}, expected {(n, cout, h // 2, wd // 2)}')
    if x_gate is not None:
        _same_dense('adv_conv_dgrad_: x_gate', x_gate, dx)
    call('pfst_adv_conv_dgrad', dy.data_ptr(), w.data_ptr(), _p(x_gate), dx.data_ptr(), n, cin, h, wd, cout, float(slope), int(bool(accumulate)),
         _stream())
    return dx


ADV_WGRAD_LAUNCHES = 0          # counts adv_conv_wgrad_ calls (the frozen-discriminator pass of the adversarial step must launch none)


def adv_conv_wgrad_(dw, db, x, dy):
    """pfst_adv_conv_wgrad: dw [Cout, Cin, 4, 4] += and db [Cout] += (db may be None) the weight / bias gradients of adv_conv(x, w) for dy"""
    global ADV_WGRAD_LAUNCHES
    n, cin, h, wd, cout = _adv_conv_shapes('adv_conv_wgrad_', x, dw)
    if tuple(_dense(dy).shape) != (n, cout, h // 2, wd // 2):
        raise ValueError(f'adv_conv_wgrad_: dy {tuple(dy.shape)}, expected {(n, cout, h // 2, wd // 2)}')
    if db is not None and (_dense(db).dim() != 1 or db.numel() != cout):
        raise ValueError(f'adv_conv_wgrad_: db {tuple(db.shape)} for {cout} output channels')
    ADV_WGRAD_LAUNCHES += 1
    call('pfst_adv_conv_wgrad', x.data_ptr(), dy.data_ptr(), dw.data_ptr(), _p(db), n, cin, h, wd, cout, _stream())
    return dw


def adv_tail(y, label, weight, grad_scale=1.0, want_grad=True):
    """pfst_adv_tail: y [N, 1, h, w], the discriminator's last plane -> (d [N] = the plane means, loss [1] = weight * mean_n |d_n - label|,
    gy like y = grad_scale * dloss/dy, or None)"""
    _dense(y)
    if y.dim() != 4 or y.shape[1] != 1:
        raise ValueError(f'adv_tail: y must be [N, 1, h, w], got {tuple(y.shape)}')
    n, hw = y.shape[0], y.shape[2] * y.shape[3]
    d = torch.empty(n, device=y.device)
    loss = torch.empty(1, device=y.device)
    gy = torch.empty_like(y) if want_grad else None
    call('pfst_adv_tail', y.data_ptr(), n, hw, float(label), float(weight), float(grad_scale), d.data_ptr(), loss.data_ptr(), _p(gy), _stream())
    return d, loss, gy


def pseudo_label(logits, size, threshold, want_i64=True, want_conf=False, want_prob=False):
    """-> (label int64 [N,H,W] | None, label uint8 [N,H,W], count uint64-as-int64 [1][, conf float [N,H,W]][, max prob float [N,H,W]])"""
    _dense(logits)
    n, c, h, w = logits.shape
    H, W = size
    l64 = torch.empty(n, H, W, dtype=I64, device=logits.device) if want_i64 else None
    l8 = torch.empty(n, H, W, dtype=U8, device=logits.device)
    cnt = torch.empty(1, dtype=I64, device=logits.device)
    conf = torch.empty(n, H, W, device=logits.device) if want_conf else None
    prob = torch.empty(n, H, W, device=logits.device) if want_prob else None
    call('pfst_pseudo_label', logits.data_ptr(), n, c, h, w, H, W, float(threshold), _p(l64), l8.data_ptr(), cnt.data_ptr(), _p(conf),
         _p(prob), _stream())
    res = (l64, l8, cnt)
    if want_conf:
        res += (conf,)
    if want_prob:
        res += (prob,)
    return res


def _entropy_shape(name, logits, size):
    _dense(_chk(logits, F32, 4))
    n, c, h, w = logits.shape
    H, W = (int(v) for v in size)
    if not (n >= 1 and 1 <= c <= 255 and h >= 1 and w >= 1 and H >= 1 and W >= 1):
        raise ValueError(f'{name}: logits {tuple(logits.shape)} (1 .. 255 classes) to size {(H, W)}')
    return n, c, h, w, H, W


def entropy_upsample(logits, size, mode=0, want_entropy=True, want_pred=True):
    """pfst_entropy_upsample: logits [N, C, h, w] resized to `size` in registers -> (entropy float [N, H, W] | None, pred uint8 [N, H, W] |
    None).  mode 0: the threshold pass (softmax arg-max, -sum p log p), mode 1: the label pass (logit arg-max, -sum p log(p + 1e-8))."""
    n, c, h, w, H, W = _entropy_shape('entropy_upsample', logits, size)
    if mode not in (0, 1) or not (want_entropy or want_pred):
        raise ValueError(f'entropy_upsample: mode {mode} (0 | 1), and at least one output')
    ent = torch.empty(n, H, W, device=logits.device) if want_entropy else None
    pred = torch.empty(n, H, W, dtype=U8, device=logits.device) if want_pred else None
    call('pfst_entropy_upsample', logits.data_ptr(), n, c, h, w, H, W, int(mode), _p(ent), _p(pred), _stream())
    return ent, pred


def entropy_class_hist(logits, size, shift, bits, hist, prefix=None):
    """pfst_entropy_class_hist: ADDS one radix level of the per-class entropy keys of logits [N, C, h, w] at `size` to hist (int64 [C, 1 << bits]
    on the device, unsigned counters): digit (key >> shift) & (2^bits - 1) of the pixels whose higher bits equal prefix[pred] (int32 [C], the
    unsigned prefixes; None: every pixel).  -> hist"""
    n, c, h, w, H, W = _entropy_shape('entropy_class_hist', logits, size)
    shift, bits = int(shift), int(bits)
    if not (shift >= 0 and 1 <= bits <= 16 and shift + bits <= 32) or (prefix is not None and shift + bits >= 32):
        raise ValueError(f'entropy_class_hist: shift {shift}, bits {bits} (1 .. 16, shift + bits <= 32, < 32 with a prefix)')
    if tuple(_dense(hist, I64).shape) != (c, 1 << bits):
        raise ValueError(f'entropy_class_hist: hist {tuple(hist.shape)} for {c} classes and {bits} bits')
    if prefix is not None and tuple(_dense(prefix, torch.int32).shape) != (c,):
        raise ValueError(f'entropy_class_hist: prefix {tuple(prefix.shape)} for {c} classes')
    call('pfst_entropy_class_hist', logits.data_ptr(), n, c, h, w, H, W, shift, bits, _p(prefix), hist.data_ptr(), _stream())
    return hist


def entropy_pseudo_label(logits, size, thr, annotation_space=False, counts=None):
    """pfst_entropy_pseudo_label: -> (label uint8 [N, H, W], counts int64 [C, 2]); thr float [C] on the device.  The label is the logit
    arg-max where the loader's entropy lies below thr[arg-max], else 255 (annotation_space: arg-max + 1, else 0); `counts` (a new zeroed
    table unless given) += per class (pixels predicted, pixels kept)."""
    n, c, h, w, H, W = _entropy_shape('entropy_pseudo_label', logits, size)
    if tuple(_dense(thr).shape) != (c,):
        raise ValueError(f'entropy_pseudo_label: thr {tuple(thr.shape)} for {c} classes')
    if counts is None:
        counts = torch.zeros(c, 2, dtype=I64, device=logits.device)
    elif tuple(_dense(counts, I64).shape) != (c, 2):
        raise ValueError(f'entropy_pseudo_label: counts {tuple(counts.shape)} for {c} classes')
    label = torch.empty(n, H, W, dtype=U8, device=logits.device)
    call('pfst_entropy_pseudo_label', logits.data_ptr(), n, c, h, w, H, W, thr.data_ptr(), int(bool(annotation_space)), label.data_ptr(),
         counts.data_ptr(), _stream())
    return label, counts


_ohem_ws_bytes = None


def ohem_sample(logits, label_u8, ignore_index=255, thresh=None, batch_kept=100000, coef=None, want_keys=False):
    """pfst_ohem_sample: OHEMPixelSampler's 0 / 1 weight map [N, H, W] of logits [N, C, h, w] under label_u8 [N, 1, H, W] or [N, H, W], every
    launch on the current stream and nothing read on the host.  thresh (a float): weight 1 where the label's softmax probability lies below
    max(s[k], fp32(thresh)), s the ascending sort over the valid pixels and k = min(batch_kept, n_valid - 1).  thresh None: the
    min(batch_kept, n_valid) valid pixels of largest coef[label] * nll (coef float [C] on the device, >= 0), ties at the cut kept in raster order.
    -> (weight, info int64 [4] = (bit pattern of the fp32 threshold / cut value, n_valid, n_kept, k)[, keys float [N, H, W]: the map the
    select ran on, -1 where the pixel is not valid])"""
    global _ohem_ws_bytes
    _dense(_chk(logits, F32, 4)), _dense(label_u8, U8)
    n, c, h, w = logits.shape
    H, W = label_u8.shape[-2:]
    if label_u8.numel() != n * H * W or not 1 <= c <= 255:
        raise ValueError(f'ohem_sample: logits {tuple(logits.shape)} (1 .. 255 classes) with labels {tuple(label_u8.shape)}')
    batch_kept = int(batch_kept)
    if batch_kept < 0:
        raise ValueError(f'ohem_sample: batch_kept {batch_kept}')
    if thresh is None:
        if coef is None or tuple(_dense(coef).shape) != (c,):
            raise ValueError(f'ohem_sample: without a threshold the per-class loss coefficients are needed, float [{c}]')
    elif thresh != thresh:
        raise ValueError('ohem_sample: thresh is NaN')
    dev = logits.device
    if _ohem_ws_bytes is None:
        nbytes = ctypes.c_longlong(0)
        call('pfst_ohem_workspace_bytes', n, H, W, ctypes.addressof(nbytes))
        _ohem_ws_bytes = nbytes.value
    ws = torch.empty(_ohem_ws_bytes // 8, dtype=I64, device=dev)
    weight = torch.empty(n, H, W, device=dev)
    info = torch.empty(4, dtype=I64, device=dev)
    keys = torch.empty(n, H, W, device=dev) if want_keys else None
    call('pfst_ohem_sample', logits.data_ptr(), n, c, h, w, label_u8.data_ptr(), H, W, int(ignore_index), int(thresh is not None),
         0.0 if thresh is None else float(thresh), batch_kept, _p(None if thresh is not None else coef), ws.data_ptr(), weight.data_ptr(),
         info.data_ptr(), _p(keys), _stream())
    return (weight, info, keys) if want_keys else (weight, info)


def label_presence(label_u8):
    _dense(label_u8, U8)
    pres = torch.empty(256, dtype=torch.int32, device=label_u8.device)
    call('pfst_label_presence', label_u8.data_ptr(), label_u8.numel(), pres.data_ptr(), _stream())
    return pres


def class_mask(gt_u8, classes):
    """classes: int32 [N, K] device tensor (entries < 0 = padding) -> mask uint8 [N,1,H,W]"""
    _dense(gt_u8, U8), _dense(classes, torch.int32)
    n = gt_u8.shape[0]
    hw = gt_u8.numel() // n
    mask = torch.empty_like(gt_u8)
    call('pfst_class_mask', gt_u8.data_ptr(), classes.data_ptr(), classes.shape[1], mask.data_ptr(), n, hw, _stream())
    return mask


def class_mix(img, trg_img, gt_u8, pseudo_u8, mask_u8, conf_count, want_i64=False, trg_weight=None):
    _dense(img), _dense(trg_img), _dense(gt_u8, U8), _dense(pseudo_u8, U8), _dense(mask_u8, U8), _dense(conf_count, I64)
    n, c, h, w = img.shape
    assert trg_img.shape == img.shape and gt_u8.numel() == n * h * w == pseudo_u8.numel() == mask_u8.numel()
    mimg = torch.empty_like(img)
    mlbl = torch.empty(n, 1, h, w, dtype=U8, device=img.device)
    mlbl64 = torch.empty(n, 1, h, w, dtype=I64, device=img.device) if want_i64 else None
    mw = torch.empty(n, h, w, device=img.device)
    call('pfst_class_mix', img.data_ptr(), trg_img.data_ptr(), gt_u8.data_ptr(), pseudo_u8.data_ptr(), mask_u8.data_ptr(),
         conf_count.data_ptr(), _p(trg_weight), mimg.data_ptr(), mlbl.data_ptr(), _p(mlbl64), mw.data_ptr(), n, c, h * w, _stream())
    return mimg, mlbl, mlbl64, mw


# ---------------------------------------------------------------- PFGSTLoss pieces
SIM_TYPES = {'cosine': 0, 'gaussian': 1}
SRC_LOSS_TYPES = {'mean_std': 0, 'margin': 1, 'margin2': 2}


def sim_map(feat, dil, sim_type='cosine', sigma=30.0, ksize=3):
    """-> (sim [N, ksize^2, H, W], norm [N, H, W]).  ksize 3: the 3x3 entry (strip kernels, production path); 5 / 7: pfst_sim_map_k.
    The similarity map and its adjoint are the only PFGSTLoss pieces with two implementations; the rest take `ksize` as an argument"""
    _dense(feat)
    n, c, h, w = feat.shape
    sim = torch.empty(n, ksize * ksize, h, w, device=feat.device)
    norm = torch.empty(n, h, w, device=feat.device)
    if ksize == 3:
        call('pfst_sim_map', feat.data_ptr(), n, c, h, w, dil, SIM_TYPES[sim_type], float(sigma), sim.data_ptr(), norm.data_ptr(), _stream())
    else:
        call('pfst_sim_map_k', feat.data_ptr(), n, c, h, w, ksize, dil, SIM_TYPES[sim_type], float(sigma), sim.data_ptr(), norm.data_ptr(),
             _stream())
    return sim, norm


def sim_map_bwd(feat, sim, norm, gsim, dil, out=None, accumulate=False, sim_type='cosine', sigma=30.0, ksize=3):
    n, c, h, w = feat.shape
    if out is None:
        assert not accumulate
        out = torch.empty_like(feat)
    if ksize == 3:
        coef = torch.empty(n * 10 * h * w, dtype=F32, device=feat.device) if sim_type == 'cosine' else None
        call('pfst_sim_map_bwd', _dense(feat).data_ptr(), _dense(sim).data_ptr(), _dense(norm).data_ptr(), _dense(gsim).data_ptr(),
             n, c, h, w, dil, SIM_TYPES[sim_type], float(sigma), _dense(out).data_ptr(), int(accumulate), _p(coef), _stream())
    else:
        coef = torch.empty(n * (ksize * ksize + 1) * h * w, dtype=F32, device=feat.device)
        call('pfst_sim_map_bwd_k', _dense(feat).data_ptr(), _dense(sim).data_ptr(), _dense(norm).data_ptr(), _dense(gsim).data_ptr(),
             n, c, h, w, ksize, dil, SIM_TYPES[sim_type], float(sigma), _dense(out).data_ptr(), int(accumulate), coef.data_ptr(), _stream())
    return out


def src_sim_losses(sim, gt_u8, dil, w_pos, w_neg, w_pos_std=0.0, w_neg_std=0.0, loss_type='mean_std', margin=(0.5, 0.5), src_perc=None,
                   ksize=3):
    """-> (losses float32[4] (mean_std) or [2] used of 4 (margin / margin2), gsim [N,ksize^2,H,W]).
    src_perc: only the int(n * src_perc) smallest positive / largest negative similarities count (pfgst_loss.py:98-102)"""
    n, _, h, w = sim.shape
    hg, wg = gt_u8.shape[-2:]
    lt = SRC_LOSS_TYPES[loss_type]
    sel = None
    if src_perc is not None:
        sel = torch.empty(lib().pfst_src_sim_select_bytes() // 8 + 1, dtype=I64, device=sim.device)       # 8-byte aligned scratch
        call('pfst_src_sim_select', _dense(sim).data_ptr(), _dense(gt_u8, U8).data_ptr(), n, h, w, hg, wg, ksize, dil, float(src_perc),
             sel.data_ptr(), _stream())
    stats = torch.empty(6, dtype=F64, device=sim.device)
    call('pfst_src_sim_stats', _dense(sim).data_ptr(), _dense(gt_u8, U8).data_ptr(), n, h, w, hg, wg, ksize, dil, lt, float(margin[0]),
         float(margin[1]), stats.data_ptr(), _p(sel), _stream())
    gsim = torch.empty_like(sim)
    losses = torch.empty(4, device=sim.device)
    call('pfst_src_sim_grad', sim.data_ptr(), gt_u8.data_ptr(), n, h, w, hg, wg, ksize, dil, lt, float(margin[0]), float(margin[1]),
         stats.data_ptr(), float(w_pos), float(w_neg), float(w_pos_std), float(w_neg_std), gsim.data_ptr(), losses.data_ptr(), _p(sel),
         _stream())
    return losses, gsim


def softmax_down(logits, ds):
    _dense(logits)
    n, c, h, w = logits.shape
    H, W = int(h // ds), int(w // ds)
    prob = torch.empty(n, c, H, W, device=logits.device)
    call('pfst_softmax_down', logits.data_ptr(), n, c, h, w, ds, prob.data_ptr(), H, W, _stream())
    return prob


def trg_valid_mask(gt_u8, mix_mask_u8, hw, dil, ksize=3):
    n = gt_u8.shape[0]
    hg, wg = gt_u8.shape[-2:]
    valid = torch.empty(n, 1, hw[0], hw[1], dtype=U8, device=gt_u8.device)
    all9 = torch.empty(n, 1, hw[0], hw[1], dtype=U8, device=gt_u8.device)
    cnt = torch.empty(1, dtype=I64, device=gt_u8.device)
    call('pfst_trg_valid_mask', _dense(gt_u8, U8).data_ptr(), _dense(mix_mask_u8, U8).data_ptr(), n, hw[0], hw[1], hg, wg, ksize, dil,
         valid.data_ptr(), all9.data_ptr(), cnt.data_ptr(), _stream())
    return valid, all9, cnt


def sim_topk_loss(ema_sim, prob, valid, count, dil, top_k, w_pos, w_neg, want_sim_grad=False, ksize=3):
    """top_k None / 0 = all ksize^2 pairs, else 1 .. ksize^2 - 1 (the top / bottom sets overlap above (ksize^2 - 1) / 2).
    -> (losses float32[2], gP [N,ksize^2,H,W][, d losses / d ema_sim [N,ksize^2,H,W]])"""
    top_k = int(top_k or 0)
    n, c, h, w = prob.shape
    kk = ksize * ksize
    gP = torch.empty(n, kk, h, w, device=prob.device)
    gS = torch.empty(n, kk, h, w, device=prob.device) if want_sim_grad else None
    acc = torch.empty(2, dtype=F64, device=prob.device)
    out = torch.empty(2, device=prob.device)
    call('pfst_sim_topk_loss', _dense(ema_sim).data_ptr(), _dense(prob).data_ptr(), _dense(valid, U8).data_ptr(), count.data_ptr(),
         n, c, h, w, ksize, dil, top_k, float(w_pos), float(w_neg), gP.data_ptr(), acc.data_ptr(), _p(gS), _stream())
    call('pfst_sim_loss_finalize', acc.data_ptr(), count.data_ptr(), ksize, top_k, float(w_pos), float(w_neg), out.data_ptr(), _stream())
    return (out, gP, gS) if want_sim_grad else (out, gP)


def cross_prob_bwd_(dlogits, prob, gP, dil, ds, unfold_grad=False, ksize=3):
    n, c, H, W = prob.shape
    h, w = dlogits.shape[-2:]
    call('pfst_cross_prob_bwd', _dense(prob).data_ptr(), _dense(gP).data_ptr(), n, c, H, W, ksize, dil, ds, int(unfold_grad),
         _dense(dlogits).data_ptr(), h, w, _stream())
    return dlogits


def sim_pair_stats_counters(ksize, bins):
    """length of the counter tensor of sim_pair_stats: hist[4][bins + 2], rank[ksize^2 - 1][2], n_centres, n_correct_centres"""
    n = lib().pfst_sim_pair_stats_counters(int(ksize), int(bins))
    if n < 0:
        raise ValueError(f'sim_pair_stats: kernel size {ksize} (3 | 5 | 7) / bins {bins} (1 .. 256)')
    return n


def sim_pair_stats(sim, pred_u8, gt_u8, dil, ksize, edges, counters):
    """pfst_sim_pair_stats: ADDS the pair statistics of sim [N, ksize^2, H, W] against pred_u8 [N, Hp, Wp] and gt_u8 [N, Hg, Wg] (255 =
    ignore; both nearest-sampled to H x W) to `counters` (int64, sim_pair_stats_counters(ksize, len(edges) - 1) entries, layout in
    include/pfst_hip.h); edges: float32 [bins + 1] on the device.  -> counters"""
    _dense(sim), _dense(pred_u8, U8), _dense(gt_u8, U8), _dense(edges), _dense(counters, I64)
    n, kk, h, w = sim.shape
    bins = edges.numel() - 1
    if kk != ksize * ksize or pred_u8.dim() != 3 or gt_u8.dim() != 3 or pred_u8.shape[0] != n or gt_u8.shape[0] != n:
        raise ValueError(f'sim_pair_stats: sim {tuple(sim.shape)}, pred {tuple(pred_u8.shape)}, gt {tuple(gt_u8.shape)} for kernel size {ksize}')
    if edges.dim() != 1 or counters.dim() != 1 or counters.numel() != sim_pair_stats_counters(ksize, bins):
        raise ValueError(f'sim_pair_stats: {counters.numel()} counters for kernel size {ksize} and {bins} bins')
    call('pfst_sim_pair_stats', sim.data_ptr(), pred_u8.data_ptr(), gt_u8.data_ptr(), n, h, w, pred_u8.shape[1], pred_u8.shape[2],
         gt_u8.shape[1], gt_u8.shape[2], ksize, int(dil), edges.data_ptr(), bins, counters.data_ptr(), _stream())
    return counters


# ---------------------------------------------------------------- flat-arena optimiser steps
def ema_update_(teacher_flat, student_flat, alpha):
    assert teacher_flat.numel() == student_flat.numel()
    call('pfst_ema_update', _dense(teacher_flat).data_ptr(), _dense(student_flat).data_ptr(), teacher_flat.numel(), float(alpha), _stream())


def adamw_step_(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=1.0):
    n = p.numel()
    assert g.numel() == n and m.numel() == n and v.numel() == n
    call('pfst_adamw_step', _dense(p).data_ptr(), _dense(g).data_ptr(), _dense(m).data_ptr(), _dense(v).data_ptr(), n, float(lr),
         float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale), _stream())


def sgd_step_(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first_step=False, grad_scale=1.0):
    """pfst_sgd_step: torch.optim.SGD's single-tensor update of the flat fp32 tensor `p` in place; `buf` (the momentum buffer, same size) is
    None exactly when momentum == 0; first_step: the buffer is written (= the decayed gradient) without being read"""
    n = p.numel()
    assert g.numel() == n and (buf is None) == (momentum == 0) and (buf is None or buf.numel() == n)
    call('pfst_sgd_step', _dense(p).data_ptr(), _dense(g).data_ptr(), None if buf is None else _dense(buf).data_ptr(), n, float(lr),
         float(momentum), float(dampening), float(weight_decay), int(bool(nesterov)), int(bool(first_step)), float(grad_scale), _stream())


# ---------------------------------------------------------------- strong augmentation
def color_jitter_(img, params, mean3, std3, denorm=True):
    _dense(img)
    n, c, h, w = img.shape
    assert c == 3 and tuple(params.shape) == (n, 8)
    call('pfst_color_jitter', img.data_ptr(), _dense(params).data_ptr(), _dense(mean3).data_ptr(), _dense(std3).data_ptr(),
         n, h * w, int(denorm), _stream())
    return img


def gaussian_blur(img, taps_y, taps_x, reach):
    _dense(img)
    n, c, h, w = img.shape
    assert taps_y.shape[0] == n and taps_x.shape[0] == n
    tmp, out = torch.empty_like(img), torch.empty_like(img)
    call('pfst_gaussian_blur', img.data_ptr(), tmp.data_ptr(), out.data_ptr(), _dense(taps_y).data_ptr(), taps_y.shape[1],
         _dense(taps_x).data_ptr(), taps_x.shape[1], n, c, h, w, int(reach), _stream())
    return out


# ---------------------------------------------------------------- evaluation
def confusion_hist_(hist, pred_u8, label_u8, num_classes, ignore_index=255):
    """hist: int64 [3*C] device tensor, accumulated in place."""
    _dense(pred_u8, U8), _dense(label_u8, U8), _dense(hist, I64)
    assert pred_u8.numel() == label_u8.numel() and hist.numel() == 3 * num_classes
    call('pfst_confusion_hist', pred_u8.data_ptr(), label_u8.data_ptr(), pred_u8.numel(), num_classes, ignore_index,
         hist.data_ptr(), _stream())
    return hist
