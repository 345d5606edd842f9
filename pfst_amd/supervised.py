"""The supervised train step of a bare segmentor: `EncoderDecoder.train_step(data_batch, optimizer)` (models.py delegates here).

Reference: segmentors/encoder_decoder.py:127-164 (train_step), base.py:177-222 (_parse_losses) and what mmcv's OptimizerHook does after
them with `optimizer_config = dict()` (no grad_clip): zero_grad, backward, step.

The device side is the scaffolding of uda.PFGST.forward_train with ONE student pass and no teacher: a flat ParamArena, one zero fill, one
Tape, the packed log vector on its way to pinned memory in front of the backward sweep, the optimizer step queued before the step's single
blocking read, the bucketed gradient reducer fired from the pass's marker closures.  It is restated here rather than shared: the PFGST
step interleaves its teacher fork, class mix and second pass with these pieces, and its launch sequence is pinned line by line
(tools/launch_trace.py)."""
from collections import OrderedDict

import torch

from . import dist as pdist
from . import hip_ops as ops
from . import layers
from .engine import ParamArena, Tape

BATCH_KEYS = ('img', 'img_metas', 'gt_semantic_seg')


class _StepState:
    """what the step keeps between calls: the arena, the cached gradient-view addresses, the pinned log buffer, the log stream"""
    __slots__ = ('arena', 'grad_ptrs', 'log_host', 'log_stream', 'steps')

    def __init__(self):
        self.arena = self.grad_ptrs = self.log_host = self.log_stream = None
        self.steps = 0


def step_state(model):
    st = model.__dict__.get('_sup_state')
    if st is None:
        st = model.__dict__['_sup_state'] = _StepState()
    return st


def ensure_arena(model, device):
    """the model's parameter arena on `device`, built on the first step, and -- on every step, before its first launch -- in step with the
    model (ParamArena.sync): a parameter whose `.data` was rebound since the last step (an evaluation hook that swapped other values in) is
    re-adopted, i.e. its current values are copied into its slot and `.data` is rebound to the slot, the optimizer's flat state kept; a
    Parameter OBJECT that was replaced (load_state_dict(assign=True), setattr) raises a RuntimeError naming it, since the optimizer holds
    the old one"""
    st = step_state(model)
    if st.arena is None or st.arena.data.device != device:
        model.to(device)
        st.arena = ParamArena(list(model.named_parameters()), device, with_grad=True)
        st.grad_ptrs = None
    st.arena.sync(model)
    return st.arena


def train_step(model, data_batch, optimizer):
    extra = sorted(set(data_batch) - set(BATCH_KEYS))
    missing = [k for k in BATCH_KEYS if k not in data_batch]
    if extra or missing:
        raise KeyError(f'EncoderDecoder.train_step takes a batch of {BATCH_KEYS}; unexpected keys {extra}, missing keys {missing} '
                       '(a source/target batch belongs to a `uda` wrapper such as PFGST)')
    img, img_metas, gt = data_batch['img'], data_batch['img_metas'], data_batch['gt_semantic_seg']
    if not img.is_cuda:
        raise RuntimeError('EncoderDecoder.train_step needs CUDA(HIP) tensors: pfst_amd has no CPU path')
    st = step_state(model)
    arena = ensure_arena(model, img.device)

    optimizer.zero_grad()
    # the optimizer's zero_grad() may have detached .grad views (set_to_none): re-attach by cached pointer compare + zero the arena
    gp = st.grad_ptrs
    if gp is None or gp[0] != arena.grad.data_ptr():
        base = arena.grad.data_ptr()
        gp = st.grad_ptrs = (base, [(name, p, base + 4 * arena.offsets[name]) for name, p in model.named_parameters()])
    for name, p, ptr in gp[1]:
        g = p.grad
        if g is None or g.data_ptr() != ptr:
            p.grad = arena.view(arena.grad, name)
    arena.zero_grad()
    model.repack_weights(need_dgrad=True)

    gt8 = ops.to_u8(gt.contiguous())
    tape = Tape()

    # data-parallel runs: the pass's marker closures tell the reducer which tail of the gradient arena is final (dist.GradReducer)
    reducer = grad_ready = None
    step_stats = pdist.step_stats_begin()
    if pdist.is_distributed() and pdist.OVERLAP_ALLREDUCE:
        reducer = pdist.GradReducer(arena.grad)
        reducer.stats = step_stats
        cuts = {'heads': arena.offsets[next(n for n in arena.names if not n.startswith('backbone.'))]}
        for n in arena.names:
            stage = n.split('.')[1] if n.startswith('backbone.layer') else None
            if stage and stage not in cuts:
                cuts[stage] = arena.offsets[n]
        grad_ready = lambda stage: reducer.ready(cuts[stage])
    want_vis = bool(getattr(model, 'return_vis_states', False))
    scalars, head_states = model.forward_train(img.contiguous(), img_metas, gt8, None, return_states=True, tape=tape, grad_ready=grad_ready)

    # every log value is a forward result: its packed copy to the host is queued in front of the backward sweep (layers.EARLY_LOG_READ), as
    # the reference reads them (`_parse_losses` before the hook's `loss.backward()`)
    def start_log_read():
        names = list(scalars.keys())
        packed = torch.cat([scalars[k].reshape(1) for k in names])
        host = st.log_host
        if host is None or host.numel() < packed.numel():
            host = st.log_host = torch.empty(max(64, packed.numel()), dtype=torch.float32, pin_memory=True)
        if pdist.is_distributed():
            if st.steps == 0:
                pdist.check_same_keys(names)
            # the mean over ranks of the log vector and its copy run on a stream of their own: the main stream never waits for this collective
            main = torch.cuda.current_stream()
            if st.log_stream is None:
                st.log_stream = torch.cuda.Stream()
            ls = st.log_stream
            ls.wait_stream(main)
            with torch.cuda.stream(ls):
                red = pdist.reduce_log_vector(packed)
                host[:red.numel()].copy_(red, non_blocking=True)
                evt = torch.cuda.Event()
                evt.record()
            packed.record_stream(ls)
            return names, host, packed.numel(), evt
        host[:packed.numel()].copy_(packed, non_blocking=True)
        evt = torch.cuda.Event()
        evt.record()
        return names, host, packed.numel(), evt

    log_read = start_log_read() if layers.EARLY_LOG_READ else None

    tape.backward()
    layers.join_side_stream()

    if pdist.is_distributed():
        if reducer is not None:
            reducer.finish()                       # the tail buckets have been in flight since the heads' backward
        else:
            if step_stats is not None:
                step_stats['bucket_elems'].append(arena.grad.numel())
                ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev[0].record()
            pdist.allreduce_mean_(arena.grad)
            if step_stats is not None:
                ev[1].record()
                step_stats['exposed_allreduce'] = ev
    if step_stats is not None:
        import time
        t_read = time.perf_counter()
    # the step's single blocking read; optimizer.step() is queued in front of it (layers.STEP_BOUNDARY_OVERLAP), so the host enters the next
    # step while the device still runs the backward sweep and the update.  A batch with labels outside [0, C) therefore raises AFTER its
    # update has been applied -- the run is over either way
    names, host, n_log, read_evt = log_read if log_read is not None else start_log_read()
    if layers.STEP_BOUNDARY_OVERLAP:
        optimizer.step()
    read_evt.synchronize()
    if not layers.STEP_BOUNDARY_OVERLAP:
        optimizer.step()
    vals = host[:n_log].tolist()
    if step_stats is not None:
        step_stats['host_read_s'] = time.perf_counter() - t_read
    st.steps += 1
    log_vars = OrderedDict(zip(names, vals))
    for k in [k for k in log_vars if k.rsplit('.', 1)[-1].startswith('_')]:
        v = log_vars.pop(k)                 # not a log value: the CE kernels' count of labels outside [0, C) / ignore_index
        if k.endswith('_bad_labels') and v > 0:
            raise ValueError(f'{int(v)} label values outside [0, {model.num_classes}) other than ignore_index reached the cross-entropy '
                             f'({k}); F.cross_entropy raises on them in the reference -- check reduce_zero_label / the label maps')
    log_vars['loss'] = sum(v for k, v in log_vars.items() if 'loss' in k)

    states = {}
    if want_vis:
        # encoder_decoder.py:153-156: the heads' states plus the batch
        states = {k: (v.data if hasattr(v, 'data') and not torch.is_tensor(v) else v) for k, v in head_states.items()}
        states.update(img=img, gt=gt)
    return dict(loss=log_vars['loss'], log_vars=log_vars, num_samples=len(img_metas), states=states)
