"""The adversarial-adaptation baseline of the reference's model zoo (ADVENT): `DomainAdaptorAdv`, `FCDiscriminator`, `AdvLoss` and the
alternating two-optimizer train step.

Reference: rsiseg/models/segmentors/domain_adaptor_adv.py:30-333 (the segmentor and its train_step), discriminators/fc_discriminator.py:5-23,
losses/adv_loss.py:12-107 (loss_type='advent').

    ent(z)_c = -p_c log2(p_c + 1e-30) / log2(C), p = softmax_c(z): a C-channel map at the logits' own resolution (hip_ops.entropy_map)
    D = 5 x Conv2d(k 4, stride 2, padding 1) with LeakyReLU(0.2) after the first four, then the global mean   (hip_ops.adv_conv*, adv_tail)
    disc:  w mean|D(ent(z_src)) - 0|, w mean|D(ent(z_trg)) - 1|  on detached logits          gen:  w mean|D(ent(z_trg)) - 0|, D frozen

The step on the device, in the reference's order: both generator passes (source with its losses, target up to the logits) on ONE tape;
D forward on both entropy maps, D backward, D step; D forward on ent(z_trg) again with the NEW weights; the packed log vector on its way to
the host; then the backward sweep, which starts with D's input gradient (no weight-gradient launch) and pfst_entropy_map_bwd into the target
pass's logits; the generator's step queued before the step's single blocking read.

Deviations from the reference, all deliberate: the batch is read by name; an auxiliary head is optional (where there is one it
runs on the target features as there, off the tape: no loss reads its logits); disc_steps other than 1 (dead code there: `self.iteration` never advances) raises;
weight_trg is accepted and ignored, as there."""
from collections import OrderedDict

import torch
import torch.nn as nn

from . import dist as pdist
from . import hip_ops as ops
from . import layers
from .engine import ParamArena, Tape
from .models import EncoderDecoder
from .registry import DISCRIMINATORS, LOSSES, SEGMENTORS, build_discriminator, build_loss

BATCH_KEYS = ('img', 'img_metas', 'gt_semantic_seg', 'target_img', 'target_img_metas')
MIN_LOGITS = 32                  # five stride-2 layers: 32 -> 16 -> 8 -> 4 -> 2 -> 1


class _Conv4(nn.Module):
    """the parameters of one Conv2d(cin, cout, kernel_size=4, stride=2, padding=1): default nn.Conv2d initialisation, drawn by nn.Conv2d
    itself so that a seeded build consumes the generator as the reference's does"""

    def __init__(self, cin, cout):
        super().__init__()
        ref_init = nn.Conv2d(cin, cout, kernel_size=4, stride=2, padding=1)
        self.weight = nn.Parameter(ref_init.weight.detach().clone())
        self.bias = nn.Parameter(ref_init.bias.detach().clone())


@DISCRIMINATORS.register_module()
class FCDiscriminator(nn.Module):
    """fc_discriminator.py:5-23.  State-dict keys net.{0,2,4,6,8}.{weight,bias}, as the reference's nn.Sequential (the odd slots are its
    LeakyReLUs, fused into the convolutions' epilogues here; slot 9 its AdaptiveAvgPool2d, part of hip_ops.adv_tail)."""
    SLOPE = 0.2
    CONV_SLOTS = (0, 2, 4, 6, 8)

    def __init__(self, num_in_channels, ndf=64):
        super().__init__()
        widths = [num_in_channels, ndf, ndf * 2, ndf * 4, ndf * 8, 1]
        slots = []
        for i in range(5):
            slots.append(_Conv4(widths[i], widths[i + 1]))
            slots.append(nn.Identity())
        self.net = nn.Sequential(*slots)
        self.num_in_channels, self.ndf = num_in_channels, ndf

    def convs(self):
        return [self.net[i] for i in self.CONV_SLOTS]

    def check_input(self, shape):
        if len(shape) != 4 or shape[1] != self.num_in_channels:
            raise ValueError(f'FCDiscriminator({self.num_in_channels}): input {tuple(shape)}')
        if shape[2] < MIN_LOGITS or shape[3] < MIN_LOGITS:
            raise NotImplementedError(f'FCDiscriminator: a {shape[2]} x {shape[3]} input does not give at least 1 x 1 out of all five stride-2 '
                                      f'convolutions (H and W of the logits must be >= {MIN_LOGITS})')

    def forward_keep(self, e):
        """-> [e, y1, y2, y3, y4, y5]: the input and every layer's output (y1..y4 after their LeakyReLU, y5 the one-channel plane)"""
        self.check_input(e.shape)
        acts = [e]
        for i, m in enumerate(self.convs()):
            acts.append(ops.adv_conv(acts[-1], m.weight.data, m.bias.data, slope=self.SLOPE if i < 4 else None))
        return acts

    def forward(self, e):
        """d [N, 1, 1, 1] as the reference's forward (no tape, nothing kept)"""
        y = self.forward_keep(e)[-1]
        return ops.adv_tail(y, 0.0, 1.0, want_grad=False)[0].view(-1, 1, 1, 1)

    def backward_params(self, acts, gy):
        """gy = dL/dy5: ADDS dL/dw, dL/db of every layer to the parameters' .grad; no data gradient below layer 1"""
        convs, g = self.convs(), gy
        for i in range(4, -1, -1):
            m = convs[i]
            for p in (m.weight, m.bias):
                if p.grad is None:
                    p.grad = torch.zeros_like(p.data)
            ops.adv_conv_wgrad_(m.weight.grad, m.bias.grad, acts[i], g)
            if i > 0:
                g = ops.adv_conv_dgrad_(torch.empty_like(acts[i]), g, m.weight.data, x_gate=acts[i], slope=self.SLOPE)

    def backward_input(self, acts, gy):
        """gy = dL/dy5 -> dL/de with the weights frozen: data gradients only, no weight-gradient launch"""
        convs, g = self.convs(), gy
        for i in range(4, -1, -1):
            g = ops.adv_conv_dgrad_(torch.empty_like(acts[i]), g, convs[i].weight.data, x_gate=acts[i] if i > 0 else None, slope=self.SLOPE)
        return g


def _data(t):
    return t.data if not torch.is_tensor(t) else t


@LOSSES.register_module()
class AdvLoss(nn.Module):
    """adv_loss.py:12-107 with loss_type='advent' (the L1 form: its BCE lines are commented out).  net_type 'disc': loss_disc_src / loss_disc_trg
    on detached logits, gradients to the discriminator; 'gen': loss_gen, gradient to logits_trg and none to the discriminator."""
    SRC_LABEL, TRG_LABEL = 0.0, 1.0
    WEIGHT_KEYS = {'disc': ('loss_disc_src', 'loss_disc_trg'), 'gen': ('loss_gen',)}

    def __init__(self, loss_type='adv_ent', net_type='gen', weights=None, **kwards):
        super().__init__()
        if loss_type != 'advent':
            raise NotImplementedError(f"AdvLoss: loss_type {loss_type!r}; 'advent' (entropy maps, L1 against the domain label) is implemented")
        if net_type not in self.WEIGHT_KEYS:
            raise ValueError(f"AdvLoss: net_type must be 'gen' or 'disc', got {net_type!r}")
        keys = self.WEIGHT_KEYS[net_type]
        if not isinstance(weights, dict) or any(k not in weights for k in keys):
            raise KeyError(f'AdvLoss(net_type={net_type!r}) reads weights{list(keys)}: weights must be a dict with these keys, got {weights!r}')
        self.loss_type, self.net_type = loss_type, net_type
        self._loss_name = f'adv_loss_{loss_type}_{net_type}'
        self.weights = dict(weights)

    @property
    def loss_name(self):
        return self._loss_name

    def forward(self, discriminator, tensors, tape=None):
        """tensors: logits_src / logits_trg (engine.Var or tensors, low-resolution logits).  tape: where the backward closures go -- for
        'disc' a tape of the discriminator's own (run before its optimizer steps), for 'gen' the generator's tape"""
        out = OrderedDict()
        if self.net_type == 'disc':
            for key, name, label in (('loss_disc_src', 'logits_src', self.SRC_LABEL), ('loss_disc_trg', 'logits_trg', self.TRG_LABEL)):
                acts = discriminator.forward_keep(ops.entropy_map(_data(tensors[name])))
                _, loss, gy = ops.adv_tail(acts[-1], label, float(self.weights[key]), want_grad=tape is not None)
                out[key] = loss
                if tape is not None:
                    tape.record(lambda acts=acts, gy=gy: discriminator.backward_params(acts, gy),
                                tag=dict(op='adv_disc', out=None, module=self, logits=tensors[name]))
            return out
        lt = tensors['logits_trg']
        z = _data(lt)
        acts = discriminator.forward_keep(ops.entropy_map(z))
        _, loss, gy = ops.adv_tail(acts[-1], self.SRC_LABEL, float(self.weights['loss_gen']), want_grad=tape is not None)
        out['loss_gen'] = loss
        if tape is not None:
            if torch.is_tensor(lt):
                raise TypeError('AdvLoss(net_type="gen") with a tape needs logits_trg as an engine.Var (the gradient goes to its slot)')

            def bwd():
                g_ent = discriminator.backward_input(acts, gy)
                buf, acc = lt.grad_target()
                ops.entropy_map_bwd_(buf, z, g_ent, accumulate=acc)
            tape.record(bwd, tag=dict(op='adv_gen', out=None, module=self, logits_trg=lt))
        return out


@SEGMENTORS.register_module()
class DomainAdaptorAdv(EncoderDecoder):
    """domain_adaptor_adv.py:30-333: an EncoderDecoder (inference, checkpoints keys backbone.* / decode_head.* / auxiliary_head.*) plus a
    discriminator (discriminator.*) and the alternating train step.  `generator` / `discriminator` are what `optimizer=dict(generator=...,
    discriminator=...)` addresses (optim.build_optimizers)."""

    def __init__(self, backbone, decode_head, discriminator=None, disc_losses=None, gen_losses=None, neck=None, auxiliary_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None, weight_trg=1.0):
        if neck is not None:
            raise NotImplementedError('DomainAdaptorAdv: neck is outside the PFST path')
        super().__init__(backbone, decode_head, neck=None, auxiliary_head=auxiliary_head, train_cfg=train_cfg, test_cfg=test_cfg,
                         pretrained=pretrained, init_cfg=init_cfg)
        disc_steps = train_cfg.get('disc_steps', 1) if train_cfg is not None else 1
        if disc_steps != 1:
            raise NotImplementedError(f'DomainAdaptorAdv: train_cfg.disc_steps = {disc_steps}; the reference never advances its iteration '
                                      'counter, so every value but 1 is dead code there -- absent or 1 only')
        if discriminator is None:
            raise ValueError('DomainAdaptorAdv needs a discriminator cfg (e.g. dict(type="FCDiscriminator", num_in_channels=num_classes))')
        self.disc_steps = disc_steps
        self.weight_trg = weight_trg            # unused, as in the reference
        self.discriminator = build_discriminator(discriminator)

        def build_list(cfgs):
            if cfgs is None:
                return None
            return nn.ModuleList([build_loss(c) for c in (cfgs if isinstance(cfgs, (list, tuple)) else [cfgs])])
        self.disc_losses, self.gen_losses = build_list(disc_losses), build_list(gen_losses)

    @property
    def generator(self):
        mods = [self.backbone, self.decode_head]
        if self.with_auxiliary_head:
            mods.append(self.auxiliary_head)
        return nn.ModuleList(mods)

    def generator_named_parameters(self):
        return [(n, p) for n, p in self.named_parameters() if not n.startswith('discriminator.')]

    def train_step(self, data_batch, optimizer, **kwargs):
        """One adversarial iteration on a UDADataset batch (img, img_metas, gt_semantic_seg, target_img, target_img_metas; other keys are
        ignored) with optimizer = {'generator': ..., 'discriminator': ...} -> dict(loss, log_vars, num_samples, states)."""
        return train_step(self, data_batch, optimizer)

    @property
    def param_arena(self):
        """the generator's flat parameter / gradient arena (None before the first train_step)"""
        return step_state(self).arenas[0]

    @property
    def disc_param_arena(self):
        return step_state(self).arenas[1]


class _GeneratorView:
    """what ParamArena.sync needs of a model, restricted to the generator's part of a DomainAdaptorAdv"""

    def __init__(self, model):
        self.model = model

    def module_tree_version(self):
        return self.model.module_tree_version()

    def named_parameters(self):
        return self.model.generator_named_parameters()

    def modules(self):
        return [m for n, m in self.model.named_modules() if not (n + '.').startswith('discriminator.')]


class _StepState:
    __slots__ = ('arenas', 'grad_ptrs', 'log_host', 'log_stream', 'steps')

    def __init__(self):
        self.arenas = (None, None)
        self.grad_ptrs = [None, None]
        self.log_host = self.log_stream = None
        self.steps = 0


def step_state(model):
    st = model.__dict__.get('_adv_state')
    if st is None:
        st = model.__dict__['_adv_state'] = _StepState()
    return st


def ensure_arenas(model, device):
    """(generator arena, discriminator arena) on `device`, built on the first step and kept in step with the model (ParamArena.sync)"""
    st = step_state(model)
    if st.arenas[0] is None or st.arenas[0].data.device != device:
        model.to(device)
        st.arenas = (ParamArena(model.generator_named_parameters(), device, with_grad=True),
                     ParamArena(list(model.discriminator.named_parameters()), device, with_grad=True))
        st.grad_ptrs = [None, None]
    st.arenas[0].sync(_GeneratorView(model))
    st.arenas[1].sync(model.discriminator)
    return st.arenas


def _attach_grads(st, which, arena, named):
    """the optimizer's zero_grad() may have detached .grad views: re-attach by cached pointer compare, then zero the arena with one fill"""
    gp = st.grad_ptrs[which]
    if gp is None or gp[0] != arena.grad.data_ptr():
        base = arena.grad.data_ptr()
        gp = st.grad_ptrs[which] = (base, [(name, p, base + 4 * arena.offsets[name]) for name, p in named()])
    for name, p, ptr in gp[1]:
        g = p.grad
        if g is None or g.data_ptr() != ptr:
            p.grad = arena.view(arena.grad, name)
    arena.zero_grad()


def train_step(model, data_batch, optimizer):
    missing = [k for k in BATCH_KEYS if k not in data_batch]
    if missing:
        raise KeyError(f'DomainAdaptorAdv.train_step reads a source / target batch by name {BATCH_KEYS}; missing keys {missing}')
    if not (hasattr(optimizer, 'keys') and 'generator' in optimizer and 'discriminator' in optimizer):
        raise TypeError("DomainAdaptorAdv.train_step takes optimizer = {'generator': ..., 'discriminator': ...} (optim.build_optimizers)")
    if model.disc_losses is None or model.gen_losses is None:
        raise ValueError('DomainAdaptorAdv.train_step needs disc_losses and gen_losses')
    img, img_metas, gt = data_batch['img'], data_batch['img_metas'], data_batch['gt_semantic_seg']
    timg, timg_metas = data_batch['target_img'], data_batch['target_img_metas']
    if not (img.is_cuda and timg.is_cuda):
        raise RuntimeError('DomainAdaptorAdv.train_step needs CUDA(HIP) tensors: pfst_amd has no CPU path')
    opt_g, opt_d = optimizer['generator'], optimizer['discriminator']
    st = step_state(model)
    gen_arena, disc_arena = ensure_arenas(model, img.device)
    disc = model.discriminator

    opt_d.zero_grad()
    opt_g.zero_grad()
    _attach_grads(st, 0, gen_arena, model.generator_named_parameters)
    _attach_grads(st, 1, disc_arena, lambda: list(disc.named_parameters()))
    model.repack_weights(need_dgrad=True)

    # ---- the generator's two passes on one tape (domain_adaptor_adv.py:264-284)
    gt8 = ops.to_u8(gt.contiguous())
    tape = Tape()
    scalars, head_states = model.forward_train(img.contiguous(), img_metas, gt8, None, return_states=True, tape=tape)
    logits_src = head_states['seg_logits']
    x_trg = model.extract_feat(timg.contiguous(), tape)
    logits_trg, _ = model.decode_head.forward(x_trg, return_features=True, tape=tape, training=True)
    disc.check_input(logits_trg.data.shape)
    if model.with_auxiliary_head:
        # :281-284 runs the auxiliary head on the target features too.  No loss reads its logits (AdvLoss takes the decode head's), so it
        # runs off the tape: what remains of it is what the reference's checkpoints carry -- the head's BatchNorm running statistics over
        # both domains and its draw from the dropout stream
        model.auxiliary_head.forward(x_trg, tape=None, training=True)
    tensors = dict(img_src=img, img_trg=timg, logits_src=logits_src, logits_trg=logits_trg)

    # ---- discriminator loss, backward, step (:296-305)
    dtape = Tape()
    for loss_module in model.disc_losses:
        scalars.update(loss_module(disc, tensors, tape=dtape))
    dtape.backward()
    if pdist.is_distributed():
        pdist.allreduce_mean_(disc_arena.grad)
    opt_d.step()

    # ---- generator loss with the UPDATED, frozen discriminator (:307-310): its backward closure goes onto the generator's tape
    for loss_module in model.gen_losses:
        scalars.update(loss_module(disc, tensors, tape=tape))

    def start_log_read():
        names = list(scalars.keys())
        packed = torch.cat([scalars[k].reshape(1) for k in names])
        host = st.log_host
        if host is None or host.numel() < packed.numel():
            host = st.log_host = torch.empty(max(64, packed.numel()), dtype=torch.float32, pin_memory=True)
        if pdist.is_distributed():
            if st.steps == 0:
                pdist.check_same_keys(names)
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

    # ---- the generator's backward sweep (:312-318): D's input gradient and the entropy map's adjoint first, then the target and source passes
    tape.backward()
    layers.join_side_stream()
    if pdist.is_distributed():
        pdist.allreduce_mean_(gen_arena.grad)
    names, host, n_log, read_evt = log_read if log_read is not None else start_log_read()
    if layers.STEP_BOUNDARY_OVERLAP:
        opt_g.step()
    read_evt.synchronize()                   # the step's single blocking read
    if not layers.STEP_BOUNDARY_OVERLAP:
        opt_g.step()
    vals = host[:n_log].tolist()
    st.steps += 1
    log_vars = OrderedDict(zip(names, vals))
    for k in [k for k in log_vars if k.rsplit('.', 1)[-1].startswith('_')]:
        v = log_vars.pop(k)
        if k.endswith('_bad_labels') and v > 0:
            raise ValueError(f'{int(v)} label values outside [0, {model.num_classes}) other than ignore_index reached the cross-entropy '
                             f'({k}); F.cross_entropy raises on them in the reference -- check reduce_zero_label / the label maps')
    # what the generator's optimizer minimises (:312-314): the source pass's losses + loss_gen
    loss = sum(v for k, v in log_vars.items() if 'loss' in k and not k.startswith('loss_disc'))
    return dict(loss=loss, log_vars=log_vars, num_samples=len(img_metas) + len(timg_metas), states={})
