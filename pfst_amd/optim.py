"""AdamW + poly LR schedule of the reference recipe (configs/_base_/schedules/adamw_40k.py:4-16) and the SGD of its supervised
schedules (configs/_base_/schedules/schedule_{20k,...,320k}.py) on the flat parameter arena: one kernel launch per step for all
43.6 M parameters."""
import torch

from . import hip_ops as ops


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (amsgrad=False).  Parameters that live in a pfst_amd ParamArena are
    updated by ONE flat launch; any other CUDA parameter gets the same kernel per tensor."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._flat = {}   # id(arena) -> dict(m, v, step)
        self.grad_scale = 1.0

    def zero_grad(self, set_to_none=False):
        # gradients live in the arena; PFGST.forward_train zeroes it with one fill kernel
        for g in self.param_groups:
            for p in g['params']:
                if not hasattr(p, '_pfst_arena') and p.grad is not None:
                    p.grad = None

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            by_arena, loose = {}, []
            for p in group['params']:
                a = getattr(p, '_pfst_arena', None)
                (by_arena.setdefault(id(a), (a, []))[1] if a is not None else loose).append(p)
            for a, plist in by_arena.values():
                covered = sum((p.numel() + 3) // 4 * 4 for p in plist)
                if covered != a.numel:
                    loose.extend(plist)       # only part of the arena is optimised: per-tensor launches
                    continue
                if id(a) not in self._flat:
                    pend = getattr(self, '_pending_flat', None)
                    if pend:
                        p0 = pend.pop(0)
                        self._flat[id(a)] = dict(m=p0['m'].to(a.data.device), v=p0['v'].to(a.data.device), step=p0['step'])
                    else:
                        self._flat[id(a)] = dict(m=torch.zeros_like(a.data), v=torch.zeros_like(a.data), step=0)
                st = self._flat[id(a)]
                st['step'] += 1
                ops.adamw_step_(a.data, a.grad, st['m'], st['v'], group['lr'], group['betas'], group['eps'],
                                group['weight_decay'], st['step'], self.grad_scale)
            for p in loose:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st.update(m=torch.zeros_like(p.data), v=torch.zeros_like(p.data), step=0)
                st['step'] += 1
                ops.adamw_step_(p.data, p.grad.contiguous(), st['m'], st['v'], group['lr'], group['betas'], group['eps'],
                                group['weight_decay'], st['step'], self.grad_scale)


    def state_dict(self):
        sd = super().state_dict()
        # attached arenas in first-step order, then what load_state_dict() left waiting for arenas that have not stepped yet (step() takes
        # those from the front): a checkpoint written between a resume and the first step keeps the moments and the step count
        sd['pfst_flat'] = [dict(m=st['m'].cpu(), v=st['v'].cpu(), step=st['step']) for st in self._flat.values()]
        sd['pfst_flat'] += [dict(st) for st in getattr(self, '_pending_flat', None) or []]
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        flat = sd.pop('pfst_flat', [])
        super().load_state_dict(sd)
        self._pending_flat = list(flat)       # attached to the arenas on the first step() after the model is on the GPU


class SGD(torch.optim.Optimizer):
    """torch.optim.SGD semantics (maximize=False).  Parameters that cover a whole pfst_amd ParamArena are updated by ONE flat launch, with the
    momentum buffer as one flat tensor; any other CUDA parameter gets the same kernel per tensor."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f'invalid SGD settings: lr={lr}, momentum={momentum}, weight_decay={weight_decay}')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov))
        self._flat = {}   # id(arena) -> dict(buf, stepped)
        self.grad_scale = 1.0

    def zero_grad(self, set_to_none=False):
        # gradients live in the arena; the train step zeroes it with one fill kernel
        for g in self.param_groups:
            for p in g['params']:
                if not hasattr(p, '_pfst_arena') and p.grad is not None:
                    p.grad = None

    def _launch(self, group, p, g, st):
        mom = group['momentum']
        if mom != 0 and st['buf'] is None:
            st['buf'] = torch.empty_like(p)          # written, not read, by the first step
        ops.sgd_step_(p, g, st['buf'] if mom != 0 else None, group['lr'], mom, group['dampening'], group['weight_decay'],
                      group['nesterov'], not st['stepped'], self.grad_scale)
        st['stepped'] = True

    @torch.no_grad()
    def step(self, closure=None):
        for group in self.param_groups:
            by_arena, loose = {}, []
            for p in group['params']:
                a = getattr(p, '_pfst_arena', None)
                (by_arena.setdefault(id(a), (a, []))[1] if a is not None else loose).append(p)
            for a, plist in by_arena.values():
                covered = sum((p.numel() + 3) // 4 * 4 for p in plist)
                if covered != a.numel:
                    loose.extend(plist)       # only part of the arena is optimised: per-tensor launches
                    continue
                if id(a) not in self._flat:
                    pend = getattr(self, '_pending_flat', None)
                    if pend:
                        p0 = pend.pop(0)
                        self._flat[id(a)] = dict(buf=None if p0['buf'] is None else p0['buf'].to(a.data.device), stepped=bool(p0['stepped']))
                    else:
                        self._flat[id(a)] = dict(buf=None, stepped=False)
                self._launch(group, a.data, a.grad, self._flat[id(a)])
            for p in loose:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st.update(buf=None, stepped=False)
                self._launch(group, p.data, p.grad.contiguous(), st)

    def state_dict(self):
        sd = super().state_dict()
        # as AdamW.state_dict: the attached arenas, then the loaded entries no step() has attached yet
        sd['pfst_flat'] = [dict(buf=None if st['buf'] is None else st['buf'].cpu(), stepped=st['stepped']) for st in self._flat.values()]
        sd['pfst_flat'] += [dict(st) for st in getattr(self, '_pending_flat', None) or []]
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        flat = sd.pop('pfst_flat', [])
        super().load_state_dict(sd)
        self._pending_flat = list(flat)       # attached to the arenas on the first step() after the model is on the GPU


def build_optimizer(model, cfg):
    """rsiseg/core/builder.py:12-34 for the shipped configs: AdamW (adamw_40k.py) or SGD (schedule_*.py) over all requires_grad parameters."""
    cfg = dict(cfg)
    t = cfg.pop('type')
    params = [p for p in model.parameters() if p.requires_grad]
    if t == 'SGD':
        if cfg.get('paramwise_cfg') is not None:
            raise NotImplementedError('paramwise_cfg is not implemented: every parameter takes the optimizer\'s own lr / weight_decay')
        cfg.pop('paramwise_cfg', None)
        return SGD(params, **cfg)
    if t != 'AdamW':
        raise NotImplementedError(f'optimizer {t}: AdamW (the PFST recipe) and SGD (the supervised schedules) are implemented')
    cfg.pop('paramwise_cfg', None)
    return AdamW(params, **cfg)


class OptimizerDict(dict):
    """{name: optimizer} as mmcv's build_optimizers returns for a GAN-style model, plus what the runner drives a single optimizer through:
    `param_groups` (the groups of every optimizer, in key order -- the same dict objects, so a learning rate written there lands in its
    optimizer), `zero_grad`, and `state_dict` / `load_state_dict` as {name: state}"""

    @property
    def param_groups(self):
        return [g for opt in self.values() for g in opt.param_groups]

    def zero_grad(self, set_to_none=False):
        for opt in self.values():
            opt.zero_grad(set_to_none)

    def state_dict(self):
        return {k: opt.state_dict() for k, opt in self.items()}

    def load_state_dict(self, sd):
        if set(sd) != set(self):
            raise KeyError(f'optimizer state for {sorted(sd)}, this run has {sorted(self)}')
        for k, opt in self.items():
            opt.load_state_dict(sd[k])


def build_optimizers(model, cfg):
    """mmcv.runner.build_optimizers: a cfg whose values are all dicts and which has no `type` key of its own -- e.g.
    dict(generator=dict(type='AdamW', ...), discriminator=dict(type='AdamW', ...)) -- builds one optimizer per key over getattr(model, key)
    and returns them as an OptimizerDict; any other cfg is build_optimizer's"""
    if 'type' not in cfg and len(cfg) > 0 and all(isinstance(v, dict) for v in cfg.values()):
        out = OptimizerDict()
        for key, sub in cfg.items():
            part = getattr(model, key, None)
            if part is None:
                raise AttributeError(f'optimizer[{key!r}]: {type(model).__name__} has no sub-module `{key}`')
            out[key] = build_optimizer(part, sub)
        return out
    return build_optimizer(model, cfg)


def poly_lr(base_lr, it, max_iters, power=1.0, min_lr=0.0, warmup_iters=1500, warmup_ratio=1e-6):
    """mmcv PolyLrUpdaterHook + linear warm-up (adamw_40k.py:8-16), by iteration."""
    coeff = (1 - it / max_iters) ** power
    lr = (base_lr - min_lr) * coeff + min_lr
    if it < warmup_iters:
        k = (1 - it / warmup_iters) * (1 - warmup_ratio)
        lr = lr * (1 - k)
    return lr
