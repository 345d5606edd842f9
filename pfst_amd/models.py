"""ResNetV1c-50-d8 backbone, DepthwiseSeparableASPPHead, FCNHead, CrossEntropyLoss and EncoderDecoder on
the HIP ops, registered under the reference's type names so `configs/pfst/*.py` build unchanged.

Reference behaviour followed (file:line under /root/reference/rsiseg/models):
  backbones/resnet.py:99-307,396-527,591-638,659-700  utils/res_layer.py:28-96
  decode_heads/decode_head.py:55-108,188-283  aspp_head.py:53-126  sep_aspp_head.py:29-111  fcn_head.py:24-98
  segmentors/encoder_decoder.py:65-217  losses/cross_entropy_loss.py:198-298
Only what the PFST hot path uses is implemented; unsupported options raise instead of silently differing."""
import os

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops as ops
from . import layers as layers_mod
from .engine import Var
from .layers import (BatchNorm2dP, Conv2dP, ConvModule, DepthwiseSeparableConvModule, WeightBatch, bn_eval, conv_bn_act,
                     conv_forward, dwsep_branches)
from .registry import (BACKBONES, HEADS, LOSSES, NECKS, PIXEL_SAMPLERS, SEGMENTORS, add_prefix, build_backbone, build_head, build_loss,
                       build_neck, build_pixel_sampler)


# False: the decode head's Dropout2d as a scaling pass of its own (the fold on / off test); default: folded into sep_bottleneck[1]'s normalisation
FOLD_DROPOUT = True


def xin_dev(v):
    return (v.data if v.lazy is None else v.lazy[0]).device


def _check_norm(norm_cfg):
    if norm_cfg is None or norm_cfg.get('type') != 'BN':
        raise NotImplementedError(f'pfst_amd implements plain BN (the PFST configs); got norm_cfg={norm_cfg}')


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=False):
        super().__init__()
        self.conv1 = Conv2dP(inplanes, planes, 1)
        self.bn1 = BatchNorm2dP(planes)
        self.conv2 = Conv2dP(planes, planes, 3, stride, dilation, dilation)   # style='pytorch': stride on the 3x3
        self.bn2 = BatchNorm2dP(planes)
        self.conv3 = Conv2dP(planes, planes * 4, 1)
        self.bn3 = BatchNorm2dP(planes * 4)
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(Conv2dP(inplanes, planes * 4, 1, stride), BatchNorm2dP(planes * 4))

    def forward(self, x, tape):
        # Three of the block's four normalised tensors have ONE reader that can normalise on load (the layers.folds_into_* predicates say when;
        # layers.norm_plan whether the producing layer can oblige) and are then never written: y1 where conv2 runs through the Winograd domain
        # (layer2.1 ... layer4.2: its input transform normalises; the weight gradient of conv2 comes from the transformed input kept in forward,
        # BatchNorm backward of bn1 from the pre-BN tensor), y2 where conv3 is a 1x1 on the 256-row f16x3 tile (its GEMM normalises between load
        # and split, and so does its weight gradient), the downsample branch as the residual operand of bn3's normalisation pass
        h, w = x.data.shape[-2:]
        o = conv_bn_act(x, self.conv1, self.bn1, tape, defer=layers_mod.folds_into_wino(self.conv2, h, w, tape is not None))
        s2 = self.conv2.stride
        o = conv_bn_act(o, self.conv2, self.bn2, tape, defer=layers_mod.folds_into_gemm(self.conv3, (h // s2) * (w // s2)))
        idt = x
        if self.downsample is not None:
            idt = conv_bn_act(x, self.downsample[0], self.downsample[1], tape, relu=False, defer=layers_mod.folds_into_residual())
        return conv_bn_act(o, self.conv3, self.bn3, tape, relu=True, residual=idt)


@BACKBONES.register_module()
class ResNetV1c(nn.Module):
    """ResNet-50 with the 3x(3x3) deep stem, strides (1,2,1,1), dilations (1,1,2,4), contract_dilation."""
    arch = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}

    def __init__(self, depth=50, in_channels=3, stem_channels=64, base_channels=64, num_stages=4,
                 strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch',
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, contract_dilation=False,
                 multi_grid=None, with_cp=False, zero_init_residual=True, pretrained=None, init_cfg=None,
                 frozen_stages=-1, conv_cfg=None, dcn=None, plugins=None, avg_down=False, deep_stem=True,
                 stage_with_dcn=(False, False, False, False)):
        super().__init__()
        _check_norm(norm_cfg)
        if depth not in self.arch:
            raise KeyError(f'invalid depth {depth} for resnet')
        unsupported = dict(style=style != 'pytorch', norm_eval=norm_eval, multi_grid=multi_grid is not None, with_cp=with_cp,
                           frozen_stages=frozen_stages >= 0, conv_cfg=conv_cfg is not None, dcn=dcn is not None,
                           plugins=plugins is not None, avg_down=avg_down, deep_stem=not deep_stem)
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f'ResNetV1c options outside the PFST path: {bad}')
        self.pretrained = pretrained
        self.out_indices = tuple(out_indices)
        self.zero_init_residual = zero_init_residual
        c2 = stem_channels // 2
        ident = nn.Identity
        self.stem = nn.Sequential(Conv2dP(in_channels, c2, 3, 2, 1), BatchNorm2dP(c2), ident(),
                                  Conv2dP(c2, c2, 3, 1, 1), BatchNorm2dP(c2), ident(),
                                  Conv2dP(c2, stem_channels, 3, 1, 1), BatchNorm2dP(stem_channels), ident())
        inplanes = stem_channels
        self.res_layers = []
        for i, nb in enumerate(self.arch[depth][:num_stages]):
            planes = base_channels * 2 ** i
            stride, dil = strides[i], dilations[i]
            first_dil = dil // 2 if (dil > 1 and contract_dilation) else dil
            blocks = [Bottleneck(inplanes, planes, stride, first_dil, downsample=(stride != 1 or inplanes != planes * 4))]
            inplanes = planes * 4
            for _ in range(1, nb):
                blocks.append(Bottleneck(inplanes, planes, 1, dil))
            name = f'layer{i + 1}'
            self.add_module(name, nn.Sequential(*blocks))
            self.res_layers.append(name)

    def init_weights(self):
        """resnet.py:430-452 with pretrained=None: Kaiming (fan_out, relu) convolutions -- done at construction --, BatchNorm weight 1 /
        bias 0, and with zero_init_residual the LAST norm of every Bottleneck starts at 0 (each block starts as the identity).
        A `pretrained` checkpoint path is loaded instead (mmcv 'Pretrained' init: backbone keys, strict=False); model-zoo URLs such as
        open-mmlab://resnet50_v1c cannot be resolved here (no network) and fail loudly."""
        if self.pretrained is not None:
            import os
            if not (isinstance(self.pretrained, str) and os.path.exists(self.pretrained)):
                raise FileNotFoundError(f'pretrained={self.pretrained!r} is not a local checkpoint file (no network here): pass a file, '
                                        'use --load-from, or set pretrained=None for random initialisation')
            ckpt = torch.load(self.pretrained, map_location='cpu', weights_only=False)
            sd = ckpt.get('state_dict', ckpt)
            sd = {(k[len('backbone.'):] if k.startswith('backbone.') else k): v for k, v in sd.items()}
            self.load_state_dict(sd, strict=False)
            return
        for m in self.modules():
            if isinstance(m, BatchNorm2dP):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)

    def forward(self, x, tape=None, grad_ready=None):
        """grad_ready (data-parallel runs, last pass of the backward sweep only): callable(stage) recorded as marker closures --
        when marker `layer{i}` runs in backward, the gradients of layer{i} and of everything after it are final"""
        s = self.stem
        x = conv_bn_act(x, s[0], s[1], tape)
        x = conv_bn_act(x, s[3], s[4], tape)
        x = conv_bn_act(x, s[6], s[7], tape, defer=True)     # its only consumer, the max-pool, normalises on load: stem.6's output is never written
        xin = x
        pool_amax = ops.amax_slots(xin_dev(xin)) if layers_mod.CONV_MATH == 'f16x3' else None     # layer1's f16x3 GEMMs read the pooled map
        if xin.lazy is not None:
            y, idx = ops.maxpool(xin.lazy[0], bnl=xin.lazy[1], amax=pool_amax)
        else:
            y, idx = ops.maxpool(xin.data, amax=pool_amax)
        in_hw = tuple((xin.data if xin.lazy is None else xin.lazy[0]).shape[-2:])
        x = Var(y, tape is not None)
        x.amax = pool_amax
        if tape is not None:
            pooled = x

            def bwd_pool():
                xin._grad = ops.maxpool_bwd(pooled.grad, idx, in_hw)
                pooled.free_grad()
            tape.record(bwd_pool, dict(op='maxpool', name='backbone.maxpool', x=xin, out=pooled))
        outs = []
        for i, name in enumerate(self.res_layers):
            if grad_ready is not None and tape is not None:
                tape.record(lambda name=name: grad_ready(name))
            for blk in getattr(self, name):
                x = blk(x, tape)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)


def _load_pretrained_backbone(module, pretrained):
    """mmcv's 'Pretrained' init from a LOCAL checkpoint (backbone keys, strict=False); model-zoo URLs cannot be resolved here and fail loudly"""
    if not (isinstance(pretrained, str) and os.path.exists(pretrained)):
        raise FileNotFoundError(f'pretrained={pretrained!r} is not a local checkpoint file (no network here): pass a file, '
                                'use --load-from, or set pretrained=None for random initialisation')
    ckpt = torch.load(pretrained, map_location='cpu', weights_only=False)
    sd = ckpt.get('state_dict', ckpt)
    sd = {(k[len('backbone.'):] if k.startswith('backbone.') else k): v for k, v in sd.items()}
    module.load_state_dict(sd, strict=False)


class BasicBlock(nn.Module):
    """backbones/resnet.py BasicBlock: conv3x3 -> bn1 -> ReLU -> conv3x3 -> bn2 (+ identity) -> ReLU"""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=False):
        super().__init__()
        self.conv1 = Conv2dP(inplanes, planes, 3, stride, dilation, dilation)
        self.bn1 = BatchNorm2dP(planes)
        self.conv2 = Conv2dP(planes, planes, 3, 1, 1, 1)
        self.bn2 = BatchNorm2dP(planes)
        self.downsample = None
        if downsample:
            self.downsample = nn.Sequential(Conv2dP(inplanes, planes, 1, stride), BatchNorm2dP(planes))

    def forward(self, x, tape):
        o = conv_bn_act(x, self.conv1, self.bn1, tape)
        idt = x
        if self.downsample is not None:
            idt = conv_bn_act(x, self.downsample[0], self.downsample[1], tape, relu=False, defer=layers_mod.folds_into_residual())
        return conv_bn_act(o, self.conv2, self.bn2, tape, relu=True, residual=idt)


def _make_res_layer(block, inplanes, planes, blocks, stride=1):
    layers = [block(inplanes, planes, stride, downsample=(stride != 1 or inplanes != planes * block.expansion))]
    layers += [block(planes * block.expansion, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


def _conv_bn_seq(cin, cout, k, stride, relu):
    """(0: conv, 1: BN[, 2: the parameter-less place of the reference's ReLU]) -- the indices of the reference's Sequentials"""
    return nn.Sequential(Conv2dP(cin, cout, k, stride, k // 2), BatchNorm2dP(cout), *([nn.Identity()] if relu else []))


# False: the exchange unit's backward writes the gated gradient into a buffer of its own and adds it to dL/dx_i with one more pass per output
# (tests/test_hrnet_gpu.py compares the two wirings bit for bit)
HR_SHARE_GATED = True


class UpsamplePlace(nn.Module):
    """the parameter-less place of the reference's `Upsample(scale_factor=2^(j-i), mode='bilinear')` at index 2 of an up path's Sequential: it keeps
    the indices, the interpolation itself happens inside the exchange launch"""

    def __init__(self, scale_factor):
        super().__init__()
        self.scale_factor = scale_factor


class HRModule(nn.Module):
    """backbones/hrnet.py:14-214: num_branches parallel branches of blocks, then the exchange unit -- output i is
    relu(sum_j t_ij), t_ii = x_i, t_ij = BN(conv3x3/s2 chain(x_j)) for j < i, t_ij = bilinear_up(BN(conv1x1(x_j)), 2^(j-i)) for j > i, summed in
    branch order.  One pfst_hr_fuse launch per output (csrc/hrnet.hip): the last conv -> BN of every fuse path is deferred,
    its normalised tensor never written; the coarser members are interpolated as they are read.  Where a coarser member's grid times 2^(j-i) is
    not the output grid (inputs whose sides are no multiple of 32) the reference interpolates twice, and the output takes the composition of
    the existing ops instead (correct and slow)."""

    def __init__(self, num_branches, block, num_blocks, in_channels, num_channels, multiscale_output=True):
        super().__init__()
        if not (num_branches == len(num_blocks) == len(num_channels) == len(in_channels)):
            raise ValueError(f'NUM_BRANCHES({num_branches}) <> NUM_BLOCKS({len(num_blocks)}) / NUM_CHANNELS({len(num_channels)}) / '
                             f'NUM_INCHANNELS({len(in_channels)})')
        if num_branches > ops.HR_MAX_BRANCHES:
            raise NotImplementedError(f'HRModule: up to {ops.HR_MAX_BRANCHES} branches, got {num_branches}')
        self.num_branches, self.multiscale_output = num_branches, multiscale_output
        self.in_channels = in_channels                    # the caller's list, updated in place as the reference does
        self.branches = nn.ModuleList()
        for b in range(num_branches):
            self.branches.append(_make_res_layer(block, in_channels[b], num_channels[b], num_blocks[b]))
            in_channels[b] = num_channels[b] * block.expansion
        self.fuse_layers = None
        if num_branches > 1:
            self.fuse_layers = nn.ModuleList()
            for i in range(num_branches if multiscale_output else 1):
                row = []
                for j in range(num_branches):
                    if j > i:
                        row.append(nn.Sequential(Conv2dP(in_channels[j], in_channels[i], 1), BatchNorm2dP(in_channels[i]), UpsamplePlace(2 ** (j - i))))
                    elif j == i:
                        row.append(None)
                    else:
                        row.append(nn.Sequential(*[_conv_bn_seq(in_channels[j], in_channels[i] if k == i - j - 1 else in_channels[j], 3, 2,
                                                                relu=k != i - j - 1) for k in range(i - j)]))
                self.fuse_layers.append(nn.ModuleList(row))

    def _path(self, i, j, x, tape, defer):
        """fuse path (i, j) up to and including its last conv -> BN (no ReLU there): deferred on the fused route"""
        fl = self.fuse_layers[i][j]
        if j > i:
            return conv_bn_act(x, fl[0], fl[1], tape, relu=False, defer=defer)
        for k, seq in enumerate(fl):
            last = k == len(fl) - 1
            x = conv_bn_act(x, seq[0], seq[1], tape, relu=not last, defer=defer if last else False)
        return x

    def forward(self, xs, tape):
        xs = list(xs)
        for b in range(self.num_branches):
            for blk in self.branches[b]:
                xs[b] = blk(xs[b], tape)
        if self.fuse_layers is None:
            return xs
        B, n_out = self.num_branches, len(self.fuse_layers)
        hws = [tuple(x.data.shape[-2:]) for x in xs]
        fused = [all(ops.hr_fuse_exact(hws[i], hws[j]) for j in range(i + 1, B)) and B - 1 - i <= ops.FPN_MAX_LEVELS for i in range(n_out)]
        defer = [layers_mod.folds_into_residual() if f else False for f in fused]
        # Recording order.  In backward the exchange of output i hands ONE buffer gy_i to x_i (as its gradient, where nothing was written yet) and
        # to every same-grid member of output i (as upstream gradient): nothing may add to dL/dx_i before the paths (i, j < i) have read gy_i.  The
        # writers of dL/dx_i are the paths (i', i).  Recorded as: up paths, down paths by DESCENDING output, then the exchanges -- backward runs
        # every exchange first, then the down paths by ascending output (path (i, j) reads gy_i before any (i' > i, i) adds to it, and adds to
        # gy_j only after the paths (j, .) have read it), then the up paths.
        t = [[None] * B for _ in range(n_out)]
        for i in range(n_out):
            for j in range(i + 1, B):
                t[i][j] = self._path(i, j, xs[j], tape, defer[i])
        for i in reversed(range(n_out)):
            for j in range(i):
                t[i][j] = self._path(i, j, xs[j], tape, defer[i])
        for i in range(n_out):
            for j in range(i):
                got = tuple((t[i][j].data if t[i][j].lazy is None else t[i][j].lazy[0]).shape[-2:])
                if got != hws[i]:
                    raise ValueError(f'HRModule: the stride-2 chain from branch {j} ends on {got}, branch {i} is on {hws[i]}')
        return [(self._exchange if fused[i] else self._exchange_composed)(i, xs, t[i], tape) for i in range(n_out)]

    @staticmethod
    def _out_var(dev, tape):
        out = Var(None, tape is not None)
        if layers_mod.CONV_MATH == 'f16x3':
            out.amax = ops.amax_slots(dev)                # the next block's f16x3 GEMM reads it: published by the launch that writes the output
        return out

    def _exchange(self, i, xs, members, tape):
        src = lambda v: (v.data, None) if v.lazy is None else (v.lazy[0], v.lazy[1])
        operands = [(xs[i].data, None) if j == i else src(members[j]) for j in range(self.num_branches)]
        out = self._out_var(xs[i].data.device, tape)
        out.data = ops.hr_fuse([o[0] for o in operands], [o[1] for o in operands], out_hw=xs[i].data.shape[-2:], amax=out.amax)
        if tape is not None:
            xi, same, coarser = xs[i], [members[j] for j in range(i)], [members[j] for j in range(i + 1, self.num_branches)]

            def bwd_exchange():
                d_out = out.grad
                for y in coarser:
                    y._grad = torch.empty_like(src(y)[0])
                alias = HR_SHARE_GATED and xi.requires_grad and xi.grad_unwritten() and xi.pending is None
                # gated in place where x_i's gradient starts here: dL/dout's buffer becomes dL/dx_i
                gy = ops.hr_fuse_bwd(d_out, out.data, [y._grad for y in coarser], gy=d_out if alias else None)
                if alias:
                    xi._grad = gy
                elif xi.requires_grad:
                    buf, acc = xi.grad_target()
                    ops.copy_planes(gy, buf, accumulate=acc)
                for y in same:
                    y._grad = gy
                out.free_grad()
            tape.record(bwd_exchange, dict(op='hr_fuse', x=xi, members=[m for m in members if m is not None], out=out))
        return out

    def _exchange_composed(self, i, xs, members, tape):
        """the same sum from the existing ops, for grids the fused form does not take: every member written by its normalisation pass, a coarser
        one resized as the reference does (Upsample(scale_factor) to 2^(j-i) times its grid, then resize to the output grid), the adds in branch
        order; the last add and the ReLU are one normalisation pass with identity coefficients (relu(fma(t, 1, 0) + partial sum))"""
        B = self.num_branches
        hi, wi = xs[i].data.shape[-2:]
        dev = xs[i].data.device
        terms = []
        for j in range(B):
            tj = xs[i].data if j == i else members[j].data
            if j > i:
                r = 2 ** (j - i)
                up = (tj.shape[2] * r, tj.shape[3] * r)
                tj = ops.resize_bilinear(tj, up)
                if up != (hi, wi):
                    tj = ops.resize_bilinear(tj, (hi, wi))
            terms.append(tj)
        part = ops.copy_planes(terms[0], torch.empty_like(terms[0]))
        for tj in terms[1:-1]:
            ops.axpy_(part, tj)
        c = part.shape[1]
        one, zero = ops.const_tensor([1.0] * c, dev), ops.const_tensor([0.0] * c, dev)
        out = self._out_var(dev, tape)
        out.data = ops.bn_apply(terms[-1], zero, one, one, zero, True, residual=part, amax=out.amax)
        if tape is not None:
            xi = xs[i]

            def bwd_composed():
                gy = ops.hr_fuse_bwd(out.grad, out.data)                 # the gate pass alone
                if xi.requires_grad:
                    buf, acc = xi.grad_target()
                    ops.copy_planes(gy, buf, accumulate=acc)
                for j in range(B):
                    if j < i:
                        members[j]._grad = gy
                    elif j > i:
                        h, w = members[j].data.shape[-2:]
                        r = 2 ** (j - i)
                        g = gy if (h * r, w * r) == (hi, wi) else ops.resize_bilinear_bwd(gy, (h * r, w * r))
                        members[j]._grad = ops.resize_bilinear_bwd(g, (h, w))
                out.free_grad()
            tape.record(bwd_composed, dict(op='hr_fuse_composed', x=xi, members=[m for m in members if m is not None], out=out))
        return out


@BACKBONES.register_module()
class HRNet(nn.Module):
    """backbones/hrnet.py:217-643: stem (two 3x3 stride-2 conv -> BN -> ReLU), layer1, three transitions and three stages of HRModules; returns
    the tuple of branch outputs (strides 4, 8, 16, 32).  Module names are the reference's (conv1, bn1, conv2, bn2, layer1, transition{1,2,3},
    stage{2,3,4}.{m}.branches.{b}.{k} / .fuse_layers.{i}.{j}) so checkpoints load by key."""
    blocks_dict = {'BASIC': BasicBlock, 'BOTTLENECK': Bottleneck}

    def __init__(self, extra, in_channels=3, conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=False, with_cp=False,
                 frozen_stages=-1, zero_init_residual=False, multiscale_output=True, pretrained=None, init_cfg=None):
        super().__init__()
        _check_norm(norm_cfg)
        bad = [k for k, v in dict(norm_eval=norm_eval, with_cp=with_cp, frozen_stages=frozen_stages >= 0, conv_cfg=conv_cfg is not None).items() if v]
        if bad:
            raise NotImplementedError(f'HRNet options outside the implemented path: {bad}')
        if not (pretrained is None or isinstance(pretrained, str)):
            raise TypeError('pretrained must be a str or None')
        assert 'stage1' in extra and 'stage2' in extra and 'stage3' in extra and 'stage4' in extra
        for s in range(4):
            cfg = extra[f'stage{s + 1}']
            assert len(cfg['num_blocks']) == cfg['num_branches'] and len(cfg['num_channels']) == cfg['num_branches']
        self.extra, self.pretrained, self.zero_init_residual = extra, pretrained, zero_init_residual
        self.conv1 = Conv2dP(in_channels, 64, 3, 2, 1)
        self.bn1 = BatchNorm2dP(64)
        self.conv2 = Conv2dP(64, 64, 3, 2, 1)
        self.bn2 = BatchNorm2dP(64)
        cfg = extra['stage1']
        block = self.blocks_dict[cfg['block']]
        self.layer1 = _make_res_layer(block, 64, cfg['num_channels'][0], cfg['num_blocks'][0])
        pre = [cfg['num_channels'][0] * block.expansion]
        for s in (2, 3, 4):
            cfg = extra[f'stage{s}']
            block = self.blocks_dict[cfg['block']]
            cur = [c * block.expansion for c in cfg['num_channels']]
            setattr(self, f'transition{s - 1}', self._make_transition_layer(pre, cur))
            mods = [HRModule(cfg['num_branches'], block, cfg['num_blocks'], cur, cfg['num_channels'],
                             multiscale_output or s != 4 or m != cfg['num_modules'] - 1) for m in range(cfg['num_modules'])]
            setattr(self, f'stage{s}', nn.Sequential(*mods))
            pre = cur

    @staticmethod
    def _make_transition_layer(pre, cur):
        layers = []
        for i in range(len(cur)):
            if i < len(pre):
                layers.append(_conv_bn_seq(pre[i], cur[i], 3, 1, relu=True) if cur[i] != pre[i] else None)
            else:
                n = i + 1 - len(pre)
                layers.append(nn.Sequential(*[_conv_bn_seq(pre[-1], cur[i] if k == n - 1 else pre[-1], 3, 2, relu=True) for k in range(n)]))
        return nn.ModuleList(layers)

    def init_weights(self):
        """hrnet.py:313-329 with pretrained=None: Kaiming convolutions (done at construction), BatchNorm weight 1 / bias 0; zero_init_residual
        starts the last norm of every block at 0.  A local `pretrained` checkpoint is loaded instead; URLs fail loudly."""
        if self.pretrained is not None:
            _load_pretrained_backbone(self, self.pretrained)
            return
        for m in self.modules():
            if isinstance(m, BatchNorm2dP):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, BasicBlock):
                    nn.init.zeros_(m.bn2.weight)
                elif isinstance(m, Bottleneck):
                    nn.init.zeros_(m.bn3.weight)

    @staticmethod
    def _transit(layer, x, tape):
        if isinstance(layer[0], Conv2dP):
            return conv_bn_act(x, layer[0], layer[1], tape)
        for seq in layer:
            x = conv_bn_act(x, seq[0], seq[1], tape)
        return x

    def forward(self, x, tape=None, grad_ready=None):
        """grad_ready is accepted and unused: the backbone records no stage markers (the branches of a stage run side by side, no prefix of the
        tape completes a stage), so a data-parallel reducer sends the whole backbone with its final flush"""
        x = conv_bn_act(x, self.conv1, self.bn1, tape)
        x = conv_bn_act(x, self.conv2, self.bn2, tape)
        for blk in self.layer1:
            x = blk(x, tape)
        ys = [x]
        for s in (2, 3, 4):
            trans = getattr(self, f'transition{s - 1}')
            # hrnet.py:607-628: an entry that exists reads the LAST branch of the previous stage, a None entry passes branch i through
            xs = [ys[i] if layer is None else self._transit(layer, ys[-1], tape) for i, layer in enumerate(trans)]
            for mod in getattr(self, f'stage{s}'):
                xs = mod(xs, tape)
            ys = xs
        return tuple(ys)


def get_class_weight(class_weight):
    """losses/utils.py:10-25: a list is taken as is; a str is a file -- .npy via NumPy, otherwise what mmcv.load reads by
    extension (.json, .yaml / .yml, .pkl / .pickle)."""
    if not isinstance(class_weight, str):
        return class_weight
    import numpy as np
    ext = class_weight.rsplit('.', 1)[-1].lower()
    if ext == 'npy':
        return np.load(class_weight).tolist()
    if ext == 'json':
        import json
        with open(class_weight) as f:
            return json.load(f)
    if ext in ('yaml', 'yml'):
        import yaml
        with open(class_weight) as f:
            return yaml.safe_load(f)
    if ext in ('pkl', 'pickle'):
        import pickle
        with open(class_weight, 'rb') as f:
            return pickle.load(f)
    raise TypeError(f'Unsupported class_weight file format: {ext}')


@LOSSES.register_module()
class CrossEntropyLoss(nn.Module):
    """Softmax CE with pixel weights, optional class weights, ignore_index, mean over ALL pixels
    (avg_non_ignore=False), fused with the bilinear up-sampling of the logits and the accuracy.
    use_sigmoid=True: cross_entropy_loss.py:68-156 -- one-hot labels and binary_cross_entropy_with_logits per (pixel, class), class_weight as
    its pos_weight (the positive term only), mean over all N C H W elements; csrc/sigmoid_loss.hip, DESIGN.md section 8k."""

    def __init__(self, use_sigmoid=False, use_mask=False, reduction='mean', class_weight=None, loss_weight=1.0,
                 loss_name='loss_ce', avg_non_ignore=False):
        super().__init__()
        if use_mask or reduction != 'mean' or avg_non_ignore:
            raise NotImplementedError('pfst_amd CrossEntropyLoss: softmax or sigmoid CE, reduction=mean, avg_non_ignore=False, use_mask=False only')
        self.use_sigmoid = bool(use_sigmoid)
        self.class_weight = get_class_weight(class_weight)
        self.loss_weight = loss_weight
        self._loss_name = loss_name
        self._cw = None
        self._coef = None

    @property
    def loss_name(self):
        return self._loss_name

    def _cw_dev(self, dev):
        if self.class_weight is None:
            return None
        if self._cw is None or self._cw.device != dev:
            self._cw = torch.tensor(self.class_weight, dtype=torch.float32, device=dev)
        return self._cw

    def sigmoid_coef(self, num_classes):
        """the (k_pos, k_neg) rows of the sigmoid form: pos_weight on the positive term, 1 on the negative"""
        if num_classes < 2:
            raise NotImplementedError('CrossEntropyLoss(use_sigmoid=True): one-channel (binary) logits are not built, num_classes >= 2 only')
        cw = self.class_weight if self.class_weight is not None else [1.0] * num_classes
        if len(cw) != num_classes:
            raise ValueError(f'CrossEntropyLoss(use_sigmoid=True): class_weight has {len(cw)} entries for {num_classes} classes')
        return [[float(v), 1.0] for v in cw]

    def fused(self, logits, label_u8, weight, tape, ignore_index=255, grad_scale=1.0, share=None):
        """logits: Var [N,C,h,w] (low res); label_u8 [N,1,H,W] or [N,H,W]; weight [N,H,W] or None.
        share: a dict the terms of one head's loss list pass along -- the log-sum-exp map is left in it for a DiceLoss that follows.
        -> device tensor [loss, acc_seg, #bad labels]"""
        if self.use_sigmoid:
            return _sigmoid_fused(self, 'bce', self.sigmoid_coef(logits.data.shape[1]), 0.0, 'mean', logits, label_u8, weight, tape,
                                  ignore_index, grad_scale)
        ld = logits.data
        n = ld.shape[0]
        H, W = label_u8.shape[-2:]
        cw = self._cw_dev(ld.device)
        lse, acc = ops.ce_upsample_fwd(ld, label_u8, weight, cw, ignore_index)
        if share is not None:
            share['lse'] = lse
        out = ops.ce_finalize(acc, n * H * W, self.loss_weight)
        if tape is not None:
            scale = grad_scale * self.loss_weight / float(n * H * W)

            def bwd():
                buf, accf = logits.grad_target()
                ops.ce_upsample_bwd(ld, label_u8, lse, scale, weight, cw, ignore_index, out=buf, accumulate=accf)
            tape.record(bwd, dict(op='ce', x=logits, out=None, label=label_u8, weight=weight, class_weight=self.class_weight,
                                  loss_weight=grad_scale * self.loss_weight, ignore_index=ignore_index))
        return out


def _sigmoid_fused(term, op, coef_rows, gamma, reduction, logits, label_u8, weight, tape, ignore_index, grad_scale):
    """the shared body of the sigmoid terms (FocalLoss, CrossEntropyLoss(use_sigmoid)): forward partials, the ordered sum, the tape record.
    Neither reads or writes share['lse'].  The divisor is known on the host: N C H W for 'mean' and for 'none' (the reference returns the
    [N,C,H,W] map there and _parse_losses takes its mean), 1 for 'sum'."""
    ld = logits.data
    n, c = ld.shape[:2]
    H, W = label_u8.shape[-2:]
    if term._coef is None or term._coef.device != ld.device or term._coef.shape[0] != c:
        term._coef = torch.tensor(coef_rows, dtype=torch.float32, device=ld.device)
    coef = term._coef
    divisor = 1.0 if reduction == 'sum' else float(n * c * H * W)
    slab, counts, _ = ops.sigloss_upsample_fwd(ld, label_u8, coef, gamma, weight, ignore_index)
    out, _ = ops.sigloss_finalize(slab, counts, divisor, term.loss_weight)
    if tape is not None:
        scale = grad_scale * term.loss_weight / divisor

        def bwd():
            buf, accf = logits.grad_target()
            ops.sigloss_upsample_bwd(ld, label_u8, coef, scale, gamma, weight, ignore_index, out=buf, accumulate=accf)
        tape.record(bwd, dict(op=op, x=logits, out=None, label=label_u8, weight=weight, coef=coef_rows, gamma=gamma, reduction=reduction,
                              loss_weight=grad_scale * term.loss_weight, ignore_index=ignore_index))
    return out


@LOSSES.register_module()
class FocalLoss(nn.Module):
    """losses/focal_loss.py (its py_sigmoid_focal_loss branch) fused with the bilinear up-sampling of the logits (csrc/sigmoid_loss.hip; the
    closed form: DESIGN.md section 8k): per (pixel, class) alpha_t (1 - p_t)^gamma BCE(x, t), times the class weight, the pixel weight and
    the validity of the label under the HEAD's ignore_index; no softmax across classes.  alpha: a float, or a list of C floats indexing the
    class axis."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.5, reduction='mean', class_weight=None, loss_weight=1.0, loss_name='loss_focal'):
        super().__init__()
        if use_sigmoid is not True:
            raise NotImplementedError('FocalLoss: only sigmoid focal loss is supported (use_sigmoid=True), as in the reference')
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"FocalLoss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not float(gamma) >= 0.0:
            raise ValueError(f'FocalLoss: gamma must be a number >= 0, got {gamma!r}')
        alphas = list(alpha) if isinstance(alpha, (list, tuple)) else [alpha]
        if not alphas or any(isinstance(a, bool) or not isinstance(a, (int, float)) or not 0.0 <= float(a) <= 1.0 for a in alphas):
            raise ValueError(f'FocalLoss: alpha (a float or a list of floats) must lie in [0, 1], got {alpha!r}')
        if class_weight is not None and not isinstance(class_weight, (list, tuple)):
            raise TypeError('FocalLoss: class_weight must be None or a list')
        self.use_sigmoid, self.gamma, self.reduction = use_sigmoid, gamma, reduction
        self.alpha = list(alpha) if isinstance(alpha, (list, tuple)) else alpha
        self.class_weight = None if class_weight is None else list(class_weight)
        self.loss_weight = loss_weight
        self._loss_name = loss_name
        self._coef = None

    loss_name = CrossEntropyLoss.loss_name

    def coef_rows(self, num_classes):
        """(k_pos, k_neg) = class_weight_c * (alpha_c, 1 - alpha_c) per class"""
        c = num_classes
        if c < 2:
            raise NotImplementedError('FocalLoss: one-channel (binary) logits are not built, num_classes >= 2 only')
        alpha = self.alpha if isinstance(self.alpha, list) else [self.alpha] * c
        if len(alpha) != c:
            raise ValueError(f'FocalLoss: alpha has {len(alpha)} entries for {c} classes')
        cw = self.class_weight if self.class_weight is not None else [1.0] * c
        if len(cw) != c:
            raise ValueError(f'FocalLoss: class_weight has {len(cw)} entries for {c} classes')
        return [[float(w) * float(a), float(w) * (1.0 - float(a))] for w, a in zip(cw, alpha)]

    def fused(self, logits, label_u8, weight, tape, ignore_index=255, grad_scale=1.0, share=None):
        """the interface of CrossEntropyLoss.fused -> device tensor [loss, acc_seg, #bad labels]"""
        return _sigmoid_fused(self, 'focal', self.coef_rows(logits.data.shape[1]), float(self.gamma), self.reduction, logits, label_u8, weight,
                              tape, ignore_index, grad_scale)


@LOSSES.register_module()
class DiceLoss(nn.Module):
    """losses/dice_loss.py fused with the bilinear up-sampling of the logits (csrc/dice_loss.hip; the closed form: DESIGN.md section 8h).
    The reference's quirks are kept: the head's `weight=` and `ignore_index=` are swallowed (a Dice term sees neither the pixel weights
    nor the head's ignore_index, only its OWN), an ignored label is clamped to class C - 1 and counted in the denominator, a class index
    equal to ignore_index is skipped while the divisor stays C, and `reduction` has no effect (dice_loss reduces a scalar).
    exponent >= 1 only: p^(e-1) at p -> 0 is not finite below."""

    def __init__(self, smooth=1, exponent=2, reduction='mean', class_weight=None, loss_weight=1.0, ignore_index=255,
                 loss_name='loss_dice', **kwards):
        super().__init__()
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"DiceLoss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        if not float(exponent) >= 1.0:
            raise ValueError(f'DiceLoss: exponent must be >= 1, got {exponent!r}')
        self.smooth, self.exponent, self.reduction = smooth, exponent, reduction
        self.class_weight = get_class_weight(class_weight)
        self.loss_weight = loss_weight
        self.ignore_index = 255 if ignore_index is None else ignore_index      # no label is None: uint8 label maps, 255 = "no class index"
        self._loss_name = loss_name
        self._cw = None

    loss_name = CrossEntropyLoss.loss_name
    _cw_dev = CrossEntropyLoss._cw_dev

    def fused(self, logits, label_u8, weight, tape, ignore_index=255, grad_scale=1.0, share=None):
        """the interface of CrossEntropyLoss.fused; `weight` is ignored and `ignore_index` (the head's) only selects the pixels of acc_seg.
        -> device tensor [loss, acc_seg, #bad labels]"""
        ld = logits.data
        if self.class_weight is not None and len(self.class_weight) != ld.shape[1]:
            raise ValueError(f'DiceLoss: class_weight has {len(self.class_weight)} entries for {ld.shape[1]} classes')
        cw = self._cw_dev(ld.device)
        ign, e = self.ignore_index, float(self.exponent)
        slab, counts, lse, _ = ops.dice_upsample_fwd(ld, label_u8, ign, ignore_index, e, lse=None if share is None else share.get('lse'))
        if share is not None:
            share['lse'] = lse
        out, coef, _ = ops.dice_finalize(slab, counts, cw, ign, self.smooth, e, self.loss_weight)
        if tape is not None:
            scale = grad_scale * self.loss_weight

            def bwd():
                buf, accf = logits.grad_target()
                ops.dice_upsample_bwd(ld, label_u8, lse, coef, scale, ign, e, out=buf, accumulate=accf)
            tape.record(bwd, dict(op='dice', x=logits, out=None, label=label_u8, class_weight=self.class_weight, loss_weight=scale,
                                  ignore_index=ign, smooth=self.smooth, exponent=self.exponent))
        return out


class LossConfigError(ValueError, KeyError):
    """a loss config whose keys contradict each other.  A ValueError like every refused option; also a KeyError, what a config that names
    `type='LovaszLoss'` without `reduction='none'` has always failed with at build time (the registry's, before the term was built):
    callers and tests that catch either keep working."""

    __str__ = ValueError.__str__          # (KeyError's would quote the message)


@LOSSES.register_module()
class LovaszLoss(nn.Module):
    """losses/lovasz_loss.py (the multi-class Lovasz-Softmax form) fused with the bilinear up-sampling of the logits (csrc/lovasz_loss.hip;
    the algorithm: DESIGN.md section 8m).  Per class c of the class set, over the pixels whose label differs from the HEAD's ignore_index:
    errors |fg - p_c|, their descending order, lovasz_grad of the sorted foreground flags, the dot product, times class_weight[c]; the mean over
    the classes kept ('present': those with foreground among the valid pixels, 'all', or a list of class indices).  per_image: one value per
    image, then `reduction` ('none' is logged as the mean of the N values, as _parse_losses takes it).  As executed by the reference the
    head's `weight=` is swallowed (pixel weights have no effect) and a label outside [0, C) other than ignore_index is a valid pixel that is
    foreground for no class (it is counted in #bad labels like everywhere).
    Deviations: loss_type='binary' (the one-channel hinge) is not built; where no pixel is valid -- the batch, one image under per_image (it adds
    0 and still counts in the divisor N), or 'present' with no class present -- the loss is 0 with a zero gradient (the reference returns an empty
    tensor or raises); equal errors are ordered by ascending pixel index (n, y, x) where the reference's unstable sort leaves their gradient
    arbitrary (the loss value does not depend on it); a list of classes must hold distinct indices in [0, C)."""

    def __init__(self, loss_type='multi_class', classes='present', per_image=False, reduction='mean', class_weight=None, loss_weight=1.0,
                 loss_name='loss_lovasz'):
        super().__init__()
        if loss_type not in ('binary', 'multi_class'):
            raise ValueError("LovaszLoss: loss_type should be 'binary' or 'multi_class'")
        if loss_type == 'binary':
            raise NotImplementedError('LovaszLoss: the binary (one-channel hinge) form is not built, multi_class only')
        if not (classes in ('all', 'present') or (isinstance(classes, (list, tuple)) and len(classes) > 0
                                                  and all(isinstance(c, int) and not isinstance(c, bool) for c in classes))):
            raise ValueError(f"LovaszLoss: classes must be 'all', 'present' or a list of ints, got {classes!r}")
        if reduction not in ('none', 'mean', 'sum'):
            raise ValueError(f"LovaszLoss: reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        if not per_image and reduction != 'none':
            raise LossConfigError("LovaszLoss: reduction should be 'none' when per_image is False")  # lovasz_loss.py:269-271 asserts
        self.classes = classes if isinstance(classes, str) else list(classes)
        self.per_image, self.reduction = bool(per_image), reduction
        self.class_weight = get_class_weight(class_weight)
        self.loss_weight = loss_weight
        self._loss_name = loss_name
        self._tables = None

    loss_name = CrossEntropyLoss.loss_name

    def _class_tables(self, num_classes, dev):
        """(slot, cls, class weights by slot | None) on the device, built at first use"""
        if self._tables is None or self._tables[0].device != dev or self._tables[0].numel() != num_classes:
            if self.class_weight is not None and len(self.class_weight) != num_classes:
                raise ValueError(f'LovaszLoss: class_weight has {len(self.class_weight)} entries for {num_classes} classes')
            slot, cls = ops.lovasz_class_tables(self.classes, num_classes, dev)
            cw = None
            if self.class_weight is not None:
                order = range(num_classes) if isinstance(self.classes, str) else self.classes
                cw = torch.tensor([float(self.class_weight[c]) for c in order], dtype=torch.float32, device=dev)
            self._tables = (slot, cls, cw)
        return self._tables

    def fused(self, logits, label_u8, weight, tape, ignore_index=255, grad_scale=1.0, share=None):
        """the interface of CrossEntropyLoss.fused; `weight` is ignored, `ignore_index` (the head's) selects the valid pixels.
        -> device tensor [loss, acc_seg, #bad labels]"""
        ld = logits.data
        slot, cls, cw = self._class_tables(ld.shape[1], ld.device)
        ign = 255 if ignore_index is None else ignore_index            # uint8 label maps: 255 = "no class index"
        r = ops.lovasz_upsample_fwd(ld, label_u8, slot, cls, cw, ign, self.per_image, self.classes == 'present',
                                    'sum' if self.reduction == 'sum' else 'mean', self.loss_weight,
                                    lse=None if share is None else share.get('lse'))
        if share is not None:
            share['lse'] = r['lse']
        if tape is not None:
            scale = grad_scale * self.loss_weight
            lse, cmap, blk = r['lse'], r['map'], r['scale']           # blk: the kept-class / per-image divisors, on the device

            def bwd():
                buf, accf = logits.grad_target()
                ops.lovasz_upsample_bwd(ld, label_u8, slot, cls, lse, cmap, blk, scale, ign, out=buf, accumulate=accf)
            tape.record(bwd, dict(op='lovasz', x=logits, out=None, label=label_u8, class_weight=self.class_weight, loss_weight=scale,
                                  ignore_index=ign, classes=self.classes, per_image=self.per_image, reduction=self.reduction))
        return r['out']


@PIXEL_SAMPLERS.register_module()
class OHEMPixelSampler:
    """core/seg/sampler/ohem_pixel_sampler.py on the device (csrc/ohem.hip): the 0 / 1 map of the hard pixels, from the
    LOW-resolution logits -- the resize is fused, the reference's full-resolution softmax and global sort are an exact radix select whose
    digits are chosen on the device, and the host reads nothing.  With `thresh` a valid pixel is kept where the softmax probability of its
    label lies below max(s[k], fp32(thresh)), s the ascending sort of those probabilities, k = min(min_kept * N, n_valid - 1); without, the
    min(min_kept * N, n_valid) valid pixels of largest unreduced loss are kept (ties at the cut: in raster order, the same from run to run).
    A label outside [0, C) other than the head's ignore_index is not valid here (the head still reports it after the step).
    context: the decode head (its ignore_index and loss terms); the terms must be CrossEntropyLoss -- a term that ignores pixel weights has no
    use for the map and no per-pixel loss to rank by."""

    def __init__(self, context, thresh=None, min_kept=100000):
        assert min_kept > 1
        self.context = context
        self.thresh = None if thresh is None else float(thresh)
        self.min_kept = int(min_kept)
        self.last_info = None          # device int64 [4] of the last call: (threshold / cut bits, n_valid, n_kept, k); never read in the step
        self._coef = None
        terms = context.loss_decode if isinstance(context.loss_decode, nn.ModuleList) else [context.loss_decode]
        coef = [0.0] * context.num_classes
        for term in terms:
            if not isinstance(term, CrossEntropyLoss):
                raise NotImplementedError(f'OHEMPixelSampler: the loss term {type(term).__name__} ({term.loss_name}) takes no pixel weights and '
                                          'has no per-pixel loss; a sampled head needs CrossEntropyLoss terms only')
            if term.use_sigmoid and self.thresh is None:
                # the reference ranks the term's unreduced loss there, which is an [N,C,H,W] map for the sigmoid form, and fails
                raise NotImplementedError(f'OHEMPixelSampler: without thresh the pixels are ranked by the unreduced loss, which {term.loss_name} '
                                          '(use_sigmoid=True) has per (pixel, class) only; give thresh')
            cw = term.class_weight if term.class_weight is not None else [1.0] * context.num_classes
            if len(cw) != context.num_classes:
                raise ValueError(f'OHEMPixelSampler: {term.loss_name} has {len(cw)} class weights for {context.num_classes} classes')
            if not term.loss_weight >= 0 or not all(float(v) >= 0 for v in cw):
                raise ValueError(f'OHEMPixelSampler: {term.loss_name} has a negative loss_weight or class weight; the per-pixel loss must be >= 0')
            coef = [a + float(term.loss_weight) * float(v) for a, v in zip(coef, cw)]
        self.coef = coef               # per class: sum over the terms of loss_weight * class_weight (cross_entropy_loss.py:45-50, 273)

    def _coef_dev(self, dev):
        if self._coef is None or self._coef.device != dev:
            self._coef = torch.tensor(self.coef, dtype=torch.float32, device=dev)
        return self._coef

    def sample(self, seg_logit, seg_label_u8):
        """seg_logit: the low-resolution logits [N, C, h, w] (tensor or Var); seg_label_u8 [N, 1, H, W] or [N, H, W] -> weight [N, H, W]"""
        ld = seg_logit.data if isinstance(seg_logit, Var) else seg_logit
        coef = self._coef_dev(ld.device) if self.thresh is None else None
        weight, self.last_info = ops.ohem_sample(ld, seg_label_u8, self.context.ignore_index, self.thresh, self.min_kept * ld.shape[0], coef)
        return weight


class BaseDecodeHead(nn.Module):
    def __init__(self, in_channels, channels, *, num_classes, dropout_ratio=0.1, conv_cfg=None, norm_cfg=None,
                 act_cfg=dict(type='ReLU'), in_index=-1, input_transform=None,
                 loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0), ignore_index=255,
                 sampler=None, align_corners=False, init_cfg=None):
        super().__init__()
        _check_norm(norm_cfg)
        if (input_transform is not None and not self._takes_input_transform(in_channels, in_index, input_transform)) or align_corners \
                or conv_cfg is not None:
            raise NotImplementedError('decode head options outside the PFST path')
        self.input_transform = input_transform
        if not isinstance(loss_decode, (dict, list, tuple)):
            raise TypeError(f'loss_decode must be a dict or a sequence of dicts, but got {type(loss_decode)}')
        self.in_channels, self.channels, self.num_classes = in_channels, channels, num_classes
        self.dropout_ratio, self.in_index, self.ignore_index = dropout_ratio, in_index, ignore_index
        self.align_corners = align_corners
        # decode_head.py:84-92: one loss module, or a ModuleList of them in the order given
        self.loss_decode = build_loss(loss_decode) if isinstance(loss_decode, dict) else nn.ModuleList([build_loss(l) for l in loss_decode])
        for term in (self.loss_decode if isinstance(self.loss_decode, nn.ModuleList) else [self.loss_decode]):
            if not hasattr(term, 'fused'):
                raise NotImplementedError(f'{type(term).__name__} has no fused up-sampling form: it cannot be a loss_decode term')
        # decode_head.py:93-96.  A plain attribute: the sampler is no module and holds the head as its context
        self.sampler = build_pixel_sampler(sampler, context=self) if sampler is not None else None
        self.conv_seg = Conv2dP(channels, num_classes, 1, bias=True)
        nn.init.normal_(self.conv_seg.weight, 0, 0.01)
        self.dropout_enabled = True            # the teacher switches this off (pfgst.py:247-251)
        self.injected_dropout_mask = None      # parity tests inject the (n, C) keep/scale mask

    @staticmethod
    def _takes_input_transform(in_channels, in_index, input_transform):
        """does this head class implement `input_transform` for these arguments?  (FCNHead: 'resize_concat' over lists; nobody else)"""
        return False

    def dropout_mask(self, n, training):
        """the (n, C) keep / (1 - p) factors of nn.Dropout2d (decode_head.py:103-107), or None when dropout is off (evaluation, the
        teacher, p = 0); the parity tests inject theirs.  Drawn by the head right before its last conv -> BN -> ReLU layer, which
        applies it in its normalisation pass (layers.conv_bn_act(post_scale=...)): the torch generator sees the same draws in the
        same order as when the mask was drawn after that layer (nothing in between draws from it)"""
        p = self.dropout_ratio
        if self.injected_dropout_mask is not None:
            return self.injected_dropout_mask
        if training and self.dropout_enabled and p > 0:
            dev = self.conv_seg.weight.device
            return (torch.rand(n, self.channels, device=dev) >= p).float() / (1.0 - p)
        return None

    def cls_seg(self, feat, tape, training, dropped=False):
        """dropout + conv_seg (decode_head.py:242-247).  dropped: `feat` already carries the Dropout2d factors (folded into the layer that
        produced it); otherwise they are applied here as a pass of their own"""
        mask = None if dropped else self.dropout_mask(feat.data.shape[0], training)
        if mask is not None:
            src = feat
            y = ops.channel_scale(src.data, mask)
            feat = Var(y, tape is not None)
            if tape is not None:
                dropped_v = feat

                def bwd():
                    src._grad = ops.channel_scale(dropped_v.grad, mask)
                    dropped_v.free_grad()
                tape.record(bwd, dict(op='channel_scale', x=src, out=dropped_v, mask=mask))
        return conv_forward(feat, self.conv_seg, tape)

    def losses(self, seg_logit, seg_label_u8, seg_weight, tape, grad_scale=1.0):
        # '_bad_labels': labels outside [0, C) other than ignore_index (F.cross_entropy raises on them); travels with the packed
        # scalars of the step and is checked on the host after the step's single read (uda.PFGST.forward_train), never logged
        if self.sampler is not None:
            # decode_head.py:258-259: the sampler's map REPLACES the weights the caller passed (PFGST's pseudo-label confidence included)
            seg_weight = self.sampler.sample(seg_logit, seg_label_u8)
        if not isinstance(self.loss_decode, nn.ModuleList):
            out = self.loss_decode.fused(seg_logit, seg_label_u8, seg_weight, tape, self.ignore_index, grad_scale)
            return {self.loss_decode.loss_name: out[0:1], 'acc_seg': out[1:2], '_bad_labels': out[2:3]}
        # decode_head.py:263-283: the terms in order, terms of one loss_name added; acc_seg once per head -- every term counts it from the
        # same logits and labels under the head's ignore_index (the first one's is kept), every term's bad-label count is added
        loss, share, first, bad = dict(), dict(), None, None
        for term in self.loss_decode:
            out = term.fused(seg_logit, seg_label_u8, seg_weight, tape, self.ignore_index, grad_scale, share=share)
            name = term.loss_name
            loss[name] = out[0:1] if name not in loss else loss[name] + out[0:1]
            first = out if first is None else first
            bad = out[2:3] if bad is None else bad + out[2:3]
        loss['acc_seg'] = first[1:2]
        loss['_bad_labels'] = bad
        return loss

    def forward_train(self, inputs, img_metas, gt_semantic_seg, train_cfg, seg_weight=None, tape=None, grad_scale=1.0):
        seg_logits, feats = self.forward(inputs, return_features=True, tape=tape, training=True)
        losses = self.losses(seg_logits, gt_semantic_seg, seg_weight, tape, grad_scale)
        return losses, {'seg_logits': seg_logits, 'decoded_features': feats}

    def forward_test(self, inputs, img_metas, test_cfg, tape=None):
        seg_logits, feats = self.forward(inputs, return_features=True, tape=None, training=False)
        return seg_logits, {'decoded_features': feats}


@HEADS.register_module()
class DepthwiseSeparableASPPHead(BaseDecodeHead):
    def __init__(self, c1_in_channels, c1_channels, dilations=(1, 6, 12, 18), **kwargs):
        super().__init__(**kwargs)
        assert c1_in_channels > 0 and dilations[0] == 1 and all(d > 1 for d in dilations[1:])
        self.dilations = tuple(dilations)
        ci, ch = self.in_channels, self.channels
        self.image_pool = nn.Sequential(nn.Identity(), ConvModule(ci, ch, 1))
        mods = [ConvModule(ci, ch, 1)]
        mods += [DepthwiseSeparableConvModule(ci, ch, 3, padding=d, dilation=d) for d in dilations[1:]]
        self.aspp_modules = nn.ModuleList(mods)
        self.bottleneck = ConvModule((len(dilations) + 1) * ch, ch, 3, padding=1)
        self.c1_bottleneck = ConvModule(c1_in_channels, c1_channels, 1)
        self.c1_channels = c1_channels
        self.sep_bottleneck = nn.Sequential(DepthwiseSeparableConvModule(ch + c1_channels, ch, 3, padding=1),
                                            DepthwiseSeparableConvModule(ch, ch, 3, padding=1))

    def forward(self, inputs, return_features=False, tape=None, training=True):
        c1, x = inputs[0], inputs[self.in_index]
        n, _, h, w = x.data.shape
        ch, nb = self.channels, len(self.dilations) + 1
        cat = Var(torch.empty(n, nb * ch, h, w, device=x.data.device), tape is not None)
        if layers_mod.CONV_MATH == 'f16x3':
            # every writer of the concat publishes max |.| into ONE group (layers._amax_target for the four slices, the broadcast below): the
            # bottleneck's f16x3 scale needs no pass of its own over the 2560-channel buffer
            cat.amax = ops.amax_slots(x.data.device)
        # The ASPP branches first, the image-pool branch after them (they write disjoint slices, so the forward result does not
        # depend on the order): in backward the pool branch's broadcast then lands in dL/dx BEFORE the 1x1 branch's data gradient,
        # which completes dL/dx and can emit the BatchNorm-backward sums of the layer that produced x (layers._dgrad_into).
        # layers.FOLD_BN_CONCAT: the four conv -> BN -> ReLU writers leave their pre-normalisation outputs in the slices; the bottleneck's Winograd
        # input transform normalises per channel (the image-pool slice holds final values: identity rows) -- four normalisation passes over
        # 512-channel maps less per pass
        sl = layers_mod.folds_into_concat(self.bottleneck.conv, h, w, tape is not None)
        if sl:
            cat.coef_table = torch.empty(nb * ch, 4, device=x.data.device)
            cat.coef_table[:ch] = layers_mod.identity_coef_row(x.data.device)          # y = max(fma(v, 1, 0), 0) = v for the (non-negative) pooled values
        self.aspp_modules[0](x, tape, out=cat.slice(ch, 2 * ch), defer=sl)
        nd = len(self.dilations)
        # on the fused path the atrous branches' launch also forms the plane means of x, its backward their adjoint
        pool = {}
        dwsep_branches(x, [self.aspp_modules[i] for i in range(1, nd)], tape, [cat.slice((i + 1) * ch, (i + 2) * ch) for i in range(1, nd)],
                       pool=pool, defer=sl)
        # image pool branch: GAP -> 1x1 conv -> BN over the n samples -> ReLU -> broadcast (bilinear from 1x1)
        fused_pool = pool is not None and 'mean' in pool
        pooled = Var(pool['mean'] if fused_pool else ops.global_avgpool(x.data), tape is not None)
        pa = self.image_pool[1](pooled, tape)
        ops.broadcast_hw(pa.data, cat.data[:, 0:ch], amax=cat.amax)
        if tape is not None:
            hw = float(h * w)

            def bwd_pool():
                g = cat.grad
                pa._grad = ops.reduce_hw(g[:, 0:ch])

            def bwd_gap():
                if fused_pool:                     # handed to the atrous branches' fused backward, which runs later and writes dL/dx once
                    pool['grad'] = pooled.grad
                    pooled.free_grad()
                    return
                buf, acc = x.grad_target()
                if not acc:
                    ops.fill_(buf, 0.0)
                ops.broadcast_hw(pooled.grad, buf, 1.0 / hw, True)
                pooled.free_grad()
            # order on the tape: gap-backward must run AFTER the image_pool conv's backward, pool-broadcast before it
            self._reorder_pool(tape, (bwd_gap, dict(op='gap', name='decode_head.gap', x=x, out=pooled)),
                               (bwd_pool, dict(op='broadcast', name='decode_head.image_pool.up', x=pa, out=cat.slice(0, ch))))
        if sl:
            # every writer deferred?  (a writer that could not -- no (min, max) partials for its shape -- wrote its slice normalised: identity rows)
            cat.lazy = (cat.data, cat.coef_table, None)
        feats = self.bottleneck(cat, tape)
        # decoder: upsample x2 to c1 size, concat with the 48-channel c1 projection
        H, W = c1.data.shape[-2:]
        cat2 = Var(torch.empty(n, ch + self.c1_channels, H, W, device=x.data.device), tape is not None)
        ops.resize_bilinear(feats.data, (H, W), out=cat2.data[:, 0:ch])
        if tape is not None:
            def bwd_up():
                buf, acc = feats.grad_target()
                ops.resize_bilinear_bwd(cat2.grad[:, 0:ch], (h, w), out=buf, accumulate=acc)
            tape.record(bwd_up, dict(op='resize', name='decode_head.up', x=feats, out=cat2.slice(0, ch)))
        self.c1_bottleneck(c1, tape, out=cat2.slice(ch, ch + self.c1_channels))
        o = self.sep_bottleneck[0](cat2, tape, defer=True)          # its only consumer, sep_bottleneck[1]'s depthwise layer, normalises on load
        fold = FOLD_DROPOUT
        mask = self.dropout_mask(n, training) if fold else None
        o = self.sep_bottleneck[1](o, tape, post_scale=mask)          # Dropout2d folded into this layer's normalisation pass
        logits = self.cls_seg(o, tape, training, dropped=fold)
        return (logits, feats) if return_features else logits

    @staticmethod
    def _reorder_pool(tape, bwd_gap, bwd_pool):
        # forward recorded: [..., image_pool ConvModule closure]; we need tape order
        # [bwd_gap, conv closure, bwd_pool] so that reverse execution is pool -> conv -> gap.
        conv_closure = tape.pop()
        tape.record(*bwd_gap)
        tape.record(*conv_closure)
        tape.record(*bwd_pool)


def _concat_var(x, channels, tape):
    """an empty [N, channels, H, W] concat buffer over x's grid; under f16x3 with the slot group every writer of it publishes max |.| into"""
    n, _, h, w = x.data.shape
    cat = Var(torch.empty(n, channels, h, w, device=x.data.device), tape is not None)
    if layers_mod.CONV_MATH == 'f16x3':
        cat.amax = ops.amax_slots(x.data.device)
    return cat


def _identity_into(x, cat, c0, tape):
    """x copied into channels [c0, c0 + C) of the concat `cat` (the reference's torch.cat([x, ...])); backward adds that slice of the
    concat's gradient to dL/dx.  Recorded AFTER the layers that read x, so that in backward it runs before their data gradients and the
    first of them still completes dL/dx"""
    c1 = c0 + x.data.shape[1]
    ops.copy_planes(x.data, cat.data[:, c0:c1], amax=cat.amax)
    if tape is not None and x.requires_grad:
        def bwd():
            buf, acc = x.grad_target()
            ops.copy_planes(cat.grad[:, c0:c1], buf, accumulate=acc)
        tape.record(bwd)


@HEADS.register_module()
class ASPPHead(BaseDecodeHead):
    """aspp_head.py (DeepLabV3): the image-pool branch and dense atrous branches -> concat -> 3x3 bottleneck -> cls_seg.  The concat, its shared
    maximum and the deferred normalisation of its writers are those of DepthwiseSeparableASPPHead (a dense 3x3 branch on the Winograd path
    writes its slice normalised: layers.norm_plan)"""

    def __init__(self, dilations=(1, 6, 12, 18), **kwargs):
        super().__init__(**kwargs)
        assert isinstance(dilations, (list, tuple)) and all(isinstance(d, int) and d >= 1 for d in dilations)
        self.dilations = tuple(dilations)
        ci, ch = self.in_channels, self.channels
        self.image_pool = nn.Sequential(nn.Identity(), ConvModule(ci, ch, 1))
        self.aspp_modules = nn.ModuleList([ConvModule(ci, ch, 1 if d == 1 else 3, padding=0 if d == 1 else d, dilation=d) for d in dilations])
        self.bottleneck = ConvModule((len(dilations) + 1) * ch, ch, 3, padding=1)

    def forward(self, inputs, return_features=False, tape=None, training=True):
        x = inputs[self.in_index]
        n, _, h, w = x.data.shape
        ch, nb = self.channels, len(self.dilations) + 1
        cat = _concat_var(x, nb * ch, tape)
        sl = layers_mod.folds_into_concat(self.bottleneck.conv, h, w, tape is not None)
        if sl:
            cat.coef_table = torch.empty(nb * ch, 4, device=x.data.device)
            cat.coef_table[:ch] = layers_mod.identity_coef_row(x.data.device)
        # the branches first, the image pool after them: in backward the pool's broadcast lands in dL/dx before the first branch's data
        # gradient, which completes it (the order of DepthwiseSeparableASPPHead)
        for i, m in enumerate(self.aspp_modules):
            m(x, tape, out=cat.slice((i + 1) * ch, (i + 2) * ch), defer=sl)
        pooled = Var(ops.global_avgpool(x.data), tape is not None)
        pa = self.image_pool[1](pooled, tape)
        ops.broadcast_hw(pa.data, cat.data[:, 0:ch], amax=cat.amax)
        if tape is not None:
            hw = float(h * w)

            def bwd_pool():
                pa._grad = ops.reduce_hw(cat.grad[:, 0:ch])

            def bwd_gap():
                buf, acc = x.grad_target()
                if not acc:
                    ops.fill_(buf, 0.0)
                ops.broadcast_hw(pooled.grad, buf, 1.0 / hw, True)
                pooled.free_grad()
            DepthwiseSeparableASPPHead._reorder_pool(tape, (bwd_gap, dict(op='gap', name='decode_head.gap', x=x, out=pooled)),
                                                     (bwd_pool, dict(op='broadcast', name='decode_head.image_pool.up', x=pa, out=cat.slice(0, ch))))
        if sl:
            cat.lazy = (cat.data, cat.coef_table, None)
        feats = self.bottleneck(cat, tape)
        # (the returned features are the PRE-dropout input of cls_seg, aspp_head.py:118-126: Dropout2d stays a pass of its own)
        logits = self.cls_seg(feats, tape, training)
        return (logits, feats) if return_features else logits


def _ppm_forward(x, ci, ch, scales, psp_modules, bottleneck, tape):
    """the pyramid pooling module and its 3x3 bottleneck over x [N, ci, H, W] (psp_head.py:9-50, :86-93; uper_head.py:77-85) -> the bottleneck's
    output Var.  Shared by PSPHead and UPerHead: [x, resize(ConvModule(AdaptiveAvgPool2d(s)(x))) for s in scales] in one concat buffer"""
    cat = _concat_var(x, ci + len(scales) * ch, tape)
    x.claim_first_use()              # dL/dx is completed by the pyramid's adjoint below, which fuses nothing
    ops.copy_planes(x.data, cat.data[:, 0:ci], amax=cat.amax)
    pooled = [Var(p, tape is not None) for p in ops.pyramid_pool(x.data, scales)]
    if tape is not None:
        # recorded before the small layers, so it runs after them: dL/dx = the identity slice's gradient + the adjoint of every pooling,
        # written once
        def bwd_pool():
            buf, acc = x.grad_target()
            ops.pyramid_pool_bwd([p.grad for p in pooled], scales, buf, accumulate=acc, add=cat.grad[:, 0:ci])
            for p in pooled:
                p.free_grad()
        tape.record(bwd_pool)
    outs = [psp_modules[k][1](pooled[k], tape) for k in range(len(scales))]
    ops.pyramid_upsample([o.data for o in outs], scales, cat.data[:, ci:], amax=cat.amax)
    if tape is not None:
        def bwd_up():
            for o, g in zip(outs, ops.pyramid_upsample_bwd(cat.grad[:, ci:], scales)):
                o._grad = g
        tape.record(bwd_up)
    return bottleneck(cat, tape)


@HEADS.register_module()
class PSPHead(BaseDecodeHead):
    """psp_head.py (PSPNet): [x, resize(ConvModule(AdaptiveAvgPool2d(s)(x))) for s in pool_scales] -> 3x3 bottleneck -> cls_seg.  The pyramid
    is four launches of csrc/pyramid.hip whatever the number of scales: every pooled grid from one read of x, every
    resize into its slice of the concat, and their adjoints; the 1x1 conv -> BN(train, over N s^2 samples) -> ReLU on the small grids are the
    library's layers.  x is copied into its slice.  Returns the bottleneck output as the decoded features (a superset of the reference's
    forward, which has no return_features: `use_decoded_feats` needs them)."""

    def __init__(self, pool_scales=(1, 2, 3, 6), **kwargs):
        super().__init__(**kwargs)
        assert isinstance(pool_scales, (list, tuple))
        self.pool_scales = ops.check_pool_scales(pool_scales)          # NotImplementedError beyond six scales of 1 .. 8
        ci, ch = self.in_channels, self.channels
        self.psp_modules = nn.ModuleList([nn.Sequential(nn.Identity(), ConvModule(ci, ch, 1)) for _ in self.pool_scales])
        self.bottleneck = ConvModule(ci + len(self.pool_scales) * ch, ch, 3, padding=1)

    def forward(self, inputs, return_features=False, tape=None, training=True):
        feats = _ppm_forward(inputs[self.in_index], self.in_channels, self.channels, self.pool_scales, self.psp_modules, self.bottleneck, tape)
        logits = self.cls_seg(feats, tape, training)
        return (logits, feats) if return_features else logits


@HEADS.register_module()
class UPerHead(BaseDecodeHead):
    """uper_head.py (UPerNet): 1x1 laterals on levels 0 .. L-2, the pyramid pooling module and its bottleneck on the last level (PSPHead's
    code path, _ppm_forward), the top-down merges lateral + resize(coarser), a 3x3 fpn_conv per merged level, every level resized to level
    0's grid and concatenated, fpn_bottleneck, cls_seg.  The module names and their construction order are the reference's (its checkpoints
    load key for key).  `in_channels` / `in_index` are lists: the head selects its levels itself (the reference's 'multiple_select'; the
    `input_transform` argument stays refused like for every head).  The merges and the concat are csrc/fpn.hip: one
    pass per merge that also publishes max |.| of the merged map, one launch for the three resized slices.  fpn_convs[0] writes straight into
    slice 0.  Returns the fpn_bottleneck output as the decoded features (pre-dropout, as ASPPHead)."""

    def __init__(self, pool_scales=(1, 2, 3, 6), **kwargs):
        super().__init__(**kwargs)
        assert isinstance(pool_scales, (list, tuple))
        ci, idx = self.in_channels, self.in_index
        if not (isinstance(ci, (list, tuple)) and isinstance(idx, (list, tuple)) and len(ci) == len(idx) and len(ci) >= 2
                and all(isinstance(c, int) and c > 0 for c in ci) and all(isinstance(i, int) for i in idx)):
            raise TypeError(f'UPerHead: in_channels and in_index are lists of equal length >= 2 (one entry per level), got {ci!r} and {idx!r}')
        if len(ci) - 1 > ops.FPN_MAX_LEVELS:
            raise NotImplementedError(f'UPerHead: up to {ops.FPN_MAX_LEVELS + 1} levels (one concat launch), got {len(ci)}')
        self.in_channels, self.in_index = list(ci), list(idx)
        self.pool_scales = ops.check_pool_scales(pool_scales)          # NotImplementedError beyond six scales of 1 .. 8
        ch = self.channels
        self.psp_modules = nn.ModuleList([nn.Sequential(nn.Identity(), ConvModule(ci[-1], ch, 1)) for _ in self.pool_scales])
        self.bottleneck = ConvModule(ci[-1] + len(self.pool_scales) * ch, ch, 3, padding=1)
        self.lateral_convs, self.fpn_convs = nn.ModuleList(), nn.ModuleList()
        for c in ci[:-1]:          # (the top level has neither: its lateral is the PPM's bottleneck)
            self.lateral_convs.append(ConvModule(c, ch, 1))
            self.fpn_convs.append(ConvModule(ch, ch, 3, padding=1))
        self.fpn_bottleneck = ConvModule(len(ci) * ch, ch, 3, padding=1)

    def forward(self, inputs, return_features=False, tape=None, training=True):
        xs = [inputs[i] for i in self.in_index]
        ch, nl = self.channels, len(xs)
        dev = xs[0].data.device
        f16 = layers_mod.CONV_MATH == 'f16x3'
        lats = [self.lateral_convs[i](xs[i], tape) for i in range(nl - 1)]
        top = _ppm_forward(xs[-1], self.in_channels[-1], ch, self.pool_scales, self.psp_modules, self.bottleneck, tape)
        # top-down, from the top level: merged[i] = lats[i] + resize(merged[i + 1]) in a buffer of its own (the lateral layer's backward reads
        # its ReLU output).  Recorded before the fpn_convs, so in backward a merge runs AFTER the fpn_conv of its output level: it finds
        # dL/dmerged[i] complete (fpn_convs[i]'s data gradient, plus the merge below for i > 0), hands that buffer to the lateral as its
        # gradient and adds its adjoint resize to the level above -- each merge is the last writer of its coarser operand, hence the claim
        merged = [None] * (nl - 1) + [top]
        for i in range(nl - 2, -1, -1):
            lat, coarse = lats[i], merged[i + 1]
            coarse.claim_first_use()
            m = Var(None, tape is not None)
            if f16:
                m.amax = ops.amax_slots(dev)          # fpn_convs[i]'s f16x3 scale: published by the merge, no pass of its own
            m.data = ops.topdown_merge(lat.data, coarse.data, amax=m.amax)
            merged[i] = m
            if tape is not None:
                def bwd_merge(m=m, lat=lat, coarse=coarse):
                    g = m.grad
                    buf, acc = coarse.grad_target()
                    ops.resize_bilinear_bwd(g, coarse.data.shape[-2:], out=buf, accumulate=acc)
                    lat._grad = g
                    m.free_grad()
                tape.record(bwd_merge)
        h, w = merged[0].data.shape[-2:]
        cat = _concat_var(merged[0], nl * ch, tape)
        sl = layers_mod.folds_into_concat(self.fpn_bottleneck.conv, h, w, tape is not None)
        if sl:
            cat.coef_table = torch.empty(nl * ch, 4, device=dev)
            cat.coef_table[ch:] = layers_mod.identity_coef_row(dev)          # the resized slices hold final, non-negative values
        self.fpn_convs[0](merged[0], tape, out=cat.slice(0, ch), defer=sl)
        outs = [self.fpn_convs[i](merged[i], tape) for i in range(1, nl - 1)] + [top]
        ops.fpn_resize_concat([o.data for o in outs], cat.data[:, ch:], amax=cat.amax)
        if tape is not None:
            def bwd_concat():
                targets = [o.grad_target() for o in outs]
                ops.fpn_resize_concat_bwd(cat.grad[:, ch:], [t[0] for t in targets], accumulate=[t[1] for t in targets])
            tape.record(bwd_concat)
        if sl:
            cat.lazy = (cat.data, cat.coef_table, None)
        feats = self.fpn_bottleneck(cat, tape)
        logits = self.cls_seg(feats, tape, training)
        return (logits, feats) if return_features else logits


class NeckConvModule(nn.Module):
    """mmcv's ConvModule as the FPN neck builds it: `conv` with a bias and nothing else when norm_cfg is None (the default), conv (no bias) ->
    `bn` [-> ReLU] with norm_cfg=dict(type='BN').  The state-dict keys are the reference's (`conv.weight`, `conv.bias` / `bn.*`)."""

    def __init__(self, cin, cout, k, padding=0, norm=False, act=False):
        super().__init__()
        if act and not norm:
            raise NotImplementedError('FPN: act_cfg without norm_cfg (a bare convolution followed by a ReLU) is outside the PFST path')
        self.conv = Conv2dP(cin, cout, k, 1, padding, bias=not norm)
        self.bn = BatchNorm2dP(cout) if norm else None
        self.act = bool(act)
        nn.init.xavier_uniform_(self.conv.weight)          # init_cfg=dict(type='Xavier', layer='Conv2d', distribution='uniform'); the bias stays 0

    def forward(self, x, tape):
        if self.bn is None:
            return conv_forward(x, self.conv, tape)
        return conv_bn_act(x, self.conv, self.bn, tape, relu=self.act)


@NECKS.register_module()
class FPN(nn.Module):
    """necks/fpn.py: a 1x1 lateral per backbone level, the top-down path merged[i - 1] = lateral[i - 1] + resize(merged[i] -> grid of i - 1) from
    the top, a 3x3 fpn_conv per merged level.  The top-down resize is 'nearest' by default as in the reference (torch's legacy rule for a given
    output size; csrc/fpn.hip pfst_topdown_merge_nearest, one pass per merge that also publishes max |.| of the merged map) or 'bilinear'
    (ops.topdown_merge).  Module names and their order are the reference's, so its checkpoints load key for key.  What the shipped config
    (configs/_base_/models/fpn_r50.py) does not use raises NotImplementedError: extra levels, a level range, scale_factor, conv_cfg.
    The 3x3 layers carry a bias and therefore run on the direct GEMM, not through the Winograd domain (open item)."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False, extra_convs_on_inputs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest'), init_cfg=None):
        super().__init__()
        if not (isinstance(in_channels, (list, tuple)) and len(in_channels) >= 1 and all(isinstance(c, int) and c > 0 for c in in_channels)):
            raise TypeError(f'FPN: in_channels is a list of channel counts, one per level, got {in_channels!r}')
        if add_extra_convs or extra_convs_on_inputs or relu_before_extra_convs:
            raise NotImplementedError('FPN: add_extra_convs (extra levels) is outside the PFST path')
        if num_outs != len(in_channels):
            raise NotImplementedError(f'FPN: num_outs == len(in_channels) (no extra levels), got {num_outs} for {len(in_channels)} levels')
        if start_level != 0 or end_level != -1:
            raise NotImplementedError(f'FPN: every backbone level (start_level=0, end_level=-1), got {start_level}, {end_level}')
        if conv_cfg is not None:
            raise NotImplementedError('FPN: conv_cfg is outside the PFST path')
        if norm_cfg is not None:
            _check_norm(norm_cfg)
        if act_cfg is not None and act_cfg.get('type') != 'ReLU':
            raise NotImplementedError(f"FPN: act_cfg None or dict(type='ReLU'), got {act_cfg!r}")
        up = dict(upsample_cfg)
        if 'scale_factor' in up or up.get('mode') not in ('nearest', 'bilinear') or up.get('align_corners') or set(up) - {'mode', 'align_corners'}:
            raise NotImplementedError(f"FPN: upsample_cfg dict(mode='nearest') or dict(mode='bilinear') for the lateral's size, got {upsample_cfg!r}")
        if len(in_channels) - 1 > ops.FPN_MAX_LEVELS:
            raise NotImplementedError(f'FPN: up to {ops.FPN_MAX_LEVELS + 1} levels (the merge chain), got {len(in_channels)}')
        self.in_channels, self.out_channels, self.num_outs = list(in_channels), out_channels, num_outs
        self.num_ins = len(in_channels)
        self.no_norm_on_lateral, self.upsample_cfg = bool(no_norm_on_lateral), up
        norm, act = norm_cfg is not None, act_cfg is not None
        self.lateral_convs, self.fpn_convs = nn.ModuleList(), nn.ModuleList()
        for c in in_channels:
            self.lateral_convs.append(NeckConvModule(c, out_channels, 1, norm=norm and not self.no_norm_on_lateral,
                                                     act=act and norm and not self.no_norm_on_lateral))
            self.fpn_convs.append(NeckConvModule(out_channels, out_channels, 3, padding=1, norm=norm, act=act))

    def forward(self, inputs, tape=None):
        assert len(inputs) == len(self.in_channels)
        nl = len(inputs)
        nearest = self.upsample_cfg['mode'] == 'nearest'
        f16 = layers_mod.CONV_MATH == 'f16x3'
        lats = [self.lateral_convs[i](inputs[i], tape) for i in range(nl)]
        # top-down, from the top: merged[i] in a buffer of its own (the lateral layer's backward may read its output).  Recorded before the
        # fpn_convs, so in backward a merge runs AFTER the fpn_conv of its output level and finds dL/dmerged[i] complete; it hands that buffer to the
        # lateral as its gradient and adds its adjoint resize to the level above -- the last writer of its coarser operand, hence the claim
        merged = [None] * (nl - 1) + [lats[-1]]
        for i in range(nl - 2, -1, -1):
            lat, coarse = lats[i], merged[i + 1]
            coarse.claim_first_use()
            m = Var(None, tape is not None)
            if f16:
                m.amax = ops.amax_slots(lat.data.device)          # fpn_convs[i]'s f16x3 scale: published by the merge, no pass of its own
            m.data = (ops.topdown_merge_nearest if nearest else ops.topdown_merge)(lat.data, coarse.data, amax=m.amax)
            merged[i] = m
            if tape is not None:
                def bwd_merge(m=m, lat=lat, coarse=coarse):
                    g = m.grad
                    buf, acc = coarse.grad_target()
                    (ops.nearest_resize_bwd if nearest else ops.resize_bilinear_bwd)(g, coarse.data.shape[-2:], out=buf, accumulate=acc)
                    lat._grad = g
                    m.free_grad()
                tape.record(bwd_merge, dict(op='fpn_merge', x=coarse, lat=lat, out=m))
        return [self.fpn_convs[i](merged[i], tape) for i in range(nl)]


class Upsample2x(nn.Module):
    """the parameter-less place of the reference's `Upsample(scale_factor=2, mode='bilinear')` inside FPNHead's scale_heads: it keeps the
    Sequential's indices (the ConvModules at the even positions), the up-sampling itself is fused into the head's kernels"""


@HEADS.register_module()
class FPNHead(BaseDecodeHead):
    """decode_heads/fpn_head.py (Semantic FPN): per level head_length x (3x3 conv -> BN -> ReLU [-> x2 bilinear up-sampling]), every level resized to
    level 0's grid and summed, cls_seg.  `in_channels` / `in_index` are lists: the head selects its levels itself (the reference's
    'multiple_select'; the `input_transform` argument stays refused like for every head).  Module names are the reference's: scale_heads.{i} is
    a Sequential with the ConvModules at its even positions.  csrc/fpn.hip: an intermediate conv -> BN -> ReLU -> x2 is
    never written normalised (pfst_upsample2x_norm normalises on load); level 0's last map and every level whose last convolution lives on
    exactly half of level 0's grid meet in ONE pfst_fpn_level_sum launch -- up-sampling is linear, so y0 + sum_k up2x(y_k) = y0 + up2x(sum_k y_k)
    -- and in backward ONE adjoint resize serves all of them.  A level elsewhere takes the composition of the existing ops into an addend the
    launch adds.  Returns the level sum as the decoded features (pre-dropout, as ASPPHead); Dropout2d stays a pass of its own."""

    def __init__(self, feature_strides, **kwargs):
        super().__init__(**kwargs)
        ci, idx = self.in_channels, self.in_index
        if not (isinstance(ci, (list, tuple)) and isinstance(idx, (list, tuple)) and len(ci) == len(idx) and len(ci) >= 1
                and all(isinstance(c, int) and c > 0 for c in ci) and all(isinstance(i, int) for i in idx)):
            raise TypeError(f'FPNHead: in_channels and in_index are lists of equal length (one entry per level), got {ci!r} and {idx!r}')
        assert len(feature_strides) == len(ci)
        assert min(feature_strides) == feature_strides[0]
        self.in_channels, self.in_index, self.feature_strides = list(ci), list(idx), list(feature_strides)
        self.scale_heads = nn.ModuleList()
        for i, s in enumerate(feature_strides):
            head_length = max(1, int(np.log2(s) - np.log2(feature_strides[0])))
            mods = []
            for k in range(head_length):
                mods.append(ConvModule(ci[i] if k == 0 else self.channels, self.channels, 3, padding=1))
                if s != feature_strides[0]:
                    mods.append(Upsample2x())
            self.scale_heads.append(nn.Sequential(*mods))

    def forward(self, inputs, return_features=False, tape=None, training=True):
        xs = [inputs[i] for i in self.in_index]
        dev = xs[0].data.device
        f16 = layers_mod.CONV_MATH == 'f16x3'
        rec = tape is not None
        src = lambda v: (v.data, None) if v.lazy is None else (v.lazy[0], v.lazy[1])          # (tensor, table) of a layer's output, written or deferred
        lasts = []
        for i, x in enumerate(xs):
            convs = [m for m in self.scale_heads[i] if isinstance(m, ConvModule)]
            ups = self.feature_strides[i] != self.feature_strides[0]
            for k, cm in enumerate(convs):
                if k == len(convs) - 1:
                    lasts.append((x, cm, ups))
                    break
                # conv -> BN -> ReLU -> x2: the up-sampling normalises the pre-BN tensor as it loads it and publishes max |.| for the next conv
                y = cm(x, tape, defer=True)
                up = Var(None, rec)
                if f16:
                    up.amax = ops.amax_slots(dev)
                pre, coef = src(y)
                up.data = ops.upsample2x_norm(pre, coef, amax=up.amax)
                if rec:
                    def bwd_up(y=y, up=up, hw=tuple(pre.shape[-2:])):
                        y._grad = ops.resize_bilinear_bwd(up.grad, hw)
                        up.free_grad()
                    tape.record(bwd_up, dict(op='upsample2x_norm', x=y, out=up))
                x = up
        # the last conv -> BN -> ReLU of every level.  Level 0's map and the maps on exactly half of its grid are read by the sum alone (deferred);
        # any other is written and resized by the existing ops
        x0, cm0, _ = lasts[0]
        h0, w0 = (x0.data if x0.lazy is None else x0.lazy[0]).shape[-2:]
        y0 = cm0(x0, tape, defer=True)
        members, others = [], []
        for x, cm, ups in lasts[1:]:
            h, w = x.data.shape[-2:]
            fused = ups and (2 * h, 2 * w) == (h0, w0) and len(members) < ops.FPN_MAX_LEVELS
            y = cm(x, tape, defer=fused)
            (members if fused else others).append((y, ups))
        addend = None
        for y, ups in others:
            t = y.data
            if ups:
                t = ops.resize_bilinear(t, (2 * t.shape[2], 2 * t.shape[3]))
            if tuple(t.shape[-2:]) != (h0, w0):
                t = ops.resize_bilinear(t, (h0, w0))
            if addend is None:
                addend = t if t is not y.data else t.clone()
            else:
                ops.axpy_(addend, t)
        feats = Var(None, rec)
        if f16:
            feats.amax = ops.amax_slots(dev)                  # conv_seg's f16x3 scale: published by the sum
        pre0, coef0 = src(y0)
        srcs = [src(y) for y, _ in members]
        feats.data = ops.fpn_level_sum(pre0, coef0, [s[0] for s in srcs], [s[1] for s in srcs], addend=addend, amax=feats.amax)
        if rec:
            def bwd_sum():
                # dL/dy0 is dL/dout itself; ONE adjoint resize is the gradient of every half-grid member: their BatchNorm backward passes read
                # the shared buffer (ops.bn_backward writes a dx of its own), each Var only drops its reference; the addend's levels get the
                # adjoints of their compositions
                g = feats.grad
                y0._grad = g
                if members:
                    gh = ops.resize_bilinear_bwd(g, (h0 // 2, w0 // 2))
                    for y, _ in members:
                        y._grad = gh
                for y, ups in others:
                    h, w = y.data.shape[-2:]
                    t = g
                    if ups:
                        if (2 * h, 2 * w) != (h0, w0):
                            t = ops.resize_bilinear_bwd(t, (2 * h, 2 * w))
                        t = ops.resize_bilinear_bwd(t, (h, w))
                    elif (h, w) != (h0, w0):
                        t = ops.resize_bilinear_bwd(t, (h, w))
                    y._grad = t
                feats.free_grad()
            tape.record(bwd_sum, dict(op='fpn_level_sum', x=y0, members=[y for y, _ in members], others=[y for y, _ in others], out=feats))
        logits = self.cls_seg(feats, tape, training)
        return (logits, feats) if return_features else logits


@HEADS.register_module()
class FCNHead(BaseDecodeHead):
    """fcn_head.py: num_convs conv -> BN -> ReLU layers (kernel 1 or 3, any dilation), optionally conv_cat over [x, feats]"""

    @staticmethod
    def _takes_input_transform(in_channels, in_index, input_transform):
        return (input_transform == 'resize_concat' and isinstance(in_channels, (list, tuple)) and isinstance(in_index, (list, tuple))
                and len(in_channels) == len(in_index) >= 1 and all(isinstance(c, int) and c > 0 for c in in_channels)
                and all(isinstance(i, int) for i in in_index))

    def __init__(self, num_convs=2, kernel_size=3, concat_input=True, dilation=1, **kwargs):
        super().__init__(**kwargs)
        if self.input_transform is not None:
            # decode_head.py _init_inputs / _transform_inputs, 'resize_concat': the levels in_index resized to the first one's grid and concatenated
            self.level_channels, self.in_index = list(self.in_channels), list(self.in_index)
            self.in_channels = sum(self.level_channels)
        if not (isinstance(num_convs, int) and num_convs >= 0 and isinstance(dilation, int) and dilation > 0):
            raise ValueError(f'FCNHead: num_convs >= 0 and dilation >= 1, got {num_convs!r}, {dilation!r}')
        if kernel_size not in (1, 3):
            raise NotImplementedError(f'FCNHead: kernel_size 1 or 3, got {kernel_size!r}')
        if num_convs == 0 and self.in_channels != self.channels:
            raise ValueError(f'FCNHead: num_convs=0 needs in_channels == channels, got {self.in_channels} and {self.channels}')
        self.num_convs, self.concat_input, self.kernel_size = num_convs, bool(concat_input), kernel_size
        pad = (kernel_size // 2) * dilation
        convs = [ConvModule(self.in_channels if i == 0 else self.channels, self.channels, kernel_size, padding=pad, dilation=dilation)
                 for i in range(num_convs)]
        self.convs = nn.Sequential(*convs) if convs else nn.Identity()
        if self.concat_input:
            self.conv_cat = ConvModule(self.in_channels + self.channels, self.channels, kernel_size, padding=kernel_size // 2)

    def _resize_concat(self, inputs, tape):
        """level 0 copied, every further level resized (bilinear, align_corners=False) into its channel slice of ONE buffer on level 0's grid;
        every writer publishes max |.| into the buffer's slot group.  One pfst_fpn_resize_concat launch per level: that entry point takes one
        channel count per call and the levels differ in width"""
        xs = [inputs[i] for i in self.in_index]
        cat = _concat_var(xs[0], self.in_channels, tape)
        offs = [sum(self.level_channels[:k]) for k in range(len(xs) + 1)]
        for k, x in enumerate(xs):
            if x.data.shape[1] != self.level_channels[k]:
                raise ValueError(f'FCNHead: level {self.in_index[k]} has {x.data.shape[1]} channels, in_channels says {self.level_channels[k]}')
            dst = cat.data[:, offs[k]:offs[k + 1]]
            if k == 0:
                ops.copy_planes(x.data, dst, amax=cat.amax)
            else:
                ops.fpn_resize_concat([x.data], dst, chan_off=[0], amax=cat.amax)
        if tape is not None:
            def bwd_concat():
                g = cat.grad
                for k, x in enumerate(xs):
                    if not x.requires_grad:
                        continue
                    buf, acc = x.grad_target()
                    gk = g[:, offs[k]:offs[k + 1]]
                    if k == 0:
                        ops.copy_planes(gk, buf, accumulate=acc)
                    else:
                        ops.fpn_resize_concat_bwd(gk, [buf], chan_off=[0], accumulate=acc)
                cat.free_grad()
            tape.record(bwd_concat, dict(op='resize_concat', xs=xs, out=cat))
        return cat

    def forward(self, inputs, return_features=False, tape=None, training=True):
        # (the features this head returns are the PRE-dropout ones, fcn_head.py:92-98, so its Dropout2d stays a pass of its own -- an eighth
        # of the decode head's tensor; the decode head returns the ASPP bottleneck output and folds its dropout, see above)
        x = inputs[self.in_index] if self.input_transform is None else self._resize_concat(inputs, tape)
        if self.num_convs == 1 and not self.concat_input:
            feats = self.convs[0](x, tape)
        else:
            ci, ch = self.in_channels, self.channels
            cat = _concat_var(x, ci + ch, tape) if self.concat_input else None
            feats = x
            for i in range(self.num_convs):
                last = cat is not None and i == self.num_convs - 1
                feats = self.convs[i](feats, tape, out=cat.slice(ci, ci + ch) if last else None)
            if cat is not None:
                if self.num_convs == 0:
                    _identity_into(x, cat, ci, tape)
                _identity_into(x, cat, 0, tape)
                feats = self.conv_cat(cat, tape)
        logits = self.cls_seg(feats, tape, training)
        return (logits, feats) if return_features else logits


@SEGMENTORS.register_module()
class EncoderDecoder(nn.Module):
    def __init__(self, backbone, decode_head, neck=None, auxiliary_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None):
        super().__init__()
        if isinstance(auxiliary_head, (list, tuple)):
            raise NotImplementedError('multiple auxiliary heads are outside the PFST path')
        if pretrained is not None:
            backbone = dict(backbone)
            backbone['pretrained'] = pretrained
        self.backbone = build_backbone(backbone)
        # encoder_decoder.py:35-36: the neck is registered between backbone and decode_head -- the order of the state dict and of the parameter
        # arena, whose 'heads' cut (supervised.py, uda.py) is the first name outside `backbone.`: the neck belongs to the heads' side
        self.neck = build_neck(neck) if neck is not None else None
        self.decode_head = build_head(decode_head)
        self.auxiliary_head = build_head(auxiliary_head) if auxiliary_head is not None else None
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg

    @property
    def with_auxiliary_head(self):
        return self.auxiliary_head is not None

    def init_weights(self):
        self.backbone.init_weights()

    def convs(self):
        return [m for m in self.modules() if isinstance(m, Conv2dP)]

    def module_tree_version(self):
        """a counter that moves whenever a sub-module of this segmentor was replaced, added or removed since the last call (`setattr`, a new
        `conv_seg`, a swapped head ...): the children of every module compared by identity against the tuples recorded at the last walk --
        one tuple compare per module, no walk of the tree while it stands.  What is cached per tree (the conv list, the replayed packing
        plan, the parameter arenas' object lists) is valid for one version."""
        d = self.__dict__
        tree = d.get('_tree')
        if tree is not None:
            for mods, kids in tree:
                if tuple(mods.values()) != kids:
                    break
            else:
                return d['_tree_version']
        d['_tree'] = [(m._modules, tuple(m._modules.values())) for m in self.modules() if m._modules]
        d['_conv_list'] = convs = self.convs()
        d['_conv_params'] = [c._parameters for c in convs]
        d['_tree_version'] = d.get('_tree_version', 0) + 1
        return d['_tree_version']

    def repack_signature(self, need_dgrad=True):
        """what repack_weights compares to choose between replaying its recorded launches and walking the layers again: the switches
        (layers.repack_key), the version of the module tree (the identity of the conv list) and the address of EVERY convolution's weight and
        bias.  Equal signatures: same layers, same decisions, same storage -- in-place updates and zero_grad leave it alone; a rebound
        `.data`, a replaced Parameter or module, a flipped switch change it.  No allocation, no launch, any device."""
        version = self.module_tree_version()
        ptrs = []
        for p in self.__dict__['_conv_params']:
            w, b = p['weight'], p.get('bias')           # (a layer built without a bias keeps None as a plain attribute)
            ptrs.append(w.data_ptr())
            ptrs.append(0 if b is None else b.data_ptr())
        return layers_mod.repack_key(need_dgrad) + (version,) + tuple(ptrs)

    def repack_weights(self, need_dgrad=True):
        """the weight images of every convolution for this step.  The first call walks the layers (modes, buffers, job tables); while
        repack_signature stays the same -- the switches, the module tree, every convolution's weight and bias storage -- later calls replay
        the recorded launches: ~0.15 instead of ~0.8 ms of host time per model (the signature itself: 0.012 ms), at the step boundary where
        the device has nothing queued.  Anything else (a weight rebound with `p.data = ...`, a replaced `conv_seg`) walks the
        layers again and records anew."""
        key = self.repack_signature(need_dgrad)
        convs = self.__dict__['_conv_list']
        plan = self.__dict__.get('_repack_plan')
        if plan is not None and plan[0] == key and WeightBatch.enabled:
            for fn, a in plan[1]:
                fn(*a)
            self._weight_batch.replay()
            return
        batch, rec = None, None
        if WeightBatch.enabled:
            batch = self.__dict__.setdefault('_weight_batch', WeightBatch())
            batch.begin()
            rec = []
        for m in convs:
            m.repack(need_dgrad, batch, rec)
        if batch is not None:
            batch.flush()
        self.__dict__['_repack_plan'] = (key, rec) if rec is not None else None

    def extract_feat(self, img, tape=None, grad_ready=None):
        """backbone [-> neck] (encoder_decoder.py:64-69).  With a neck and a `grad_ready` callback the marker 'heads' is recorded HERE, after the
        backbone's last op and before the neck's first: in backward it fires once every gradient of neck and heads is complete"""
        x = img if isinstance(img, Var) else Var(img, False)
        x = self.backbone(x, tape, grad_ready) if grad_ready is not None else self.backbone(x, tape)
        if self.neck is not None:
            if grad_ready is not None and tape is not None:
                tape.record(lambda: grad_ready('heads'))
            x = self.neck(x, tape)
        return x

    def encode_decode(self, img, img_metas=None):
        """teacher-style forward: no tape, dropout off, BN still in train mode; returns the LOW-resolution
        logits Var (the bilinear upsampling to the image size is fused into the consumers) + states."""
        x = self.extract_feat(img, None)
        logits, states = self.decode_head.forward_test(x, img_metas, self.test_cfg)
        states.update({'feats': x, 'seg_logits': logits})
        return logits, states

    # ------------------------------------------------------------------ test time (encoder_decoder.py:220-372)
    def _eval_encode_decode(self, img):
        """encode_decode as the test loop runs it (model.eval(): BatchNorm on running statistics, dropout off): the logits resized to the
        INPUT size (encoder_decoder.py:72-84) -> (full-size logits tensor, backbone features, low-resolution logits)"""
        with bn_eval():
            x = self.extract_feat(img.contiguous(), None)
            logits = self.decode_head(x, return_features=False, tape=None, training=False)
        return ops.resize_bilinear(logits.data, tuple(img.shape[2:])), x, logits

    def slide_inference(self, img, img_meta, rescale):
        """Inference by sliding window with overlap (encoder_decoder.py:220-263): crops of test_cfg.crop_size every test_cfg.stride pixels,
        the last window of a row / column shifted back inside the image, crop logits summed into place and divided by the cover count.
        An image smaller than the crop is decoded whole, without padding."""
        h_stride, w_stride = self.test_cfg['stride']
        h_crop, w_crop = self.test_cfg['crop_size']
        n, _, h_img, w_img = img.shape
        num_classes = self.decode_head.num_classes
        h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
        w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
        preds = torch.zeros(n, num_classes, h_img, w_img, device=img.device)
        count = torch.zeros(n, 1, h_img, w_img, device=img.device)
        covered = np.zeros((h_img, w_img), bool)                     # the reference's `assert (count_mat == 0).sum() == 0`, without a device read
        for h_idx in range(h_grids):
            for w_idx in range(w_grids):
                y1, x1 = h_idx * h_stride, w_idx * w_stride
                y2, x2 = min(y1 + h_crop, h_img), min(x1 + w_crop, w_img)
                y1, x1 = max(y2 - h_crop, 0), max(x2 - w_crop, 0)
                crop_logit, _, _ = self._eval_encode_decode(img[:, :, y1:y2, x1:x2])
                ops.window_accumulate_(preds, count, crop_logit, y1, x1)
                covered[y1:y2, x1:x2] = True
        assert covered.all()
        ops.window_normalize_(preds, count)
        if rescale:
            preds = ops.resize_bilinear(preds, tuple(img_meta[0]['ori_shape'][:2]))
        return preds

    def inference_probs(self, img, img_meta=None, rescale=True):
        """`inference` of the reference (encoder_decoder.py:284-327): slide / whole logits -> softmax over the classes -> flipped inputs
        flipped back; -> (probabilities [N, C, H, W], states)"""
        mode = (self.test_cfg or {}).get('mode', 'whole')
        assert mode in ('slide', 'whole')
        if img_meta is not None and 'ori_shape' in img_meta[0]:
            assert all(tuple(m['ori_shape']) == tuple(img_meta[0]['ori_shape']) for m in img_meta)
        rescale = bool(rescale and img_meta is not None and 'ori_shape' in img_meta[0])
        self.repack_weights(need_dgrad=False)
        if mode == 'slide':
            seg_logit, states = self.slide_inference(img, img_meta, rescale), {}
        else:
            seg_logit, x, low = self._eval_encode_decode(img)
            size = tuple(img_meta[0]['ori_shape'][:2]) if rescale else tuple(img.shape[2:])
            if size != tuple(img.shape[2:]):
                seg_logit = ops.resize_bilinear(seg_logit, size)          # whole_inference (:269-280): a second resize from the input size
            states = dict(feats=[v.data for v in x], seg_logits=low.data)
        output = ops.softmax_nchw(seg_logit)
        if img_meta is not None and img_meta[0].get('flip'):
            direction = img_meta[0]['flip_direction']
            for d in (direction if isinstance(direction, list) else [direction]):
                assert d in ('horizontal', 'vertical')
                output = ops.flip_planes(output, horizontal=d == 'horizontal', vertical=d == 'vertical')
        return output, states

    def inference(self, img, img_meta=None, rescale=True):
        """-> (argmax label map uint8 [N,H,W], low-res logits or None).  Whole-image mode (all shipped configs): the softmax of the
        reference (`F.softmax(seg_logit)` then `argmax`) is what the fused upsample+softmax+argmax kernel evaluates (its tie rule: §7).
        As in the reference the logits are first resized to the INPUT size (encode_decode, encoder_decoder.py:77-81) and, when `rescale`
        asks for another `ori_shape`, resized a second time from there (whole_inference :269-280); flipped inputs are flipped back
        (:314-325).  Slide mode: the arg-max of `inference_probs`."""
        if self.test_cfg is not None and self.test_cfg.get('mode', 'whole') != 'whole':
            probs, _ = self.inference_probs(img, img_meta, rescale)
            self._last_states = None                              # the reference returns no states in slide mode (:306-307)
            return ops.argmax_nchw(probs), None
        self.repack_weights(need_dgrad=False)
        with bn_eval():
            x = self.extract_feat(img.contiguous(), None)
            logits = self.decode_head(x, return_features=False, tape=None, training=False)
        in_size = tuple(img.shape[2:])
        size = in_size
        if rescale and img_meta is not None and 'ori_shape' in img_meta[0]:
            assert all(tuple(m['ori_shape']) == tuple(img_meta[0]['ori_shape']) for m in img_meta)
            size = tuple(img_meta[0]['ori_shape'][:2])
        src = logits.data if size == in_size else ops.resize_bilinear(logits.data, in_size)
        _, lab8, _ = ops.pseudo_label(src, size, 2.0, want_i64=False)
        if img_meta is not None and img_meta[0].get('flip'):
            direction = img_meta[0]['flip_direction']
            for d in (direction if isinstance(direction, list) else [direction]):
                assert d in ('horizontal', 'vertical')
                lab8 = lab8.flip(dims=(2,) if d == 'horizontal' else (1,))
            lab8 = lab8.contiguous()
        self._last_states = dict(feats=[v.data for v in x], seg_logits=logits.data)
        return lab8, logits.data

    def eval_features(self, img):
        """One whole-image forward as the test loop runs it (BatchNorm on running statistics, dropout off, no tape) that keeps what the
        pseudo-feature statistics read (pfst_amd/statistics.py) -> dict(feats=[the four backbone maps], decoded_feats=the ASPP bottleneck
        output (the head's return_features=True), seg_logits=the low-resolution logits), device tensors.  The logits are those of
        `inference` on the same input, bit for bit (the same launches)."""
        self.repack_weights(need_dgrad=False)
        with bn_eval():
            x = self.extract_feat(img.contiguous(), None)
            logits, decoded = self.decode_head(x, return_features=True, tape=None, training=False)
        return dict(feats=[v.data for v in x], decoded_feats=decoded.data, seg_logits=logits.data)

    def simple_test(self, img, img_meta=None, rescale=True):
        """-> (list of per-image label maps, list of per-image state dicts), the fork's contract (encoder_decoder.py:329-353; consumed as
        `result, state = model(return_loss=False, **data)` by apis/test.py:97).  The states hold the backbone features and the low-res
        logits of each image (device tensors; the reference copies them to the host); empty dicts in slide mode."""
        lab8, _ = self.inference(img, img_meta, rescale)
        st = self._last_states
        if st is None:
            states = [dict() for _ in range(lab8.shape[0])]
        else:
            states = [dict(feats=[f[i] for f in st['feats']], seg_logits=st['seg_logits'][i]) for i in range(lab8.shape[0])]
        self._last_states = None
        return list(lab8.cpu().numpy()), states

    # ------------------------------------------------------------------ test-time augmentation (encoder_decoder.py:355-372)
    @staticmethod
    def _flip_axes(direction):
        """(horizontal, vertical) un-flips of a view: `direction` None (not flipped) or its flip_direction (a name or a list of names,
        each applied once per mention, as `inference` does)"""
        if direction is None:
            return False, False
        d = direction if isinstance(direction, list) else [direction]
        assert all(x in ('horizontal', 'vertical') for x in d), d
        return d.count('horizontal') % 2 == 1, d.count('vertical') % 2 == 1

    def _tta_forward(self, img):
        """the forward of a batch of views -> (src, mid_hw): in whole mode the 1/4-resolution logits and the input size they are resized to
        first (encode_decode); in slide mode the window average at the input size, whose one resize goes to ori_shape"""
        mode = (self.test_cfg or {}).get('mode', 'whole')
        assert mode in ('slide', 'whole')
        hw = tuple(img.shape[2:])
        if mode == 'slide':
            return self.slide_inference(img, None, False), hw
        with bn_eval():
            x = self.extract_feat(img.contiguous(), None)
            logits = self.decode_head(x, return_features=False, tape=None, training=False)
        return logits.data, hw

    @staticmethod
    def _tta_add(acc, src, mid_hw, ori_hw, direction):
        """acc (None: a new sum) += the view's probabilities at ori_shape, un-flipped: pfst_tta_accumulate, or for more than
        ops.TTA_MAX_C classes the chain it fuses (resize, resize, softmax, flip, axpy) -- the same values either way"""
        hflip, vflip = EncoderDecoder._flip_axes(direction)
        n, c = src.shape[:2]
        if c <= ops.TTA_MAX_C:
            first = acc is None
            if first:
                acc = torch.empty(n, c, ori_hw[0], ori_hw[1], device=src.device)
            return ops.tta_accumulate_(acc, src, mid_hw, hflip, vflip, accumulate=not first)
        p = src if tuple(src.shape[2:]) == tuple(mid_hw) else ops.resize_bilinear(src, mid_hw)
        if tuple(mid_hw) != tuple(ori_hw):
            p = ops.resize_bilinear(p, ori_hw)
        p = ops.softmax_nchw(p)
        if hflip or vflip:
            p = ops.flip_planes(p, horizontal=hflip, vertical=vflip)
        if acc is None:
            return p
        ops.axpy_(acc, p)
        return acc

    def aug_test_scale_(self, img, img_meta, flips, acc=None):
        """One scale of a test-time augmentation, the data path's entry (shared by aug_test).  `img` [1, 3, H, W] is the scale's plain view,
        `flips` lists the scale's views in view order, each None (the plain view) or its flip_direction.  ONE forward at batch 1 + D: the view
        and its D distinct flips, made on the device with flip_planes -- exact when the pipeline flips after Resize and the steps after the flip
        are per pixel (Normalize), which the pipeline records as `flip_permutes` --, then each view's probabilities are added to `acc` in view
        order (a duplicated view adds twice).  The f16x3 convolutions scale by the maximum over the batch, so the sum is within the tolerance
        of per-view forwards, not bit-identical to them.  -> acc (None: a new sum) [1, C, *ori_shape]"""
        assert img.shape[0] == 1, 'the paired-flip forward takes one image'
        ori_hw = tuple(img_meta[0]['ori_shape'][:2])
        keys = [self._flip_axes(d) for d in flips]
        distinct = []
        for k in keys:
            if k != (False, False) and k not in distinct:
                distinct.append(k)
        batch = torch.cat([img] + [ops.flip_planes(img.contiguous(), horizontal=h, vertical=v) for h, v in distinct], 0) if distinct else img
        src, mid_hw = self._tta_forward(batch)
        for d, k in zip(flips, keys):
            b = 0 if k == (False, False) else 1 + distinct.index(k)
            acc = self._tta_add(acc, src[b:b + 1], mid_hw, ori_hw, d)
        return acc

    def aug_test_labels(self, imgs, img_metas, rescale=True):
        """aug_test's prediction as a device tensor uint8 [N, *ori_shape].  The views are summed in the reference's order; a run of views of
        one scale whose metas say `flip_permutes` (the pipeline flips after Resize) goes through aug_test_scale_, every other view through
        its own forward.  The sum over views / len(imgs) and the arg-max are one pass (pfst_tta_finalize)."""
        assert rescale
        assert len(imgs) == len(img_metas) and len(imgs) > 0
        ori = tuple(img_metas[0][0]['ori_shape'][:2])
        assert all(tuple(m['ori_shape'][:2]) == ori for ms in img_metas for m in ms)
        self.repack_weights(need_dgrad=False)
        direction = lambda m: m['flip_direction'] if m.get('flip') else None
        acc, i = None, 0
        while i < len(imgs):
            m = img_metas[i][0]
            if imgs[i].shape[0] == 1 and m.get('flip_permutes') and not m.get('flip') and m.get('scale_index') is not None:
                j = i + 1
                while j < len(imgs) and img_metas[j][0].get('scale_index') == m['scale_index']:
                    j += 1
                acc = self.aug_test_scale_(imgs[i], img_metas[i], [direction(img_metas[v][0]) for v in range(i, j)], acc)
                i = j
                continue
            src, mid_hw = self._tta_forward(imgs[i])
            acc = self._tta_add(acc, src, mid_hw, ori, direction(m))
            i += 1
        return ops.tta_finalize(acc, len(imgs))

    def aug_test(self, imgs, img_metas, rescale=True):
        """Test with augmentations (encoder_decoder.py:355-372): the class probabilities of every augmented view, each mapped back to
        `ori_shape` and un-flipped, are averaged; the arg-max of the average is the prediction.  Only rescale=True, like the reference.
        Each view's resizes, softmax, un-flip and sum are one kernel (pfst_tta_accumulate, bit-identical to the separate passes); see
        aug_test_labels for the paired-flip forward of pipeline items."""
        return list(self.aug_test_labels(imgs, img_metas, rescale).cpu().numpy()), {}

    def forward_test(self, imgs, img_metas=None, **kwargs):
        """base.py:74-99: one view -> simple_test, several -> aug_test"""
        if isinstance(imgs, (list, tuple)):
            if len(imgs) != 1:
                if img_metas is None or len(img_metas) != len(imgs):
                    raise ValueError(f'forward_test with {len(imgs)} augmented views needs one img_metas list per view (ori_shape, flip), '
                                     f'got {None if img_metas is None else len(img_metas)}')
                return self.aug_test(list(imgs), list(img_metas), **kwargs)
            imgs, img_metas = imgs[0], (img_metas[0] if img_metas else None)
        return self.simple_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas=None, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    # ------------------------------------------------------------------ supervised training (encoder_decoder.py:127-164)
    def train_step(self, data_batch, optimizer, **kwargs):
        """One supervised iteration on `img` / `img_metas` / `gt_semantic_seg` (any other key is an error) ->
        dict(loss, log_vars, num_samples, states).  The reference's train_step (encoder_decoder.py:127-164, base.py:177-222) PLUS what
        mmcv's OptimizerHook does after it under `optimizer_config = dict()` (no grad_clip): zero_grad, backward, step -- this project's
        runner has no hooks, and PFGST.train_step steps inside as well.  log_vars holds the reference's keys in the reference's order
        (decode.loss_ce, decode.acc_seg, aux.loss_ce, aux.acc_seg, loss) as Python floats; `loss` stays in it (base.py:214 -- only
        PFGST pops it) and is the top-level `loss` too.  `states` is {} unless `self.return_vis_states` is set.  Labels outside
        [0, C) other than ignore_index raise ValueError after the step's single read.  The step itself: pfst_amd/supervised.py."""
        from . import supervised
        return supervised.train_step(self, data_batch, optimizer)

    @property
    def param_arena(self):
        """the flat parameter / gradient arena of the supervised step (None before the first train_step)"""
        from . import supervised
        return supervised.step_state(self).arena

    def forward_train(self, img, img_metas, gt_semantic_seg, seg_weight=None, return_feats=False,
                      return_decoded_feats=False, return_logits=False, return_states=False, tape=None, grad_scale=1.0,
                      grad_ready=None):
        """gt_semantic_seg: uint8 [N,1,H,W]; returns the losses dict (device tensors) like the reference.
        grad_ready: see ResNetV1c.forward; the marker `heads` covers both heads and the neck"""
        x = self.extract_feat(img, tape, grad_ready)
        if grad_ready is not None and tape is not None and self.neck is None:
            tape.record(lambda: grad_ready('heads'))          # (with a neck: recorded by extract_feat, in front of the neck)
        losses, states = dict(), dict()
        loss_decode, state = self.decode_head.forward_train(x, img_metas, gt_semantic_seg, self.train_cfg, seg_weight,
                                                            tape=tape, grad_scale=grad_scale)
        losses.update(add_prefix(loss_decode, 'decode'))
        states.update(state)
        if self.with_auxiliary_head:
            loss_aux, state_aux = self.auxiliary_head.forward_train(x, img_metas, gt_semantic_seg, self.train_cfg,
                                                                    seg_weight, tape=tape, grad_scale=grad_scale)
            losses.update(add_prefix(loss_aux, 'aux'))
            states.update(add_prefix(state_aux, 'aux'))
        if return_feats:
            losses['features'] = x
        if return_logits:
            losses['logits'] = state['seg_logits']
        if return_decoded_feats:
            losses['decoded_features'] = state['decoded_features']
        return (losses, states) if return_states else losses
