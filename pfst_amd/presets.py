"""The four shipped PFST configurations as plain dicts (values of the reference's
configs/_base_/models/deeplabv3plus_r50-d8.py:2-46, configs/_base_/uda/pfst.py:7-34,
configs/_base_/schedules/adamw_40k.py:4-21 and configs/pfst/*.py:17-53 after `_base_` merging), so that bench.py
and the GPU tests can build the workload without the reference tree.  `Config.fromfile` loads the reference's own
files unchanged when they are available (tests/test_config_dropin.py)."""
import copy

NORM_CFG = dict(type='BN', requires_grad=True)


def model_cfg(num_classes=6, in_channels=3, dropout=0.1):
    return dict(
        type='EncoderDecoder', pretrained=None,
        backbone=dict(type='ResNetV1c', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), dilations=(1, 1, 2, 4),
                      strides=(1, 2, 1, 1), norm_cfg=dict(NORM_CFG), norm_eval=False, style='pytorch',
                      contract_dilation=True, in_channels=in_channels),
        decode_head=dict(type='DepthwiseSeparableASPPHead', in_channels=2048, in_index=3, channels=512,
                         dilations=(1, 12, 24, 36), c1_in_channels=256, c1_channels=48, dropout_ratio=dropout,
                         num_classes=num_classes, norm_cfg=dict(NORM_CFG), align_corners=False,
                         loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
        auxiliary_head=dict(type='FCNHead', in_channels=1024, in_index=2, channels=256, num_convs=1, concat_input=False,
                            dropout_ratio=dropout, num_classes=num_classes, norm_cfg=dict(NORM_CFG), align_corners=False,
                            loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=0.4)),
        train_cfg=dict(), test_cfg=dict(mode='whole'))


BASELINE_KINDS = ('pspnet', 'deeplabv3', 'fcn', 'upernet', 'fpn', 'hrnet')


def baseline_model_cfg(kind, num_classes, in_channels, depth=50, dropout=0.1, width=18):
    """The comparison models of the reference (configs/_base_/models/pspnet_r50-d8.py, deeplabv3_r50-d8.py, fcn_r50-d8.py): the same
    ResNetV1c-d8 backbone and auxiliary FCN head on layer3 as model_cfg, under a PSPHead, an ASPPHead or a two-layer FCNHead with
    concat_input; 'upernet' (upernet_r50.py) is a UPerHead over all four levels of the stride-32 backbone, strides (1, 2, 2, 2) without
    dilation, with the same auxiliary head; 'fpn' (fpn_r50.py, Semantic FPN) is that stride-32 backbone under an FPN neck (256 channels, four
    levels, nearest top-down path) and an FPNHead (128 channels, feature strides 4 .. 32) -- WITHOUT an auxiliary head, as the reference's file.  Plain BN, as the reference's DeepLabV3+ file; `depth` 50 or 101 (the reference's PSPNet file runs 101).  The class
    weights of the reference's two-class PSPNet edit are a property of its data set: add `class_weight` to the loss dicts where wanted.
    'hrnet' (fcn_hr18.py) is another backbone altogether: HRNet-W`width` (18, or 48 for fcn_hr48) under a one-layer 1x1 FCNHead that reads all
    four branches through input_transform='resize_concat', channels = the sum of the widths, dropout_ratio -1 (no dropout), no auxiliary
    head; plain BN; `depth` and `dropout` do not apply."""
    if kind not in BASELINE_KINDS:
        raise ValueError(f'baseline_model_cfg: kind must be one of {BASELINE_KINDS}, got {kind!r}')
    if kind == 'hrnet':
        widths = [width, 2 * width, 4 * width, 8 * width]
        extra = dict(stage1=dict(num_modules=1, num_branches=1, block='BOTTLENECK', num_blocks=(4,), num_channels=(64,)),
                     stage2=dict(num_modules=1, num_branches=2, block='BASIC', num_blocks=(4, 4), num_channels=tuple(widths[:2])),
                     stage3=dict(num_modules=4, num_branches=3, block='BASIC', num_blocks=(4, 4, 4), num_channels=tuple(widths[:3])),
                     stage4=dict(num_modules=3, num_branches=4, block='BASIC', num_blocks=(4, 4, 4, 4), num_channels=tuple(widths)))
        return dict(type='EncoderDecoder', pretrained=None,
                    backbone=dict(type='HRNet', norm_cfg=dict(NORM_CFG), norm_eval=False, extra=extra, in_channels=in_channels),
                    decode_head=dict(type='FCNHead', in_channels=widths, in_index=[0, 1, 2, 3], channels=sum(widths),
                                     input_transform='resize_concat', kernel_size=1, num_convs=1, concat_input=False, dropout_ratio=-1,
                                     num_classes=num_classes, norm_cfg=dict(NORM_CFG), align_corners=False,
                                     loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)),
                    train_cfg=dict(), test_cfg=dict(mode='whole'))
    cfg = model_cfg(num_classes, in_channels, dropout)
    cfg['backbone']['depth'] = depth
    common = dict(in_channels=2048, in_index=3, channels=512, dropout_ratio=dropout, num_classes=num_classes, norm_cfg=dict(NORM_CFG),
                  align_corners=False, loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
    head = dict(pspnet=dict(type='PSPHead', pool_scales=(1, 2, 3, 6)), deeplabv3=dict(type='ASPPHead', dilations=(1, 12, 24, 36)),
                fcn=dict(type='FCNHead', num_convs=2, concat_input=True), upernet=dict(type='UPerHead', pool_scales=(1, 2, 3, 6)),
                fpn=dict(type='FPNHead'))[kind]
    cfg['decode_head'] = dict(head, **common)
    if kind == 'upernet':
        # configs/_base_/models/upernet_r50.py: the stride-32 backbone (no dilation) under a head that reads all four levels
        cfg['backbone'].update(strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1))
        cfg['decode_head'].update(in_channels=[256, 512, 1024, 2048], in_index=[0, 1, 2, 3])
    if kind == 'fpn':
        # configs/_base_/models/fpn_r50.py: the same stride-32 backbone, an FPN neck, FPNHead over its four outputs, no auxiliary head
        cfg['backbone'].update(strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1))
        cfg['neck'] = dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=4)
        cfg['decode_head'] = dict(type='FPNHead', in_channels=[256, 256, 256, 256], in_index=[0, 1, 2, 3], feature_strides=[4, 8, 16, 32],
                                  channels=128, dropout_ratio=dropout, num_classes=num_classes, norm_cfg=dict(NORM_CFG), align_corners=False,
                                  loss_decode=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0))
        del cfg['auxiliary_head']
    return cfg


def uda_cfg(num_classes=6, in_channels=3, dropout=0.1, blur=True, color_jitter_probability=0.2, downscale=0.5,
            pseudo_threshold=0.98, max_iters=40000):
    return dict(
        type='PFGST', alpha=0.999, pseudo_threshold=pseudo_threshold, pseudo_weight_ignore_top=0,
        pseudo_weight_ignore_bottom=0, imnet_feature_dist_lambda=0, imnet_feature_dist_classes=None,
        imnet_feature_dist_scale_min_ratio=None, mix='class', blur=blur, color_jitter_strength=0.2,
        color_jitter_probability=color_jitter_probability, print_grad_magnitude=False, thre_type='all',
        trg_loss_weight=1., use_decoded_feats=True,
        aux_losses=[dict(type='PFGSTLoss', kernel_size=3, dilation=2, top_k=3,
                         weights={'src_pos': 0.1, 'src_neg': 0.1, 'sim_pos': 0.1, 'sim_neg': 0.1,
                                  'src_pos_std': 0.1, 'src_neg_std': 0.1},
                         sim_type='cosine', feat_level=None, detach_unfold=True, downscale=downscale)],
        model=model_cfg(num_classes, in_channels, dropout), max_iters=max_iters)


def dacs_uda_cfg(num_classes=6, in_channels=3, dropout=0.1, blur=True, color_jitter_probability=0.2, pseudo_threshold=0.968,
                 max_iters=40000):
    """The DACS self-training baseline with the values of the reference's configs/_base_/uda/dacs.py:7-22: uda_cfg's arguments without
    the PFGSTLoss ones, no auxiliary losses"""
    return dict(
        type='DACS', alpha=0.99, pseudo_threshold=pseudo_threshold, pseudo_weight_ignore_top=0, pseudo_weight_ignore_bottom=0,
        imnet_feature_dist_lambda=0, imnet_feature_dist_classes=None, imnet_feature_dist_scale_min_ratio=None, mix='class', blur=blur,
        color_jitter_strength=0.2, color_jitter_probability=color_jitter_probability, debug_img_interval=1000, print_grad_magnitude=False,
        model=model_cfg(num_classes, in_channels, dropout), max_iters=max_iters)


# Adversarial baseline (ADVENT).  The reference ships the model (DomainAdaptorAdv, FCDiscriminator, AdvLoss) but NO config for it: these
# defaults are the ADVENT paper's (Vu et al., CVPR 2019: lambda_adv = 0.001 on the generator's adversarial term, the discriminator's two
# terms halved, Adam with lr 1e-4 and betas (0.9, 0.99) for the discriminator), not numbers of the reference.  The project builds AdamW and
# SGD only: the discriminator takes AdamW with weight_decay = 0, which is torch.optim.Adam's update without weight decay.
ADVENT_WEIGHTS = dict(loss_gen=0.001, loss_disc_src=0.5, loss_disc_trg=0.5)
ADVENT_DISC_OPTIMIZER = dict(type='AdamW', lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0)


def advent_cfg(model, generator_optimizer=None, ndf=64, weights=None):
    """-> dict(model=..., optimizer=...) of the adversarial baseline around a segmentor cfg `model` (e.g. model_cfg()): the segmentor turned
    into a DomainAdaptorAdv with an FCDiscriminator on the per-class entropy maps and the two AdvLoss lists; optimizer = one entry per
    sub-network (optim.build_optimizers): the generator keeps `generator_optimizer` (default: the PFST recipe's AdamW)"""
    w = dict(ADVENT_WEIGHTS, **(weights or {}))
    m = copy.deepcopy(dict(model))
    m['type'] = 'DomainAdaptorAdv'
    m['discriminator'] = dict(type='FCDiscriminator', num_in_channels=m['decode_head']['num_classes'], ndf=ndf)
    m['disc_losses'] = [dict(type='AdvLoss', loss_type='advent', net_type='disc',
                             weights=dict(loss_disc_src=w['loss_disc_src'], loss_disc_trg=w['loss_disc_trg']))]
    m['gen_losses'] = [dict(type='AdvLoss', loss_type='advent', net_type='gen', weights=dict(loss_gen=w['loss_gen']))]
    return dict(model=m, optimizer=dict(generator=copy.deepcopy(dict(generator_optimizer or OPTIMIZER)),
                                        discriminator=dict(ADVENT_DISC_OPTIMIZER)))


OPTIMIZER = dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01)
LR_CONFIG = dict(policy='poly', warmup='linear', warmup_iters=1500, warmup_ratio=1e-6, power=1.0, min_lr=0.0, by_epoch=False)

# configs/_base_/schedules/schedule_40k.py:2-5 (the supervised schedules; 20k ... 320k differ in max_iters and the intervals only)
SGD_OPTIMIZER = dict(type='SGD', lr=0.01, momentum=0.9, weight_decay=0.0005)
SGD_LR_CONFIG = dict(policy='poly', power=0.9, min_lr=1e-4, by_epoch=False)

# BASELINE.json configs[1..4]: name -> (num_classes, in_channels, tile size, per-GPU batch, PFGSTLoss downscale)
WORKLOADS = {
    'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8': dict(num_classes=6, in_channels=3, size=1024, per_gpu_batch=8, downscale=0.5),
    'pfst_vaih_irrg2pots_irrg_deeplabv3plus_r50-d8': dict(num_classes=6, in_channels=3, size=1024, per_gpu_batch=8, downscale=0.5),
    'pfst_inria_da_deeplabv3plus_r50-d8': dict(num_classes=2, in_channels=3, size=1024, per_gpu_batch=8, downscale=0.5),
    'pfst_season_net_sp2fa_deeplabv3plus_r50-d8': dict(num_classes=33, in_channels=10, size=512, per_gpu_batch=8, downscale=1,
                                                       strong_aug_denorm_type='none'),
}


def workload_cfg(name, **overrides):
    w = dict(WORKLOADS[name])
    cfg = uda_cfg(w['num_classes'], w['in_channels'], downscale=w['downscale'])
    if 'strong_aug_denorm_type' in w:                   # configs/pfst/pfst_season_net_sp2fa_*.py:53
        cfg['strong_aug_denorm_type'] = w['strong_aug_denorm_type']
    in_channels = overrides.pop('in_channels', None)    # e.g. the SHIPPED 3-band SeasonNet variant of BASELINE config #5
    if in_channels is not None:
        cfg['model']['backbone']['in_channels'] = w['in_channels'] = in_channels
    cfg.update(overrides)
    return copy.deepcopy(cfg), w
