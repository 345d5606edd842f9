#!/usr/bin/env python3
"""Train a PFST model on MI355X -- the flag surface of the reference's tools/train.py:23-107 on top of pfst_amd.

  python tools/train.py configs/pfst/pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8.py --work-dir work_dirs/x
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/train.py CONFIG --launcher pytorch

`--synthetic` trains on seeded synthetic tiles (benchmarks); otherwise `cfg.data.train` (UDADataset: source / target folders of
converted tiles, each with the config's own pipeline list) is read by pfst_amd/data.py + pfst_amd/pipeline.py, and
`cfg.data.val` is evaluated every `evaluation.interval` iterations unless --no-validate (rsiseg/apis/train.py:152-168).

Supervised training (source-only / target-only baselines, a source-trained start for self-training): a config WITHOUT a `uda` section
builds a bare EncoderDecoder (registry.build_train_model) whose own train_step runs; `cfg.data.train` is then a plain dataset dict
(type / data_root / img_dir / ann_dir / pipeline) and the optimizer usually the SGD of configs/_base_/schedules/schedule_*.py.
`--supervised` drops the `uda` section of a config or preset (a UDADataset in data.train is replaced by its `source` entry; a preset takes
schedule_40k's SGD + poly schedule); `--supervised --model pspnet|deeplabv3|fcn|upernet|fpn|hrnet` swaps in the reference's comparison models (PSPNet,
DeepLabV3, FCN on the same backbone, UPerNet and Semantic FPN -- neck included -- on the stride-32 one: presets.baseline_model_cfg), `--synthetic` included.  Checkpoints of such a run have bare keys: tools/test.py reads them without key revision, and
`--init-student-from CKPT` starts a self-training run (a `uda` config) with them in both the student and the EMA teacher.

Self-training baselines: `--uda dacs` swaps the `uda` section for DACS (rsiseg/models/uda/dacs.py), `--synthetic` included; MinEnt and
max-squares are PFGST with an EntropyLoss among its auxiliary losses, e.g.
`--cfg-options "uda.aux_losses=[{'type':'EntropyLoss','loss_type':'entropy','weights':{'loss_ent':W}}]"` (W: yours to choose, README).

Adversarial baseline: `--adversarial advent` drops the `uda` section and turns cfg.model into a DomainAdaptorAdv with an FCDiscriminator on
the entropy maps (presets.advent_cfg; optimizer = one entry per sub-network), `--synthetic` included.  The reference ships no config for
this model: the loss weights and the discriminator's optimizer are the ADVENT paper's (README).  It is a flag of its own because `--uda`
names a self-training wrapper kept in the `uda` section, which this model does not have (`--uda advent` stays an unknown choice)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Train a segmentor (pfst_amd)')
    p.add_argument('config', help='train config file path (reference format) or a preset name from pfst_amd.presets')
    p.add_argument('--work-dir')
    p.add_argument('--load-from')
    p.add_argument('--init-student-from', help='a bare-keyed segmentor checkpoint (backbone.* / decode_head.* / auxiliary_head.*, e.g. of a '
                                               'supervised run) loaded into the student AND the EMA teacher of a `uda` config; every key must match')
    p.add_argument('--supervised', action='store_true', help='drop the `uda` section: train the bare segmentor on img / gt_semantic_seg')
    p.add_argument('--model', choices=['pspnet', 'deeplabv3', 'fcn', 'upernet', 'fpn', 'hrnet'],
                   help='with --supervised: replace cfg.model by the comparison model of that name (presets.baseline_model_cfg: PSPHead / ASPPHead / '
                        'two-layer FCNHead on the same backbone and auxiliary head; upernet / fpn: the stride-32 backbone, fpn with its FPN neck and no '
                        'auxiliary head; hrnet: HRNet-W18 under a one-layer FCNHead over its four branches, no auxiliary head), keeping num_classes and in_channels, and -- for the ResNetV1c models -- the backbone depth and the dropout ratio (hrnet has neither: width 18, no dropout)')
    p.add_argument('--uda', choices=['dacs'],
                   help='replace the `uda` section of the config or preset by the DACS self-training baseline (presets.dacs_uda_cfg: the values of '
                        "the reference's configs/_base_/uda/dacs.py, no auxiliary losses), keeping strong_aug_denorm_type, a property of the data")
    p.add_argument('--adversarial', choices=['advent'],
                   help='drop the `uda` section of the config or preset and train cfg.model adversarially (presets.advent_cfg: DomainAdaptorAdv + '
                        'FCDiscriminator on the entropy maps, one optimizer each); --uda names a self-training wrapper and keeps refusing this name')
    p.add_argument('--resume-from')
    p.add_argument('--no-validate', action='store_true')
    g = p.add_mutually_exclusive_group()
    g.add_argument('--gpus', type=int)
    g.add_argument('--gpu-ids', type=int, nargs='+')
    g.add_argument('--gpu-id', type=int, default=0)
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--diff_seed', action='store_true')
    p.add_argument('--deterministic', action='store_true')
    p.add_argument('--options', nargs='+')
    p.add_argument('--cfg-options', nargs='+')
    p.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none')
    p.add_argument('--local_rank', '--local-rank', type=int, default=0)
    p.add_argument('--auto-resume', action='store_true')
    p.add_argument('--synthetic', action='store_true', help='seeded synthetic batches instead of cfg.data')
    p.add_argument('--random-init', action='store_true',
                   help='train from random initialisation when cfg.model.pretrained cannot be loaded (model-zoo URL, no network)')
    p.add_argument('--max-iters', type=int, default=None)
    p.add_argument('--batch-size', type=int, default=None)
    p.add_argument('--crop-size', type=int, default=None)
    p.add_argument('--workers', type=int, default=None, help='data-loading worker processes per GPU (default: cfg.data.workers_per_gpu)')
    p.add_argument('--seeding', choices=['sample', 'worker'], default='sample',
                   help="'sample': one RNG stream per sample (batches independent of the worker count); 'worker': the reference's "
                        'worker_init_fn (rsiseg/datasets/builder.py:170-181)')
    args = p.parse_args(argv)
    if args.options and args.cfg_options:
        raise ValueError('--options and --cfg-options cannot be both specified')
    if args.options:
        args.cfg_options = args.options
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    return args


def load_cfg(args):
    from pfst_amd.config import Config, parse_cfg_options
    from pfst_amd.presets import LR_CONFIG, OPTIMIZER, SGD_LR_CONFIG, SGD_OPTIMIZER, WORKLOADS, workload_cfg
    if os.path.exists(args.config):
        cfg = Config.fromfile(args.config)
    elif args.config in WORKLOADS:
        uda, w = workload_cfg(args.config)
        opt, lr = (SGD_OPTIMIZER, SGD_LR_CONFIG) if args.supervised else (OPTIMIZER, LR_CONFIG)
        cfg = Config(dict(model=uda.pop('model'), uda=uda, optimizer=dict(opt), lr_config=dict(lr),
                          runner=dict(type='IterBasedRunner', max_iters=40000), checkpoint_config=dict(by_epoch=False, interval=4000),
                          evaluation=dict(interval=4000, metric='mIoU'), log_config=dict(interval=50),
                          data=dict(samples_per_gpu=w['per_gpu_batch']), seed=0))
    else:
        raise FileNotFoundError(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    if args.model:
        if not args.supervised:
            raise ValueError('--model builds a comparison model for supervised training: pass --supervised (self-training over these heads takes '
                             'a config whose PFGSTLoss has downscale=None, README)')
        from pfst_amd.presets import baseline_model_cfg
        old = cfg.model
        new = baseline_model_cfg(args.model, old['decode_head']['num_classes'], old['backbone'].get('in_channels', 3),
                                 depth=old['backbone'].get('depth', 50), dropout=old['decode_head'].get('dropout_ratio', 0.1))
        new['pretrained'] = old.get('pretrained')
        cfg.model = new
        if args.cfg_options:                                  # options addressed at the new model's keys apply to it
            cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    if args.uda:
        if args.supervised or 'uda' not in cfg:
            raise ValueError('--uda swaps the self-training wrapper of a config with a `uda` section: it cannot be combined with --supervised '
                             'or a supervised config')
        if args.adversarial:
            raise ValueError('--uda and --adversarial each replace the `uda` section: pass one of them')
        from pfst_amd.presets import dacs_uda_cfg
        old = cfg.uda
        new = dacs_uda_cfg()
        new.pop('model'), new.pop('max_iters')                # build_train_model hands both in (cfg.model, cfg.runner.max_iters)
        if 'strong_aug_denorm_type' in old:
            new['strong_aug_denorm_type'] = old['strong_aug_denorm_type']
        cfg.uda = new
        if args.cfg_options:                                  # options addressed at the new section's keys apply to it
            cfg.merge_from_dict(parse_cfg_options(args.cfg_options))
    if args.adversarial:
        if args.supervised or 'uda' not in cfg:
            raise ValueError('--adversarial replaces the self-training wrapper of a config with a `uda` section: it cannot be combined with '
                             '--supervised or a supervised config')
        # no teacher, no mixing: the `uda` wrapper goes, the segmentor itself becomes the adversarial model and brings two optimizers
        from pfst_amd.presets import advent_cfg
        if cfg.model.get('type', 'EncoderDecoder') != 'EncoderDecoder':
            raise ValueError(f"--adversarial advent wraps an EncoderDecoder model cfg, got type {cfg.model.get('type')!r}")
        # the config's single optimizer becomes the generator's.  Options addressed at the sections that exist only after this rewrite
        # (optimizer.generator.*, optimizer.discriminator.*) were merged into it above as stray sub-dicts: they are taken out here and land
        # where they belong in the merge below
        gen_opt = {k: v for k, v in dict(cfg.get('optimizer') or {}).items()
                   if not (k in ('generator', 'discriminator') and isinstance(v, dict))}
        if 'type' not in gen_opt:
            raise ValueError('--adversarial advent takes the generator\'s optimizer from the config\'s `optimizer` section, which must be one '
                             f'optimizer with a `type`; got keys {sorted(gen_opt)}')
        new = advent_cfg(cfg.model.to_dict() if hasattr(cfg.model, 'to_dict') else dict(cfg.model), generator_optimizer=gen_opt)
        cfg.pop('uda')
        cfg.model, cfg.optimizer = new['model'], new['optimizer']
        if args.cfg_options:                                  # options addressed at the new sections' keys apply to them
            # (an option of the single optimizer, e.g. optimizer.weight_decay, went into the generator's section above: not merged again)
            sub = ('optimizer.generator', 'optimizer.discriminator')
            cfg.merge_from_dict({k: v for k, v in parse_cfg_options(args.cfg_options).items()
                                 if not (k + '.').startswith('optimizer.') or k in sub or k.startswith(tuple(s + '.' for s in sub))})
    if args.max_iters:
        cfg.runner['max_iters'] = args.max_iters
    if args.supervised:
        cfg.pop('uda', None)
        train = (cfg.get('data') or {}).get('train')
        if train is not None and 'source' in train:          # a source / target pairing: the supervised run reads its source entry
            cfg.data['train'] = train['source']
    if 'uda' not in cfg and ((cfg.get('optimizer_config') or {}).get('grad_clip') is not None):
        raise NotImplementedError('optimizer_config.grad_clip: EncoderDecoder.train_step implements the hook without gradient clipping '
                                  '(optimizer_config = dict(), every shipped schedule)')
    return cfg


def main(argv=None):
    args = parse_args(argv)
    import torch
    import torch.distributed as dist
    import pfst_amd  # noqa: F401
    from pfst_amd import dist as pdist
    from pfst_amd.data import build_dataset, build_loader, synthetic_loader
    from pfst_amd.evaluation import build_eval_fn
    from pfst_amd.optim import build_optimizers
    from pfst_amd.registry import build_train_model
    from pfst_amd.runner import IterBasedRunner, find_latest_checkpoint, init_random_seed, init_student_from, set_random_seed

    cfg = load_cfg(args)
    distributed = args.launcher != 'none'
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    torch.cuda.set_device(local_rank if distributed else args.gpu_id)
    dev = torch.device('cuda', torch.cuda.current_device())
    if distributed:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group((cfg.get('dist_params') or {}).get('backend', 'nccl'), device_id=dev)
    rank = dist.get_rank() if distributed else 0
    world = dist.get_world_size() if distributed else 1
    work_dir = args.work_dir or cfg.get('work_dir') or os.path.join('./work_dirs', os.path.splitext(os.path.basename(args.config))[0])
    seed = init_random_seed(args.seed if args.seed is not None else cfg.get('seed'), dev)
    seed = seed + rank if args.diff_seed else seed
    set_random_seed(seed, args.deterministic)

    adversarial = cfg.model.get('type') == 'DomainAdaptorAdv'          # no `uda` wrapper either, but it reads the source / target batch
    supervised = 'uda' not in cfg and not adversarial
    if args.init_student_from and supervised:
        raise SystemExit('--init-student-from fills the student and the teacher of a `uda` wrapper; a supervised run takes --load-from')
    load_from = args.load_from or cfg.get('load_from')
    resume = args.resume_from or cfg.get('resume_from')
    if resume is None and args.auto_resume:
        resume = find_latest_checkpoint(work_dir)
    pretrained = cfg.model.get('pretrained')
    if pretrained and not os.path.exists(str(pretrained)):
        # e.g. 'open-mmlab://resnet50_v1c': a model-zoo URL cannot be fetched here.  Never silently replace it by random weights.
        if not (load_from or resume or args.init_student_from or args.random_init or args.synthetic):
            raise SystemExit(f'cfg.model.pretrained={pretrained!r} cannot be loaded offline: give --load-from / --resume-from a '
                             'checkpoint, point `pretrained` to a local file, or pass --random-init explicitly')
        cfg.model['pretrained'] = None
    model = build_train_model(cfg)
    model.init_weights()
    model.to(dev)
    optimizer = build_optimizers(model, cfg.optimizer)
    nc = cfg.model.decode_head.num_classes
    eval_fn = None
    data_cfg = cfg.get('data') or {}
    if not args.no_validate and not args.synthetic and 'val' in data_cfg:
        ev = cfg.get('evaluation') or {}
        eval_fn = build_eval_fn(data_cfg['val'], nc, dev, metric=ev.get('metric', 'mIoU'))
    runner = IterBasedRunner(model, optimizer, cfg, work_dir, eval_fn=eval_fn)
    if args.deterministic and rank == 0:
        # measured at b = 8 x 1024^2 (tools/det_cost.py): 296 ms against 288 ms per step -- the split-K slices of the weight gradients go through a
        # scratch and an ordered reduction instead of atomics, the launch shapes are the default mode's
        runner.log('deterministic mode: weight gradients / BatchNorm-backward / depthwise / bias sums in a fixed order -- bit-reproducible '
                   'gradients run to run and for any stream schedule; about 3 % slower (compare the `time` column with a run without '
                   '--deterministic)')
    if args.init_student_from and not resume:            # a resumed run continues from its own checkpoint
        init_student_from(model, args.init_student_from)
        runner.log(f'student and EMA teacher initialised from {args.init_student_from}')
    if load_from:
        runner.load_checkpoint(load_from)
    if resume:
        runner.resume(resume)
    # every rank continues from rank 0's parameters and buffers (what MMDistributedDataParallel's constructor does in the reference);
    # only then may the per-rank random streams diverge (--diff_seed)
    pdist.broadcast_module_state_(model)

    bs = args.batch_size or data_cfg.get('samples_per_gpu', 2)
    cin = cfg.model.backbone.get('in_channels', 3)
    if args.synthetic or 'train' not in data_cfg:
        loader = synthetic_loader(bs, args.crop_size or 1024, nc, cin, seed=1234 + rank, device=dev)
        if supervised:                       # the synthetic batches without their target side
            loader = ({k: v for k, v in b.items() if not k.startswith('target_')} for b in loader)
    else:
        # img_scale / ratio_range / crop_size / reduce_zero_label / flips / photometric steps all come from the config's pipelines
        dataset = build_dataset(data_cfg['train'])
        model.CLASSES = dataset.CLASSES
        model.PALETTE = dataset.PALETTE
        # the RESOLVED seed (--seed / cfg.seed / the broadcast random one) drives the sampler's shuffle (apis/train.py:74-89 passes
        # cfg.seed to build_dataloader) and the per-sample streams; the data side never touches the training thread's NumPy stream
        workers = args.workers if args.workers is not None else int(data_cfg.get('workers_per_gpu', 0))
        loader = build_loader(dataset, bs, dev, seed=seed, rank=rank, world=world, workers=workers, seeding=args.seeding,
                              start_epoch=runner.epoch)          # a resumed run continues with the checkpoint's data epoch
    runner.run(iter(loader))
    runner.save_checkpoint()
    if hasattr(loader, 'close'):
        loader.close()                       # stop the data-loading worker processes
    if distributed:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
