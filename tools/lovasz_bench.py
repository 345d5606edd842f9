#!/usr/bin/env python3
"""Times LovaszLoss (csrc/lovasz_loss.hip) at the flagship workload's shape -- 8 tiles, 6 classes, the decode head's 256^2
logits to 1024^2 labels (the x4 block route) -- forward (key pass, segmented radix sort, gradient pass, finalize: each between device
events) and backward, beside a torch restatement of the reference on the same device in the same process: materialise the up-sampled logits,
softmax, per class |fg - p|, `torch.sort`, cumsum, the dot product, autograd.  The two alternate, round by round; the median over --rounds.
Then a supervised step (EncoderDecoder.train_step under SGD, the step `tools/train.py --synthetic --supervised` runs) with [CE, Lovasz]
against [CE] on the decode head, alternating blocks, host clock between device synchronisations.  One JSON line (and --out FILE).

  python tools/lovasz_bench.py [--tiles 8] [--classes 6] [--size 1024] [--rounds 9] [--warmup 2] [--steps 12] [--no-step] [--out FILE]

Bytes, from the shapes (E = classes x tiles x size^2 elements, 8 bytes per (key, value) pair): the key pass writes 8 E; each of the four
sort passes reads the keys for the histograms (4 E), reads the pairs and writes them (16 E): 20 E a pass, 80 E in all; the gradient pass
reads the values (4 E), then the pairs (8 E), and scatters 4 E of coefficients; the backward reads the 4 E coefficient map."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAME = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
STAGES = ('keys', 'sort', 'grad', 'finalize')


def torch_lovasz(logits, label, ignore_index=255):
    """lovasz_loss.py (lovasz_softmax_flat, classes='present', per_image=False) behind the decode head's resize, statement for statement, on
    the device -> (loss, d loss / d logits)"""
    import torch
    import torch.nn.functional as F
    z = logits.detach().requires_grad_()
    probs = F.softmax(F.interpolate(z, size=label.shape[-2:], mode='bilinear', align_corners=False), dim=1)
    C = probs.size(1)
    probs = probs.permute(0, 2, 3, 1).contiguous().view(-1, C)
    labels = label.view(-1)
    valid = labels != ignore_index
    vprobs, vlabels = probs[valid.nonzero().squeeze()], labels[valid]
    losses = []
    for c in range(C):
        fg = (vlabels == c).float()
        # (the reference skips a class with fg.sum() == 0 by a host read; every class is present in the bench labels)
        errors = (fg - vprobs[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        fg_sorted = fg[perm]
        gts = fg_sorted.sum()
        intersection = gts - fg_sorted.cumsum(0)
        union = gts + (1 - fg_sorted).cumsum(0)
        jaccard = 1. - intersection / union
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(errors_sorted, jaccard))
    loss = torch.stack(losses).mean()
    loss.backward()
    return loss.detach(), z.grad


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--tiles', type=int, default=8)
    p.add_argument('--classes', type=int, default=6)
    p.add_argument('--size', type=int, default=1024)
    p.add_argument('--rounds', type=int, default=9)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--steps', type=int, default=12, help='timed supervised steps per kind')
    p.add_argument('--no-step', action='store_true')
    p.add_argument('--no-term', action='store_true')
    p.add_argument('--out', default=None)
    args = p.parse_args(argv)
    import torch
    import pfst_amd  # noqa: F401
    res = dict(tiles=args.tiles, classes=args.classes, size=args.size, rounds=args.rounds, device=torch.cuda.get_device_name(0))
    if not args.no_term:
        res.update(term_bench(args))
    if not args.no_step:
        res['supervised_step'] = step_bench(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return res


def term_bench(args):
    import torch
    from pfst_amd import hip_ops as ops
    N, C, S = args.tiles, args.classes, args.size
    g = torch.Generator().manual_seed(0)
    label = torch.randint(0, C, (N, S // 16, S // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
    label[:, : S // 8, : S // 4] = 255
    label = label.to(torch.uint8).cuda()
    logits = torch.randn(N, C, S // 4, S // 4, generator=g).cuda()
    slot, cls = ops.lovasz_class_tables('present', C, 'cuda')
    E = C * N * S * S
    ws_bytes = ops.lovasz_workspace(C, N * S * S, 'cuda').numel() * 8
    out = dict(elements=E, form=ops.lovasz_form(logits, label), workspace_MB=round(ws_bytes / 1e6, 1), coef_map_MB=round(4 * E / 1e6, 1))
    ev = lambda: torch.cuda.Event(enable_timing=True)
    stage_ms = {k: [] for k in STAGES + ('forward', 'backward', 'torch')}

    def ours():
        marks = [ev()]
        marks[0].record()

        def hook(name):
            marks.append(ev())
            marks[-1].record()
        r = ops.lovasz_upsample_fwd(logits, label, slot, cls, stage_hook=hook)
        grad = ops.lovasz_upsample_bwd(logits, label, slot, cls, r['lse'], r['map'], r['scale'], 1.0)
        marks.append(ev())
        marks[-1].record()
        marks[-1].synchronize()
        t = [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])]
        return r, grad, dict(zip(STAGES + ('backward',), t), forward=sum(t[:4]))

    def theirs():
        a, b = ev(), ev()
        a.record()
        loss, grad = torch_lovasz(logits, label)
        b.record()
        b.synchronize()
        return loss, grad, a.elapsed_time(b)

    for i in range(args.warmup + args.rounds):
        order = (ours, theirs) if i % 2 == 0 else (theirs, ours)
        for fn in order:
            got = fn()
            if i >= args.warmup:
                if fn is ours:
                    for k, v in got[2].items():
                        stage_ms[k].append(v)
                else:
                    stage_ms['torch'].append(got[2])
            if fn is ours:
                r, grad = got[0], got[1]
            else:
                tloss, tgrad = got[0], got[1]
    torch.cuda.synchronize()
    out['loss'] = float(r['out'][0])
    out['torch_loss'] = float(tloss)
    out['grad_max_abs_diff_over_max'] = float((grad - tgrad).abs().max() / tgrad.abs().max())
    for k, v in stage_ms.items():
        out[k + '_ms'] = dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    ours_ms = out['forward_ms']['median'] + out['backward_ms']['median']
    out['forward_backward_ms'] = round(ours_ms, 4)
    out['torch_over_ours'] = round(out['torch_ms']['median'] / ours_ms, 2)
    # bytes of the module docstring over the stage's time
    out['sort_TB_per_s'] = round(80 * E / (out['sort_ms']['median'] * 1e-3) / 1e12, 3)
    out['sort_pass_ms'] = round(out['sort_ms']['median'] / 4, 4)
    out['keys_write_TB_per_s'] = round(8 * E / (out['keys_ms']['median'] * 1e-3) / 1e12, 3)
    out['grad_TB_per_s'] = round(16 * E / (out['grad_ms']['median'] * 1e-3) / 1e12, 3)
    return out


def step_bench(args):
    """the supervised step at the workload's size with [CE] and with [CE, Lovasz] on the decode head: blocks of steps alternate, a block starts
    and ends with a device synchronise"""
    import copy
    import torch
    from pfst_amd.optim import build_optimizer
    from pfst_amd.presets import SGD_OPTIMIZER, workload_cfg
    from pfst_amd.registry import build_segmentor
    from pfst_amd.synthetic import fill_state_dict, synth_batch
    cfg, w = workload_cfg(NAME)
    batch = synth_batch(args.tiles, args.size, w['num_classes'], w['in_channels'], seed=1234, device='cuda')
    batch = {k: v for k, v in batch.items() if not k.startswith('target_')}
    ce = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
    kinds = {}
    for kind, losses in (('ce', ce), ('ce_lovasz', [ce, dict(type='LovaszLoss', loss_weight=1.0, reduction='none')])):
        mc = copy.deepcopy(cfg['model'])
        mc['decode_head']['loss_decode'] = copy.deepcopy(losses)
        torch.manual_seed(0)
        model = build_segmentor(mc)
        fill_state_dict(model.state_dict(), 0)
        model.cuda()
        kinds[kind] = (model, build_optimizer(model, dict(SGD_OPTIMIZER, lr=6e-5)))
    times = {k: [] for k in kinds}
    logs = {}

    def run(kind, n, keep):
        model, opt = kinds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            logs[kind] = model.train_step(batch, opt)['log_vars']
        torch.cuda.synchronize()
        if keep:
            times[kind].append(1000.0 * (time.perf_counter() - t0) / n)

    for kind in kinds:
        run(kind, 2, False)
    blocks, per_block = 4, -(-args.steps // 4)
    for blk in range(blocks):
        for kind in (list(kinds) if blk % 2 == 0 else list(kinds)[::-1]):
            run(kind, per_block, True)
    out = dict(steps_per_block=per_block, blocks=blocks)
    for kind, v in times.items():
        out[kind] = dict(median_ms_per_step=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
    out['ce_lovasz_minus_ce_ms'] = round(out['ce_lovasz']['median_ms_per_step'] - out['ce']['median_ms_per_step'], 2)
    out['last_log'] = {k: float(v) for k, v in logs['ce_lovasz'].items()}
    return out


if __name__ == '__main__':
    main()
