"""The adversarial (ADVENT) baseline without a GPU: the fp64 oracle (tests/advent_oracle.py) against the executed reference
(tests/golden/advent.npz, written by tests/golden/make_golden_advent.py), the registry names, the discriminator's state-dict keys, the
two-optimizer builder, every refusal, and the `--adversarial advent` config rewriting (`--uda` keeps its one choice, which an
earlier test pins: the adversarial model is no `uda` wrapper and takes a flag of its own).

Bounds: losses within 1e-5 relative; gradients per element |a - b| <= 1e-4 max|ref| + 1e-3 |ref| (the per-link bound)."""
import os
import sys

import numpy as np
import pytest
import torch

import advent_oracle as orc
from advent_oracle import per_link_excess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'advent.npz'))


@pytest.mark.parametrize('case', orc.GOLDEN_CASES)
def test_oracle_against_the_executed_reference(golden, case):
    c = orc.golden_case(golden, case)
    dg = orc.disc_grads(c['params'], c['logits_src'], c['logits_trg'], c['weights'])
    gl = orc.gen_loss(c['params'], c['logits_trg'], c['weights'])
    for key, got in (('loss_disc_src', dg['loss_disc_src']), ('loss_disc_trg', dg['loss_disc_trg']), ('loss_gen', gl['loss_gen'])):
        ref = float(golden[f'{case}|{key}'])
        print(f'{case} {key}: oracle {got:.8g} reference {ref:.8g} rel. difference {abs(got - ref) / abs(ref):.2e}')
        assert abs(got - ref) <= 1e-5 * abs(ref)
    assert per_link_excess(golden[f'{case}|d_src'], dg['d_src'].numpy()) <= 0
    assert per_link_excess(golden[f'{case}|d_trg'], dg['d_trg'].numpy()) <= 0
    ex = per_link_excess(golden[f'{case}|grad_trg'], gl['grad'].numpy())
    print(f'{case} d loss_gen / d logits_trg: excess over the per-link bound {ex:.2e}, max |ref| {float(gl["grad"].abs().max()):.2e}')
    assert ex <= 0
    for key, g in zip(orc.KEYS, dg['grads']):
        assert per_link_excess(golden[f'{case}|dgrad|{key}'], g.numpy()) <= 0, key
    if case == 'wide':
        zeros = golden['wide|grad_trg'] == 0
        assert int(zeros.sum()) > 100
        assert float(gl['grad'].numpy()[zeros].__abs__().max()) <= 1e-4 * float(gl['grad'].abs().max())


def test_registry_resolves_the_three_names():
    from pfst_amd.registry import DISCRIMINATORS, LOSSES, SEGMENTORS
    assert SEGMENTORS.get('DomainAdaptorAdv').__name__ == 'DomainAdaptorAdv'
    assert DISCRIMINATORS.get('FCDiscriminator').__name__ == 'FCDiscriminator'
    assert LOSSES.get('AdvLoss').__name__ == 'AdvLoss'


def test_discriminator_state_dict_keys_and_default_init(golden):
    from pfst_amd.registry import build_discriminator
    torch.manual_seed(3)
    d = build_discriminator(dict(type='FCDiscriminator', num_in_channels=6, ndf=4))
    assert list(d.state_dict().keys()) == [str(k) for k in golden['keys']] == orc.KEYS
    shapes = [tuple(v.shape) for v in d.state_dict().values()]
    assert shapes == [(4, 6, 4, 4), (4,), (8, 4, 4, 4), (8,), (16, 8, 4, 4), (16,), (32, 16, 4, 4), (32,), (1, 32, 4, 4), (1,)]
    # the default nn.Conv2d initialisation, consuming the generator in the reference's order
    torch.manual_seed(3)
    ref = [torch.nn.Conv2d(a, b, 4, 2, 1) for a, b in ((6, 4), (4, 8), (8, 16), (16, 32), (32, 1))]
    for conv, r in zip(d.convs(), ref):
        assert torch.equal(conv.weight, r.weight) and torch.equal(conv.bias, r.bias)
    assert build_discriminator(dict(type='FCDiscriminator', num_in_channels=19)).net[6].weight.shape == (512, 256, 4, 4)


def adv_model_cfg(**over):
    from helpers import model_cfg
    from pfst_amd.presets import advent_cfg
    m = advent_cfg(model_cfg(num_classes=6), ndf=4)['model']
    m.update(over)
    return m


def test_segmentor_builds_with_the_reference_keys():
    from pfst_amd.registry import build_segmentor
    model = build_segmentor(adv_model_cfg())
    keys = list(model.state_dict().keys())
    assert {k.split('.')[0] for k in keys} == {'backbone', 'decode_head', 'auxiliary_head', 'discriminator'}
    assert [k for k in keys if k.startswith('discriminator.')] == ['discriminator.' + k for k in orc.KEYS]
    gen = {id(p) for p in model.generator.parameters()}
    disc = {id(p) for p in model.discriminator.parameters()}
    assert not gen & disc and len(gen) + len(disc) == len(list(model.parameters()))
    assert [id(p) for _, p in model.generator_named_parameters()] == [id(p) for p in model.generator.parameters()]
    assert not any(isinstance(m, type(model.discriminator.net[0])) for m in model.convs())      # nothing of D in the generator's repack list
    no_aux = build_segmentor(adv_model_cfg(auxiliary_head=None))                                 # the reference raises NameError here
    assert len(list(no_aux.generator)) == 2


def test_build_optimizers_and_optimizer_dict():
    from pfst_amd import optim
    from pfst_amd.presets import advent_cfg
    from pfst_amd.registry import build_segmentor
    from helpers import model_cfg
    full = advent_cfg(model_cfg(num_classes=6), ndf=4)
    model = build_segmentor(full['model'])
    assert full['optimizer']['discriminator'] == dict(type='AdamW', lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0)
    opts = optim.build_optimizers(model, full['optimizer'])
    assert isinstance(opts, optim.OptimizerDict) and list(opts) == ['generator', 'discriminator']
    groups = opts.param_groups
    assert [g['lr'] for g in groups] == [6e-5, 1e-4]
    assert groups[0] is opts['generator'].param_groups[0] and groups[1] is opts['discriminator'].param_groups[0]
    assert [id(p) for p in groups[1]['params']] == [id(p) for p in model.discriminator.parameters()]
    assert groups[1]['weight_decay'] == 0.0 and groups[1]['betas'] == (0.9, 0.99)           # AdamW without decay: Adam's update
    groups[1]['lr'] = 5e-5                                                                   # what the runner's schedule does
    assert opts['discriminator'].param_groups[0]['lr'] == 5e-5
    sd = opts.state_dict()
    assert sorted(sd) == ['discriminator', 'generator'] and sd['discriminator']['param_groups'][0]['lr'] == 5e-5
    again = optim.build_optimizers(model, full['optimizer'])
    again.load_state_dict(sd)
    assert again['discriminator'].param_groups[0]['lr'] == 5e-5 and again['generator'].param_groups[0]['lr'] == 6e-5
    with pytest.raises(KeyError, match='optimizer state'):
        again.load_state_dict(dict(generator=sd['generator']))
    opts.zero_grad()
    # a plain cfg still returns a single optimizer, through build_optimizer
    single = optim.build_optimizers(model, dict(type='AdamW', lr=6e-5, betas=(0.9, 0.999), weight_decay=0.01))
    assert isinstance(single, optim.AdamW) and not isinstance(single, dict)
    assert isinstance(optim.build_optimizers(model, dict(type='SGD', lr=0.01, momentum=0.9)), optim.SGD)
    with pytest.raises(NotImplementedError, match='AdamW'):
        optim.build_optimizers(model, dict(generator=dict(type='AdamW', lr=6e-5), discriminator=dict(type='Adam', lr=1e-4)))
    with pytest.raises(AttributeError, match='critic'):
        optim.build_optimizers(model, dict(critic=dict(type='AdamW', lr=1e-4)))


def test_refusals():
    from pfst_amd.adversarial import AdvLoss, FCDiscriminator, train_step
    from pfst_amd.registry import build_loss, build_segmentor
    with pytest.raises(NotImplementedError, match='loss_type'):
        build_loss(dict(type='AdvLoss', loss_type='adv_ent', net_type='gen', weights=dict(loss_gen=1.0)))
    with pytest.raises(NotImplementedError, match='loss_type'):
        AdvLoss(net_type='disc', weights=dict(loss_disc_src=1.0, loss_disc_trg=1.0))         # the reference's default loss_type
    with pytest.raises(ValueError, match='net_type'):
        AdvLoss(loss_type='advent', net_type='both', weights={})
    with pytest.raises(KeyError, match='loss_disc_trg'):
        AdvLoss(loss_type='advent', net_type='disc', weights=dict(loss_disc_src=1.0))
    d = FCDiscriminator(6, ndf=4)
    for shape in ((2, 6, 31, 40), (2, 6, 40, 31)):
        with pytest.raises(NotImplementedError, match='>= 32'):
            d.check_input(shape)
    d.check_input((1, 6, 32, 32))
    with pytest.raises(ValueError, match='input'):
        d.check_input((1, 5, 32, 32))
    with pytest.raises(NotImplementedError, match='neck'):
        build_segmentor(adv_model_cfg(neck=dict(type='FPN')))
    with pytest.raises(NotImplementedError, match='disc_steps'):
        build_segmentor(adv_model_cfg(train_cfg=dict(disc_steps=2)))
    model = build_segmentor(adv_model_cfg(train_cfg=dict(disc_steps=1), weight_trg=0.5))     # accepted; weight_trg ignored as in the reference
    assert model.weight_trg == 0.5
    with pytest.raises(ValueError, match='discriminator'):
        build_segmentor(adv_model_cfg(discriminator=None))
    batch = dict(img=torch.zeros(1, 3, 8, 8), img_metas=[{}], gt_semantic_seg=torch.zeros(1, 1, 8, 8, dtype=torch.long))
    with pytest.raises(KeyError, match="'target_img', 'target_img_metas'"):
        train_step(model, batch, {})
    batch.update(target_img=torch.zeros(1, 3, 8, 8), target_img_metas=[{}], extra_key=1)      # other keys are ignored
    with pytest.raises(TypeError, match='generator'):
        train_step(model, batch, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1))
    with pytest.raises(RuntimeError, match='no CPU path'):
        train_step(model, batch, dict(generator=None, discriminator=None))


def test_train_cli_adversarial_advent_rewrites_the_config():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.presets import ADVENT_DISC_OPTIMIZER, ADVENT_WEIGHTS, OPTIMIZER
    from pfst_amd.registry import build_train_model
    cfg = train_cli.load_cfg(train_cli.parse_args([PRESET, '--synthetic', '--adversarial', 'advent', '--max-iters', '20']))
    assert 'uda' not in cfg and cfg.runner['max_iters'] == 20
    assert cfg.model['type'] == 'DomainAdaptorAdv'
    assert dict(cfg.model['discriminator']) == dict(type='FCDiscriminator', num_in_channels=6, ndf=64)
    assert dict(cfg.model['gen_losses'][0]['weights']) == dict(loss_gen=0.001) == dict(loss_gen=ADVENT_WEIGHTS['loss_gen'])
    assert dict(cfg.model['disc_losses'][0]['weights']) == dict(loss_disc_src=0.5, loss_disc_trg=0.5)
    assert dict(cfg.optimizer['generator']) == OPTIMIZER and cfg.optimizer['discriminator']['lr'] == 1e-4
    model = build_train_model(cfg)
    assert type(model).__name__ == 'DomainAdaptorAdv' and model.discriminator.net[0].weight.shape == (64, 6, 4, 4)
    from pfst_amd.optim import build_optimizers
    opt = build_optimizers(model, cfg.optimizer)
    assert list(opt) == ['generator', 'discriminator']
    assert [g['lr'] for g in opt['generator'].param_groups] == [OPTIMIZER['lr']] * len(opt['generator'].param_groups)
    assert [g['lr'] for g in opt['discriminator'].param_groups] == [1e-4] * len(opt['discriminator'].param_groups)
    # options addressed at the new sections apply to them, and to them only: the sections must still BUILD (the options are first merged
    # into the config's single optimizer section, where `generator` / `discriminator` would be stray optimizer arguments)
    cfg = train_cli.load_cfg(train_cli.parse_args([PRESET, '--adversarial', 'advent', '--cfg-options', 'model.discriminator.ndf=8',
                                                   'optimizer.discriminator.lr=0.0002', 'optimizer.generator.lr=0.00003',
                                                   'optimizer.weight_decay=0.02']))
    assert cfg.model['discriminator']['ndf'] == 8 and cfg.optimizer['discriminator']['lr'] == 0.0002
    assert sorted(cfg.optimizer) == ['discriminator', 'generator']
    assert dict(cfg.optimizer['generator']) == dict(OPTIMIZER, lr=0.00003, weight_decay=0.02)     # the single section's own option stays
    assert dict(cfg.optimizer['discriminator']) == dict(ADVENT_DISC_OPTIMIZER, lr=0.0002)
    model = build_train_model(cfg)
    opt = build_optimizers(model, cfg.optimizer)
    assert model.discriminator.net[0].weight.shape == (8, 6, 4, 4)
    gen, dis = opt['generator'].param_groups, opt['discriminator'].param_groups
    assert opt.param_groups == gen + dis and len(gen) >= 1 and len(dis) >= 1
    assert all(g['lr'] == 0.00003 and g['weight_decay'] in (0.02, 0.0) for g in gen)
    assert all(g['lr'] == 0.0002 and g['weight_decay'] == 0.0 and tuple(g['betas']) == (0.9, 0.99) for g in dis)
    cfg = train_cli.load_cfg(train_cli.parse_args(['pfst_inria_da_deeplabv3plus_r50-d8', '--adversarial', 'advent']))
    assert cfg.model['discriminator']['num_in_channels'] == 2
    with pytest.raises(ValueError, match='--adversarial'):
        train_cli.load_cfg(train_cli.parse_args([PRESET, '--supervised', '--adversarial', 'advent']))
    with pytest.raises(ValueError, match='--model'):
        train_cli.load_cfg(train_cli.parse_args([PRESET, '--adversarial', 'advent', '--model', 'pspnet']))
    with pytest.raises(ValueError, match='--adversarial'):
        train_cli.load_cfg(train_cli.parse_args([PRESET, '--supervised', '--model', 'pspnet', '--adversarial', 'advent']))
    with pytest.raises(ValueError, match='--adversarial'):                 # two replacements of the one `uda` section
        train_cli.load_cfg(train_cli.parse_args([PRESET, '--uda', 'dacs', '--adversarial', 'advent']))
    with pytest.raises(SystemExit):                                        # --uda names self-training wrappers only
        train_cli.parse_args([PRESET, '--uda', 'advent'])
