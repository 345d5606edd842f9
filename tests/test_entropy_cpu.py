"""The self-training baselines without a device: the fp64 EntropyLoss oracle against the executed reference (tests/golden/entropy_loss.npz,
written by tests/golden/make_golden_entropy.py), the two registered types (EntropyLoss, DACS), their refusals, the DACS preset and the
`--uda dacs` front end.

Oracle against the reference's own fp32: the loss within 1e-6 relative, the gradient within the per-link bound 1e-4 max|ref| + 1e-3 |ref|
(DESIGN section 7).  Measured over the ten goldens: the loss at most 1.5e-7 relative, the gradient always inside the bound (the largest
|fp32 - fp64| is 3e-10 where max|ref| is 3e-3) -- no case needed a wider bound."""
import os
import sys

import numpy as np
import pytest

from entropy_oracle import WEIGHT_KEYS, entropy_loss, per_link_excess
from helpers import model_cfg, uda_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
# configs/_base_/uda/dacs.py:7-22, literally
REF_DACS = dict(
    type='DACS', alpha=0.99, pseudo_threshold=0.968, pseudo_weight_ignore_top=0, pseudo_weight_ignore_bottom=0,
    imnet_feature_dist_lambda=0, imnet_feature_dist_classes=None, imnet_feature_dist_scale_min_ratio=None, mix='class', blur=True,
    color_jitter_strength=0.2, color_jitter_probability=0.2, debug_img_interval=1000, print_grad_magnitude=False)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'entropy_loss.npz'))


def dacs_cfg(**over):
    return dict(REF_DACS, model=model_cfg(), max_iters=40000, **over)        # what build_train_model hands in: cfg.model, runner.max_iters


def test_oracle_reproduces_every_golden(golden):
    assert list(golden['cases']) == ['c6', 'c2', 'c11', 'c19', 'wide'] and list(golden['types']) == ['entropy', 'max_square']
    shapes = {c: golden[c + '|logits'].shape for c in golden['cases']}
    assert shapes == {'c6': (2, 6, 19, 17), 'c2': (2, 2, 5, 7), 'c11': (2, 11, 7, 9), 'c19': (2, 19, 37, 41), 'wide': (2, 6, 19, 17)}
    for case in golden['cases']:
        for t in golden['types']:
            loss, grad = entropy_loss(golden[case + '|logits'], t, float(golden[t + '|weights'][0]))
            ref_loss, ref_grad = float(golden[f'{case}|{t}|loss']), golden[f'{case}|{t}|grad']
            assert ref_grad.dtype == np.float32 and np.isfinite(ref_loss) and np.isfinite(ref_grad).all()
            rel, excess = abs(loss - ref_loss) / abs(ref_loss), per_link_excess(ref_grad, grad)
            print(f'{case} {t}: loss {loss:.9g} reference {ref_loss:.9g} rel {rel:.2e}; gradient max |fp32 - fp64| '
                  f'{np.abs(ref_grad - grad).max():.2e} of max |ref| {np.abs(grad).max():.2e}, excess over the bound {excess:.2e}')
            assert rel <= 1e-6
            assert excess <= 0
    # the wide case is what the 1e-30 is for: probabilities that are exactly 0 in fp32
    z = golden['wide|logits']
    e = np.exp(z - z.max(axis=1, keepdims=True), dtype=np.float32)
    assert int((e / e.sum(axis=1, keepdims=True) == 0).sum()) > 100
    assert int((golden['wide|entropy|grad'] == 0).sum()) > 100


def test_oracle_gradient_is_the_derivative_of_its_loss():
    """central differences in fp64 on a tiny input, both types"""
    rng = np.random.default_rng(0)
    z = rng.standard_normal((1, 3, 2, 2))
    for t in WEIGHT_KEYS:
        _, grad = entropy_loss(z, t, 0.9)
        num = np.zeros_like(z)
        for i in np.ndindex(*z.shape):
            d = np.zeros_like(z)
            d[i] = 1e-6
            num[i] = (entropy_loss(z + d, t, 0.9)[0] - entropy_loss(z - d, t, 0.9)[0]) / 2e-6
        assert np.abs(num - grad).max() <= 1e-8 * max(1.0, np.abs(grad).max()), t


def test_entropy_loss_builds_and_refuses():
    from pfst_amd.registry import LOSSES, build_loss
    a = LOSSES.build(dict(type='EntropyLoss', loss_type='entropy', weights={'loss_ent': 0.01}))
    b = build_loss(dict(type='EntropyLoss', loss_type='max_square', weights={'loss_max_square': 0.5, 'other': 1}, unused_option=3))
    assert (a.loss_name, a.key, a.weights) == ('loss_entropy', 'loss_ent', {'loss_ent': 0.01})
    assert (b.loss_name, b.key) == ('loss_max_square', 'loss_max_square')
    assert not list(a.parameters())
    with pytest.raises(ValueError, match='loss_type'):
        build_loss(dict(type='EntropyLoss', loss_type='renyi', weights={'loss_ent': 1.0}))
    for weights in (None, {'loss_max_square': 1.0}, 0.1):
        with pytest.raises(KeyError, match='loss_ent'):
            build_loss(dict(type='EntropyLoss', loss_type='entropy', weights=weights))
    with pytest.raises(KeyError, match='loss_max_square'):
        build_loss(dict(type='EntropyLoss', loss_type='max_square', weights={'loss_ent': 1.0}))


def test_c_abi_refuses_one_class_before_any_launch():
    """log2(1) = 0 is the reference's division by zero; C above the class loop's range; bad kind -- all PFST_ERR_ARG on the host"""
    from pfst_amd import _lib
    L = _lib.lib()
    p = 256          # any non-null address: refused before anything is launched
    assert L.pfst_softmax_entropy_fwd(p, 2, 1, 64, 0, 0, 1.0, p, p, None) == -1
    assert b'C >= 2' in L.pfst_last_error() and b'entropy_loss.hip' in L.pfst_last_error()
    assert L.pfst_softmax_entropy_bwd(p, 2, 1, 64, 0, 0, 1.0, 1.0, p, 1, None) == -1
    assert b'C >= 2' in L.pfst_last_error()
    assert L.pfst_softmax_entropy_fwd(p, 2, 256, 64, 0, 0, 1.0, p, p, None) == -1
    assert L.pfst_softmax_entropy_fwd(p, 2, 6, 64, 2, 0, 1.0, p, p, None) == -1
    assert L.pfst_softmax_entropy_fwd(p, 2, 6, 64, 0, 0, 1.0, None, p, None) == -1
    assert L.pfst_softmax_entropy_bwd(p, 2, 6, 64, 0, 0, 1.0, 1.0, p, 2, None) == -1
    import ctypes
    n = ctypes.c_longlong(0)
    assert L.pfst_softmax_entropy_workspace_bytes(8, 256 * 256, ctypes.addressof(n)) == 0 and n.value == 8 * 256 * 8
    assert L.pfst_softmax_entropy_workspace_bytes(2, 1517, ctypes.addressof(n)) == 0 and n.value == 2 * 6 * 8


def test_entropy_loss_forward_has_no_host_read():
    """a reading of the path: nothing between EntropyLoss.forward and the launches brings a value to the host (the step keeps its single
    packed log read)"""
    import inspect
    from pfst_amd import hip_ops, uda
    for fn in (uda.EntropyLoss.forward, hip_ops.softmax_entropy, hip_ops.softmax_entropy_bwd_, hip_ops._entropy_args):
        src = inspect.getsource(fn)
        for word in ('.item(', '.cpu(', '.tolist(', 'synchronize', 'float(loss', '.numpy('):
            assert word not in src, (fn.__name__, word)


def test_dacs_builds_from_the_reference_values_with_pfgst_state_keys():
    from pfst_amd.registry import UDA
    dacs = UDA.build(dacs_cfg())
    assert type(dacs).__name__ == 'DACS' and not dacs.apply_aux and (dacs.alpha, dacs.pseudo_threshold) == (0.99, 0.968)
    assert hasattr(dacs, 'model') and hasattr(dacs, 'ema_model')            # what --init-student-from fills
    pf = uda_cfg()
    pf['aux_losses'] = None
    pfgst = UDA.build(pf)
    keys = list(dacs.state_dict())
    assert keys == list(pfgst.state_dict())
    assert all(k.startswith(('model.', 'ema_model.')) or k == '_extra_state' for k in keys)
    assert sum(k.startswith('model.') for k in keys) == sum(k.startswith('ema_model.') for k in keys) > 100
    assert dacs.get_extra_state() == {'local_iter': 0}
    assert not any(p.requires_grad for p in dacs.ema_model.parameters())


def test_dacs_refusals():
    from pfst_amd.registry import UDA
    with pytest.raises(NotImplementedError, match='fdist'):
        UDA.build(dacs_cfg(imnet_feature_dist_lambda=0.005))
    over = dacs_cfg()
    over['print_grad_magnitude'] = True
    with pytest.raises(NotImplementedError, match='print_grad'):
        UDA.build(over)
    with pytest.raises(NotImplementedError, match='auxiliary'):
        UDA.build(dacs_cfg(aux_losses=[dict(type='EntropyLoss', loss_type='entropy', weights={'loss_ent': 0.01})]))
    # the same refusals, the same words, as PFGST's
    pf = uda_cfg()
    pf['imnet_feature_dist_lambda'] = 0.005
    with pytest.raises(NotImplementedError, match='fdist'):
        UDA.build(pf)


def test_dacs_preset_equals_the_reference_file():
    from pfst_amd import presets
    cfg = presets.dacs_uda_cfg()
    model, max_iters = cfg.pop('model'), cfg.pop('max_iters')
    assert cfg == REF_DACS
    assert model == presets.model_cfg(6, 3, 0.1) and max_iters == 40000
    assert presets.dacs_uda_cfg(num_classes=2, pseudo_threshold=0.9)['model']['decode_head']['num_classes'] == 2


def test_train_cli_uda_dacs_rewrites_the_config():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.registry import build_train_model
    cfg = train_cli.load_cfg(train_cli.parse_args([PRESET, '--synthetic', '--uda', 'dacs', '--max-iters', '20']))
    assert {k: v for k, v in dict(cfg.uda).items()} == REF_DACS and cfg.runner['max_iters'] == 20
    model = build_train_model(cfg)
    assert type(model).__name__ == 'DACS' and model.max_iters == 20 and not model.apply_aux
    # options addressed at the new section apply to it; the data's normalisation type survives the swap
    cfg = train_cli.load_cfg(train_cli.parse_args(['pfst_season_net_sp2fa_deeplabv3plus_r50-d8', '--uda', 'dacs', '--cfg-options',
                                                   'uda.pseudo_threshold=0.9']))
    assert cfg.uda['pseudo_threshold'] == 0.9 and cfg.uda['strong_aug_denorm_type'] == 'none' and cfg.uda['type'] == 'DACS'
    with pytest.raises(ValueError, match='--uda'):
        train_cli.load_cfg(train_cli.parse_args([PRESET, '--supervised', '--uda', 'dacs']))
    with pytest.raises(SystemExit):
        train_cli.parse_args([PRESET, '--uda', 'advent'])
    # MinEnt / max-squares: PFGST with an EntropyLoss among its auxiliary losses, through --cfg-options
    opt = "uda.aux_losses=[{'type':'EntropyLoss','loss_type':'entropy','weights':{'loss_ent':0.001}}]"
    model = build_train_model(train_cli.load_cfg(train_cli.parse_args([PRESET, '--cfg-options', opt])))
    assert type(model).__name__ == 'PFGST' and [type(m).__name__ for m in model.aux_losses] == ['EntropyLoss']
    assert model.aux_losses[0].weights == {'loss_ent': 0.001}
