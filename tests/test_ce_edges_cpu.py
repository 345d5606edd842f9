"""Conditions on the inputs of tests/test_ce_edges_gpu.py (tests/ce_oracle.py), checked on the float64 references alone: the caps that keep
that test from hiding a failure behind its exclusions.  They are conditions, not measurements: another seed or magnitude has to meet them too."""
import pytest
import torch

import ce_oracle as O

RUNS = [(name, 255) for name in O.CASES] + O.IGNORE_CASES


def test_the_table_of_cases():
    assert list(O.CASES) == ['g_up', 'g_c9', 'g_c33', 'g_down', 'g_same', 'g_x2', 'g_one', 'g_mixed', 'x4', 'x8', 'x4_c1']
    for name, (C, (h, w), (H, W), N) in O.CASES.items():
        d = O.inputs(name)
        assert d['logits'].shape == (N, C, h, w) and d['label'].shape == (N, H, W) and d['label'].dtype == torch.uint8
        assert N == (1 if name == 'x4' else 3)
    assert O.is_pow2_ratio((17, 16), (68, 64)) and O.is_pow2_ratio((10, 12), (10, 12)) and O.is_pow2_ratio((8, 6), (32, 48))
    assert not O.is_pow2_ratio((13, 9), (50, 37)) and not O.is_pow2_ratio((20, 24), (11, 15)) and not O.is_pow2_ratio((1, 1), (5, 7))
    assert not O.is_pow2_ratio((4, 4), (12, 12))


@pytest.mark.parametrize('name', list(O.CASES))
def test_label_maps_hold_what_the_cases_are_for(name):
    C, lo, (H, W), N = O.CASES[name]
    lab = O.inputs(name)['label'].long()
    assert bool((lab[:, H - 1, :] == 255).all()), 'a run of 255 along one full border row'
    assert int((lab[:, :H - 1] == 255).sum()) >= N, 'a 255 region inside'
    for n in range(N):
        assert int(((lab[n] >= C) & (lab[n] < 255)).sum()) >= 1, 'labels in [C, 255)'
        assert float((lab[n] < C).double().mean()) >= O.MIN_VALID
    assert int(((lab >= C) & (lab < C + 8)).sum()) == 0, 'the classes a padded twin adds are never labelled'
    assert float(O.inputs(name)['pw'].min()) > 0 and float(O.inputs(name)['cw'].min()) > 0


@pytest.mark.parametrize('name,ign', RUNS)
@pytest.mark.parametrize('weighted', [False, True])
def test_ce_conditions(name, ign, weighted):
    C, lo, (H, W), N = O.CASES[name]
    r = O.reference(name, weighted, ign)
    lab = r['lab']
    if ign != 255:
        assert ign < C and int((lab == ign).sum()) > 0, 'the ignored class occurs'
        assert int((r['bad'] & (lab == 255)).sum()) > 0, '255 counts as a bad label'
    assert r['n_bad'] >= 1
    assert float(r['valid'].double().mean((1, 2)).min()) >= O.MIN_VALID
    assert float(r['wp'].sum()) > 0
    share = float(r['near_tie'].double().mean())
    print(f'{name} ignore={ign}: valid pixels with a top-2 logit gap below 2 tol_z: {share:.4%}')
    assert share <= O.SHARE
    assert torch.isfinite(r['grad']).all() and float(r['grad'].abs().max()) > 0 or C == 1
    if C == 1:
        assert float(r['grad'].abs().max()) == 0.0 and r['loss'] == 0.0


@pytest.mark.parametrize('name', list(O.PSEUDO))
def test_pseudo_label_conditions(name):
    r = O.pseudo_reference(name)
    unsure = float((~r['sure']).double().mean())
    print(f'{name}: pixels with a top-2 probability gap below 2 tol_z + 8u: {unsure:.4%}')
    assert unsure <= O.SHARE
    for thr in O.THRESHOLDS:
        near = float(((r['pmax'] - thr).abs() <= r['tol_p']).double().mean())
        print(f'{name}: pixels within tol_z + 4u of the threshold {thr}: {near:.4%}')
        assert near <= O.SHARE
    if O.PSEUDO[name][0] == 1:
        assert bool((r['pmax'] == 1.0).all())
    else:
        conf = float((r['pmax'] >= 0.9).double().mean())
        assert 0.0 < conf < 1.0, 'both sides of the threshold 0.9 occur'


def test_padded_twin():
    x = O.padded_twin('g_up', 3)
    assert x.shape == (3, 9, 13, 9) and torch.equal(x[:, :6], O.inputs('g_up')['logits']) and bool((x[:, 6:] == -1e30).all())
