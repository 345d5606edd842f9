"""OHEMPixelSampler, the parts that need no GPU: configs with a sampler build (both head types, the segmentor, tools/train.py's
--cfg-options), bad options fail loudly, the C ABI of the two entry points, and the plain-torch oracle of the GPU tests (tests/ohem_oracle.py)
against the weight maps the reference's own sampler returned (tests/golden/ohem_sampler.npz, written by tests/golden/make_golden_ohem.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import ohem_oracle as O
import pfst_amd  # noqa: F401
from helpers import model_cfg
from pfst_amd.registry import build_head, build_segmentor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CE = dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0)
DICE = dict(type='DiceLoss', loss_weight=3.0)
OHEM = dict(type='OHEMPixelSampler', thresh=0.7, min_kept=100000)
N = 2


def head_cfg(which, loss_decode, **over):
    cfg = dict(model_cfg()[which], loss_decode=loss_decode)
    cfg.update(over)
    return cfg


def test_a_ce_head_with_a_sampler_builds():
    from pfst_amd.models import OHEMPixelSampler
    from pfst_amd.registry import PIXEL_SAMPLERS, build_pixel_sampler
    assert PIXEL_SAMPLERS.get('OHEMPixelSampler') is OHEMPixelSampler
    for which in ('decode_head', 'auxiliary_head'):
        head = build_head(head_cfg(which, CE, sampler=OHEM))
        assert isinstance(head.sampler, OHEMPixelSampler) and head.sampler.context is head
        assert (head.sampler.thresh, head.sampler.min_kept, head.sampler.last_info) == (0.7, 100000, None)
        assert build_head(head_cfg(which, CE)).sampler is None
    # the reference's defaults; a loss list of CE terms; the per-class coefficients the top-k mode ranks by
    cw = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
    head = build_head(head_cfg('auxiliary_head', [dict(CE, loss_weight=0.4, class_weight=cw), dict(CE, loss_weight=0.2, loss_name='loss_ce2')],
                               sampler=dict(type='OHEMPixelSampler')))
    assert (head.sampler.thresh, head.sampler.min_kept) == (None, 100000)
    assert head.sampler.coef == pytest.approx([0.4 * v + 0.2 for v in cw], rel=1e-12)
    assert isinstance(build_pixel_sampler(dict(type='OHEMPixelSampler', min_kept=2), context=head), OHEMPixelSampler)
    cfg = model_cfg()
    cfg['decode_head']['sampler'] = OHEM
    cfg['auxiliary_head']['sampler'] = dict(type='OHEMPixelSampler', min_kept=5000)
    model = build_segmentor(cfg)
    assert model.decode_head.sampler.thresh == 0.7 and model.auxiliary_head.sampler.thresh is None
    plain = build_segmentor(model_cfg())
    assert list(model.state_dict()) == list(plain.state_dict()), 'a sampler adds no parameters or buffers'
    assert len(list(model.modules())) == len(list(plain.modules())), 'the sampler is no module (its context is the head)'
    # the other refused options stay refused
    for over in (dict(align_corners=True), dict(input_transform='resize_concat'), dict(conv_cfg=dict(type='Conv2d'))):
        with pytest.raises(NotImplementedError, match='outside the PFST path'):
            build_head(head_cfg('decode_head', CE, **over))


def test_bad_sampler_options_fail_loudly():
    for min_kept in (1, 0, -5):
        with pytest.raises(AssertionError):
            build_head(head_cfg('decode_head', CE, sampler=dict(type='OHEMPixelSampler', min_kept=min_kept)))
    with pytest.raises(KeyError, match='pixel sampler'):
        build_head(head_cfg('decode_head', CE, sampler=dict(type='UniformSampler')))
    # a term that ignores pixel weights: the message names it
    for losses in ([CE, DICE], DICE, [DICE, CE]):
        with pytest.raises(NotImplementedError, match=r'DiceLoss \(loss_dice\)'):
            build_head(head_cfg('auxiliary_head', losses, sampler=OHEM))
    for bad in (dict(CE, loss_weight=-1.0), dict(CE, class_weight=[1, 1, -0.5, 1, 1, 1])):
        for sampler in (OHEM, dict(type='OHEMPixelSampler')):
            with pytest.raises(ValueError, match='negative'):
                build_head(head_cfg('decode_head', [CE, bad], sampler=sampler))
        build_head(head_cfg('decode_head', [CE, bad]))                  # without a sampler the head takes them, as before
    with pytest.raises(ValueError, match='class weights'):
        build_head(head_cfg('decode_head', dict(CE, class_weight=[1, 2, 3]), sampler=OHEM))


def test_the_entry_points_are_declared():
    import ctypes
    import re
    from pfst_amd import _lib, hip_ops
    decls = _lib.parse_header()
    text = open(_lib.HEADER).read()
    src = open(os.path.join(ROOT, 'pfst_amd', 'csrc', 'ohem.hip')).read()
    for name, nargs in {'pfst_ohem_workspace_bytes': 4, 'pfst_ohem_sample': 18}.items():
        restype, args = decls[name]
        assert restype is ctypes.c_int and len(args) == nargs, (name, len(args))
        norm = lambda s: ' '.join(re.search(name + r'\s*\(([^)]*)\)', s).group(1).split())
        assert norm(text) == norm(src[src.index('extern "C" int ' + name):]), name
        assert hasattr(_lib.lib(), name)
    kinds = dict((a, k) for k, a in decls['pfst_ohem_sample'][1])
    assert decls['pfst_ohem_sample'][1][-1] == (ctypes.c_void_p, 'stream')
    assert kinds['batch_kept'] is ctypes.c_longlong and kinds['thresh'] is ctypes.c_float and kinds['has_thresh'] is ctypes.c_int
    assert all(kinds[k] is ctypes.c_void_p for k in ('logits', 'label', 'coef', 'workspace', 'weight', 'info', 'keys_out'))
    with pytest.raises(TypeError, match='takes 18 arguments'):
        _lib.call('pfst_ohem_sample', *([0] * 17))
    nbytes = ctypes.c_longlong(0)
    _lib.call('pfst_ohem_workspace_bytes', 2, 64, 64, ctypes.addressof(nbytes))            # host only: no device is touched
    assert 0 < nbytes.value <= 1 << 20 and nbytes.value % 8 == 0
    with pytest.raises(_lib.PfstHipError):
        _lib.call('pfst_ohem_workspace_bytes', 0, 64, 64, ctypes.addressof(nbytes))
    from pfst_amd.build import NO_SLP, SOURCES
    assert 'ohem.hip' in SOURCES and 'ohem.hip' in NO_SLP and '#pragma clang fp contract(off)' in src
    with pytest.raises(RuntimeError, match='GPU only'):
        hip_ops.ohem_sample(torch.zeros(1, 2, 4, 4), torch.zeros(1, 16, 16, dtype=torch.uint8), 255, 0.7, 100)


def test_the_sampler_path_reads_nothing_on_the_host():
    """a reading of the path: no .item() / .cpu() / synchronisation between the head's losses() and the launches"""
    import inspect
    from pfst_amd import hip_ops, models
    text = inspect.getsource(models.OHEMPixelSampler.sample) + inspect.getsource(hip_ops.ohem_sample)
    src = open(os.path.join(ROOT, 'pfst_amd', 'csrc', 'ohem.hip')).read()
    for word in ('.item(', '.cpu(', '.tolist(', 'synchronize', 'float(info', 'int(info'):
        assert word not in text, word
    for word in ('hipStreamSynchronize', 'hipDeviceSynchronize', 'hipMemcpy(', 'hipMalloc', 'hipEventSynchronize'):
        assert word not in src, word


def test_cfg_options_with_a_sampler_round_trip():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import train as train_cli
    from pfst_amd.registry import build_train_model
    name = 'pfst_pots_irrg2vaih_irrg_deeplabv3plus_r50-d8'
    opt = "model.decode_head.sampler={'type':'OHEMPixelSampler','thresh':0.7,'min_kept':100000}"
    cfg = train_cli.load_cfg(train_cli.parse_args([name, '--supervised', '--cfg-options', opt]))
    model = build_train_model(cfg)
    assert (model.decode_head.sampler.thresh, model.decode_head.sampler.min_kept) == (0.7, 100000) and model.auxiliary_head.sampler is None
    uda = build_train_model(train_cli.load_cfg(train_cli.parse_args([name, '--cfg-options', opt])))
    for m in (uda.get_model(), uda.get_ema_model()):
        assert m.decode_head.sampler.thresh == 0.7 and m.decode_head.sampler.context is m.decode_head


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'ohem_sampler.npz'))


# name: (logits of, thresh, min_kept, coef)                     -- tests/golden/make_golden_ohem.py's CASES and HEADS
CW6 = [0.5, 1.0, 1.5, 2.0, 0.7, 1.2]
GOLDEN_CASES = {
    'x4r_thresh': ('x4r_thresh', 0.7, 100, None),
    'x4r_sk': ('x4r_thresh', 0.3, 1500, None),
    'x8_topk': ('x8_topk', None, 750, None),
    'g19_sk': ('g19_sk', 0.3, 1500, None),
    'head_thresh': ('x4r_thresh', 0.7, 100, None),
    'head_topk': ('x8_topk', None, 800, [0.4 * v + 0.2 for v in CW6]),
}


@pytest.mark.parametrize('name', list(GOLDEN_CASES))
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_the_oracle_reproduces_the_reference_weight_maps(golden, name, dtype):
    src, thresh, min_kept, coef = GOLDEN_CASES[name]
    logits = torch.from_numpy(golden[src + '|logits'])
    label = torch.from_numpy(golden[(src if name.startswith('head') else name) + '|label'])
    want = torch.from_numpy(np.unpackbits(golden[name + '|weight_bits'])[:label.numel()].astype(np.float32)).view(label.shape)
    key, valid = O.keys(logits, label, 255, thresh is not None, coef, dtype=dtype)
    assert int((label == 255).sum()) > 0 and torch.equal(valid, label != 255)
    if thresh is not None:
        w, cut, k = O.select_thresh(key, valid, thresh, min_kept * N)
    else:
        w, cut, k = O.select_topk(key, valid, min_kept * N)
        s = key[valid].sort(descending=True)[0]
        assert float(s[k - 1]) > float(s[k]), 'no tie at the cut'
    assert torch.equal(w, want), f'{int((w != want).sum())} pixels differ from the reference map'
    assert 0 < int(w.sum()) < int(valid.sum())
    if not name.startswith('head'):
        assert int(w.sum()) == int(golden[name + '|kept'])
        if dtype is torch.float64:
            assert cut == float(golden[name + '|cut'])
        # the fp64 band around the cut is thin (the condition of the GPU tests' comparison with this oracle)
        k64, _ = O.keys(logits, label, 255, thresh is not None, coef, dtype=torch.float64)
        c64 = float(golden[name + '|cut'])
        band = O.band_thresh(k64, valid, c64) if thresh is not None else O.band_topk(k64, valid, c64)
        assert int(band.sum()) <= O.BAND_SHARE * int(valid.sum())


def test_the_oracle_keeps_ties_in_raster_order_and_handles_empty_sets():
    key = torch.tensor([[[0.5, 2.0, 0.5, -1.0], [0.5, 3.0, 0.5, 0.5]]])
    valid = key >= 0
    w, cut, m = O.select_topk(key, valid, 4)
    assert (cut, m) == (0.5, 4) and w.flatten().tolist() == [1, 1, 1, 0, 0, 1, 0, 0]
    w, cut, m = O.select_topk(key, valid, 100)
    assert m == 7 and torch.equal(w.bool(), valid)
    none = torch.zeros_like(valid)
    assert not O.select_topk(key, none, 4)[0].any() and not O.select_thresh(key, none, 0.7, 4)[0].any()
    # strict comparison; thresh acts as its fp32 rounding
    w, thr, k = O.select_thresh(key, valid, 0.7, 1)
    assert thr == float(np.float32(0.7)) and k == 1 and w.flatten().tolist() == [1, 0, 1, 0, 1, 0, 1, 1]
    w, thr, k = O.select_thresh(key, valid, 0.1, 5)
    assert (thr, k) == (2.0, 5) and w.flatten().tolist() == [1, 0, 1, 0, 1, 0, 1, 1]
