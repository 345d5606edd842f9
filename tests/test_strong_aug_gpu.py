"""Strong-augmentation kernels (colour jitter, gaussian blur) against a restatement of the SAME documented kornia-0.6 formulas
(kornia itself is not installed: parity with the reference's third-party arithmetic is 'unpinned'; this test pins the
kernels to the restated formulas -- the jitter to the float64 ones of tests/strong_aug_oracle.py, the blur to F.conv2d -- and checks
their invariants).  The edge cases live in tests/test_strong_aug_edges_gpu.py, the train step in tests/test_strong_aug_step_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import strong_aug_oracle as SO

pytestmark = pytest.mark.gpu
MEAN = torch.tensor([123.675, 116.28, 103.53]).view(1, 3, 1, 1)
STD = torch.tensor([58.395, 57.12, 57.375]).view(1, 3, 1, 1)


def test_color_jitter_matches_restated_formulas():
    from pfst_amd import hip_ops as ops
    g = torch.Generator().manual_seed(0)
    n, S = 3, 48
    img = torch.randn(n, 3, S, S, generator=g)
    prm = torch.tensor([[1.1, 0.9, 1.15, 0.3, 0, 1, 2, 3], [0.85, 1.2, 0.8, -0.7, 3, 2, 1, 0], [1.0, 1.0, 1.0, 0.0, 2, 0, 3, 1]])
    out = ops.color_jitter_(img.clone().cuda(), prm.cuda(), MEAN.flatten().cuda(), STD.flatten().cuda(), True).cpu()
    # the fp64 reference and the out-of-gamut bound of tests/strong_aug_oracle.py (64 x 2^-24 x 255 / std x the factors above 1 x
    # max(1, |s|)), EVERY pixel: the composed map is continuous across sector borders and hue ties, so no pixel is exempt.  (This test
    # used to let 0.2 % of the pixels be off by more than 1e-3; on the MI355X none is off by more than 4.1e-6, 0.2 of this bound.)
    ratio, ref, _ = SO.jitter_ratio(out, img, prm, True, out_of_gamut=True)
    assert float(SO.jitter_ex(img, prm)[2].max()) < 8.0, 'condition on the input: |s| stays off the singularity, the bound is not vacuous'
    print(f'colour jitter on the N(0, 1) image: {ratio:.3g} of the bound')
    err = (out.double() - ref).abs()
    assert ratio < 1.0 and float(err.median()) < 1e-5
    # identity parameters leave in-gamut pixels unchanged
    ident = torch.tensor([[1.0, 1.0, 1.0, 0.0, 0, 1, 2, 3]])
    x = (torch.rand(1, 3, S, S, generator=g) * 255.0 - MEAN) / STD
    y = ops.color_jitter_(x.clone().cuda(), ident.cuda(), MEAN.flatten().cuda(), STD.flatten().cuda(), True).cpu()
    assert float((y - x).abs().max()) < 2e-4


def test_gaussian_blur_matches_conv_reference():
    from pfst_amd import hip_ops as ops
    from pfst_amd.strong_aug import _blur_kernel_size, _gauss_taps
    g = torch.Generator().manual_seed(1)
    n, H, W = 2, 96, 128
    img = torch.randn(n, 3, H, W, generator=g)
    ky, kx = _blur_kernel_size(H), _blur_kernel_size(W)
    assert ky % 2 == 1 and kx % 2 == 1 and (ky, kx) == (9, 13)
    sig = [0.4, 1.1]
    ty = torch.stack([_gauss_taps(ky, s) for s in sig])
    tx = torch.stack([_gauss_taps(kx, s) for s in sig])
    ref = []
    for i in range(n):
        x = F.pad(img[i:i + 1], (kx // 2, kx // 2, ky // 2, ky // 2), mode='reflect')
        x = F.conv2d(x, tx[i].view(1, 1, 1, kx).repeat(3, 1, 1, 1), groups=3)
        x = F.conv2d(x, ty[i].view(1, 1, ky, 1).repeat(3, 1, 1, 1), groups=3)
        ref.append(x)
    ref = torch.cat(ref)
    out = ops.gaussian_blur(img.cuda(), ty.cuda(), tx.cuda(), reach=13).cpu()
    assert float((out - ref).abs().max()) < 1e-5
    const = ops.gaussian_blur(torch.full((1, 3, 64, 64), 2.5).cuda(), ty[:1].cuda(), tx[:1].cuda(), reach=13).cpu()
    assert float((const - 2.5).abs().max()) < 1e-6          # taps sum to one


def test_strong_aug_entry_point_respects_draws():
    from pfst_amd.strong_aug import apply_strong_aug
    x = torch.randn(2, 3, 64, 64).cuda()
    metas = [dict(img_norm_cfg=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375]))] * 2
    y = apply_strong_aug(x.clone(), metas, jitter_draw=0.1, jitter_p=0.2, jitter_s=0.2, blur_draw=0.3)
    assert torch.equal(y, x)                                  # neither draw exceeds its threshold -> untouched
    z = apply_strong_aug(x.clone(), metas, jitter_draw=0.9, jitter_p=0.2, jitter_s=0.2, blur_draw=0.9)
    assert z.shape == x.shape and bool(torch.isfinite(z).all()) and not torch.equal(z, x)
    ten = torch.randn(2, 10, 32, 32).cuda()
    assert apply_strong_aug(ten, metas, 0.9, 0.2, 0.2, 0.9) is ten   # != 3 channels: skipped like the reference
    import pytest
    with pytest.raises(ValueError, match='No such denorm type'):      # raised only when the jitter actually runs (dacs_transforms.py:69-74)
        apply_strong_aug(x.clone(), metas, 0.9, 0.2, 0.2, 0.3, denorm_type='minmax')
    assert torch.equal(apply_strong_aug(x.clone(), metas, 0.1, 0.2, 0.2, 0.3, denorm_type='minmax'), x)
    w01 = torch.rand(2, 3, 64, 64).cuda()                              # season_net: images already in [0, 1], no de-normalisation
    unit = [dict(img_norm_cfg=dict(mean=[0.0] * 3, std=[1.0] * 3, to_rgb=False))] * 2
    j = apply_strong_aug(w01.clone(), unit, 0.9, 0.2, 0.2, 0.3, denorm_type='none')
    assert bool(torch.isfinite(j).all()) and float(j.min()) >= -1e-6 and float(j.max()) <= 1.0 + 1e-6
