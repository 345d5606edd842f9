"""fp64 restatement of HRNet's exchange unit (backbones/hrnet.py:199-213) for the kernel tests of csrc/hrnet.hip, with the error bound of the
fp32 kernel derived from its roundings.  CPU torch only.

    out = relu(sum_j t_j),  t_j = x_j * sc_j + sh_j on the output grid, or its bilinear (align_corners=False) interpolation from a coarser grid

Bound of the forward (no free constant): 2^-24 times the magnitude of what is rounded, once per rounding on the path --
  * a tabled operand: the normalisation's two roundings (the table's product and the fused multiply-add) of values of magnitude at most
    A_j = max |normalised plane|;
  * a coarser operand: the blend's four roundings (two products, two fused multiply-adds), each of a value of magnitude at most A_j.  The scales
    1/2, 1/4, 1/8 are exact, so the tap weights carry no error of their own;
  * add number k (k = 1 .. B-1): one rounding of a partial sum of magnitude at most A_0 + ... + A_k.
The ReLU rounds nothing."""
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24


def fuse_fp64(ops, coefs, out_hw):
    """ops: fp32 CPU tensors [N, C, h_j, w_j] in branch order; coefs: [C, 4] tables (mean, invstd, sc, sh) or None -> (out fp64, bound fp64 [N, C, 1, 1])"""
    total = bound = partial = None
    for j, (x, coef) in enumerate(zip(ops, coefs)):
        t = x.double()
        roundings = 0
        if coef is not None:
            c = coef.double().cpu()
            t = t * c[:, 2].view(1, -1, 1, 1) + c[:, 3].view(1, -1, 1, 1)
            roundings += 2
        A = t.abs().amax((2, 3), keepdim=True)
        if tuple(t.shape[2:]) != tuple(out_hw):
            t = F.interpolate(t, size=tuple(out_hw), mode='bilinear', align_corners=False)
            roundings += 4
        if j == 0:
            total, partial, bound = t, A, U24 * A * roundings
        else:
            total, partial = total + t, partial + A
            bound = bound + U24 * A * roundings + U24 * partial
    return torch.relu(total), bound


def fuse_bwd_fp64(d_out, out, coarse_hws):
    """-> (gy fp64, [resize^T(gy) on every coarse grid] fp64)"""
    gy = torch.where(out.double() > 0, d_out.double(), torch.zeros((), dtype=torch.float64))
    grads = []
    for hw in coarse_hws:
        src = torch.zeros(gy.shape[:2] + tuple(hw), dtype=torch.float64, requires_grad=True)
        F.interpolate(src, size=tuple(gy.shape[2:]), mode='bilinear', align_corners=False).backward(gy)
        grads.append(src.grad)
    return gy, grads


# ---- what tests/golden/hrnet.npz keeps of a large tensor: make_golden_hrnet.py and tests/test_hrnet_gpu.py share this rule
KEEP_GRAD, KEEP_MAP = 448, 4096


def sample(t, keep):
    """a tensor of more than `keep` elements is stored as every stride-th element of its flat view, stride = ceil(numel / keep); smaller ones whole"""
    flat = t.reshape(-1)
    stride = -(-flat.numel() // keep)
    return flat[::stride] if stride > 1 else flat
