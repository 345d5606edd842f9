"""An fp64 restatement of the Lovasz-Softmax loss behind the decode head's bilinear resize (rsiseg/models/losses/lovasz_loss.py as executed),
with the tie rule of csrc/lovasz_loss.hip: descending error, equal errors by ascending pixel index (n, y, x).  Shared by the CPU and GPU tests.

Besides the loss and d loss / d logits it returns the mask of the low-resolution cells whose gradient is NOT determined at fp32 resolution.
The gradient of a pixel's error in class c is +-g_k with k its rank among the errors.  Swapping two neighbours of the sorted order changes
their g by O(1 / U^2) when both have the same foreground status, but by O(1 / U) -- the size of g itself -- when one is foreground and the
other is not.  An fp32 run (fp32 blend, fp32 softmax: errors <= 1 carry a few 1e-7 of rounding each) may order such a pair either way when
their fp64 errors differ by less than MASK_EPS = 2e-6 (16 ulp at 1).  A pixel that sits next, in a class's sorted order, to an element of
the other status within MASK_EPS is flagged; every low-resolution cell one of a flagged pixel's four bilinear taps reaches is masked (the
pixel's uncertain coefficient enters exactly those cells' gradients -- the cell whose S x S block holds the pixel is always among them)."""
import numpy as np
import torch
import torch.nn.functional as F

MASK_EPS = 2e-6
MASK_CAP = 0.05          # the tests assert that at most this fraction of the cells is masked


def lovasz_grad64(fg_sorted):
    """lovasz_loss.py:15-27 in fp64"""
    p = len(fg_sorted)
    gts = fg_sorted.sum()
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (1.0 - fg_sorted).cumsum(0)
    jac = 1.0 - inter / union
    if p > 1:
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return jac


def _tap_cells(size, lo):
    """per full-resolution row / column: the two source indices of torch's bilinear resize (align_corners=False)"""
    out = []
    for n_out, n_in in zip(size, lo):
        src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        out.append((i0, i1, src - i0))
    return out


def lovasz_oracle(logits, label, size, classes='present', per_image=False, reduction='none', class_weight=None, loss_weight=1.0,
                  ignore_index=255, mask_eps=MASK_EPS):
    """logits [N, C, h, w] (any float dtype), label uint8 / int64 [N, H, W] -> dict(loss, grad float64 [N, C, h, w], mask bool [N, h, w],
    acc_seg, bad, seg_loss {(group, class): value before the class weight})"""
    N, C, h, w = logits.shape
    H, W = size
    z = logits.detach().double().clone().requires_grad_()
    up = F.interpolate(z, size=size, mode='bilinear', align_corners=False)
    p = F.softmax(up, dim=1)
    lab = label.long().reshape(N, H, W)
    cls = list(range(C)) if classes in ('all', 'present') else list(classes)
    cw = None if class_weight is None else torch.tensor(class_weight, dtype=torch.float64)
    flagged = torch.zeros(N * H * W, dtype=torch.bool)
    groups = [[n] for n in range(N)] if per_image else [list(range(N))]
    values, seg_loss = [], {}
    for gi, imgs in enumerate(groups):
        pix = torch.cat([torch.arange(n * H * W, (n + 1) * H * W) for n in imgs])          # ascending (n, y, x)
        lg = lab.reshape(-1)[pix]
        pix = pix[lg != ignore_index]
        lg = lab.reshape(-1)[pix]
        pg = p.permute(0, 2, 3, 1).reshape(-1, C)[pix]
        losses = []
        for c in cls:
            fg = (lg == c).double()
            if classes == 'present' and float(fg.sum()) == 0:
                continue
            if len(pix) == 0:
                losses.append(z.sum() * 0.0)
                continue
            err = (fg - pg[:, c]).abs()
            es, perm = torch.sort(err, dim=0, descending=True, stable=True)
            fs = fg[perm]
            val = torch.dot(es, lovasz_grad64(fs))
            seg_loss[(gi, c)] = float(val.detach())
            losses.append(val * (cw[c] if cw is not None else 1.0))
            ed = es.detach()
            near = ((ed[:-1] - ed[1:]).abs() < mask_eps) & (fs[:-1] != fs[1:])
            hit = torch.zeros(len(perm), dtype=torch.bool)
            hit[:-1] |= near
            hit[1:] |= near
            flagged[pix[perm[hit]]] = True
        values.append(torch.stack(losses).mean() if losses else z.sum() * 0.0)
    vals = torch.stack(values)
    if per_image:
        loss = vals.sum() if reduction == 'sum' else vals.mean()
    else:
        loss = vals[0]
    loss = loss_weight * loss
    loss.backward()
    # flagged pixels -> the cells their taps reach
    (y0, y1, _), (x0, x1, _) = _tap_cells(size, (h, w))
    mask = torch.zeros(N, h, w, dtype=torch.bool)
    fl = flagged.reshape(N, H, W).numpy()
    for n, yy, xx in zip(*np.nonzero(fl)):
        for a in (y0[yy], y1[yy]):
            for b in (x0[xx], x1[xx]):
                mask[n, a, b] = True
    ok = (lab != ignore_index) & (lab < C)
    arg = up.detach().argmax(1)
    eps = float(np.finfo(np.float32).eps)
    acc = (float((arg[ok] == lab[ok]).sum()) + eps) * 100.0 / (float(ok.sum()) + eps)
    bad = int(((lab != ignore_index) & (lab >= C)).sum())
    return dict(loss=float(loss.detach()), grad=z.grad.clone(), mask=mask, acc_seg=acc, bad=bad, seg_loss=seg_loss,
                flagged=int(flagged.sum()))


def link_ratio(got, ref, keep=None):
    """max over the (kept) elements of |got - ref| / (1e-4 max|ref| + 1e-3 |ref|): within the per-link bound iff <= 1 (the form of
    tests/test_dice_loss_gpu.py); max|ref| is taken over ALL elements"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    r = (got - ref).abs() / (1e-4 * ref.abs().max() + 1e-3 * ref.abs())
    if keep is not None:
        r = r[keep.expand_as(r)]
    return float(r.max()) if r.numel() else 0.0


def closed_form_uniform(label, C, ignore_index=255):
    """all logits zero: every p = 1/C, so class c's errors are 1 - 1/C on its G foreground pixels (all ranked first) and 1/C on the other
    P - G valid pixels.  sum_k e_k g_k = (1 - 1/C) J_G + (1/C) (J_P - J_G) with J_G = 1 - 0/G = 1 (G > 0) and J_P = 1:
    loss_c = 1 - 1/C for a present class, whatever the tie order; the 'present' mean over the classes is 1 - 1/C as well."""
    lab = label.long().reshape(-1)
    present = [c for c in range(C) if int((lab[lab != ignore_index] == c).sum()) > 0]
    return (1.0 - 1.0 / C) if present else 0.0
