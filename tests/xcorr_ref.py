"""The long-range style term, xcorr (nst_level_set_xcorr in include/nst_hip.h has the definition), restated in torch from the
definition: the Gram matrix of a map against its shifted copy, the per-map value, and the closed-form gradient.  It works in
any dtype and the value is differentiable in the image map: in float64 it is the reference, in float32 the yardstick the
device's errors are held to."""
import torch


def matrix(f, d):
    """G_d (C, C) of a (1,C,h,w) map for the shift d = (dx, dy): G_d[c][e] = (1/Z_d) sum_{y < h-dy, x < w-dx}
    F(y+dy, x+dx)[c] F(y, x)[e], Z_d = C (h-dy)(w-dx)."""
    dx, dy = d
    _, c, h, w = f.shape
    assert 0 <= dx < w and 0 <= dy < h and (dx, dy) != (0, 0), (d, h, w)
    a = f[0, :, dy:, dx:].reshape(c, -1)                    # F(p + d)
    b = f[0, :, :h - dy, :w - dx].reshape(c, -1)            # F(p)
    return (a @ b.t()) / float(c * (h - dy) * (w - dx))


def matrices(f, shifts):
    """(|D|, C, C): matrix(f, d) for every shift, in order."""
    return torch.stack([matrix(f, d) for d in shifts])


def value(f, gt, shifts):
    """xcorr = (1/|D|) sum_d mean_{c,e} (G_d - Gt_d)^2; gt: (|D|, C, C)."""
    total = None
    for k, d in enumerate(shifts):
        t = ((matrix(f, d) - gt[k]) ** 2).mean()
        total = t if total is None else total + t
    return total / len(shifts)


def gradient(f, gt, shifts, weight=1.0):
    """The closed form of d(weight xcorr)/dF as the header writes it: S_d = (2 weight / (|D| C^2 Z_d)) (G_d - Gt_d),
    dF(q) = sum_d ([x >= dx, y >= dy] F(q - d) S_d^T + [x < w-dx, y < h-dy] F(q + d) S_d), with F(q) a row vector."""
    _, c, h, w = f.shape
    out = torch.zeros_like(f)
    for k, (dx, dy) in enumerate(shifts):
        z = float(c * (h - dy) * (w - dx))
        s = (2.0 * weight / (len(shifts) * c * c * z)) * (matrix(f, (dx, dy)) - gt[k])
        lo = f[0, :, :h - dy, :w - dx]                      # F(q - d) for the pixels q with x >= dx, y >= dy
        hi = f[0, :, dy:, dx:]                              # F(q + d) for the pixels q with x < w-dx, y < h-dy
        # (F(q - d) S^T)[e'] = sum_e S[e'][e] F(q - d)[e];  (F(q + d) S)[e'] = sum_c F(q + d)[c] S[c][e']
        out[0, :, dy:, dx:] += torch.einsum("ab,bhw->ahw", s, lo)
        out[0, :, :h - dy, :w - dx] += torch.einsum("ca,chw->ahw", s, hi)
    return out
