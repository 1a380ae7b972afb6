"""The relaxed EMD term (nst_level_set_remd in include/nst_hip.h has the definition) restated in torch: samples, cosines,
matches, and the value at given matches.  It works in any dtype and the value is differentiable in the image map: in float64
it is the reference, in float32 the yardstick the device's errors are held to."""
import torch

EPS = 1e-5


def samples(f, stride):
    """(count, C) rows: the pixels (a s, b s) of a (1,C,h,w) map in row-major order."""
    c = f.shape[1]
    return f[0, :, ::stride, ::stride].permute(1, 2, 0).reshape(-1, c)


def counts(h, w, stride):
    return ((h - 1) // stride + 1) * ((w - 1) // stride + 1)


def rnorm(v, eps=EPS):
    """1 / sqrt(|V_k|^2 + eps) per row."""
    return 1.0 / torch.sqrt((v * v).sum(dim=1) + eps)


def cosines(f, fs, si=1, ss=1, eps=EPS):
    """(n, m): c(i, j) = <X_i, Y_j> rp_i rq_j in f's dtype."""
    x, y = samples(f, si), samples(fs, ss)
    return (x @ y.t()) * rnorm(x, eps)[:, None] * rnorm(y, eps)[None, :]


def matches(cos):
    """(nnA (n,), nnB (m,)): the lowest index among the maxima of every row and of every column."""
    # (torch.argmax documents the first maximal index; stated here once more so that the rule does not hang on it)
    big_rows = cos == cos.max(dim=1, keepdim=True).values
    big_cols = cos == cos.max(dim=0, keepdim=True).values
    return big_rows.int().argmax(dim=1), big_cols.int().argmax(dim=0)


def sides(f, fs, nnA, nnB, si=1, ss=1, eps=EPS):
    """(rA, rB, a (n,), b (m,)) at the given matches, differentiable in f."""
    x, y = samples(f, si), samples(fs, ss)
    rp, rq = rnorm(x, eps), rnorm(y, eps)
    ja, ib = nnA.reshape(-1).long(), nnB.reshape(-1).long()
    a = (x * y[ja]).sum(dim=1) * rp * rq[ja]
    b = (x[ib] * y).sum(dim=1) * rp[ib] * rq
    return 1.0 - a.mean(), 1.0 - b.mean(), a, b


def value(f, fs, nnA, nnB, si=1, ss=1, eps=EPS, side=-1):
    """(remd, side, rA, rB): the active side is A (0) when rA >= rB, else B (1); side = 0 / 1 forces it."""
    rA, rB, _, _ = sides(f, fs, nnA, nnB, si, ss, eps)
    if side < 0:
        side = 0 if float(rA.detach()) >= float(rB.detach()) else 1
    return (rB if side else rA), side, rA, rB
