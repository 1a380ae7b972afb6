"""The self-similarity content term (nst_level_set_selfsim in include/nst_hip.h has the definition) restated in torch: samples,
the distance matrix with its zero diagonal and its clamp, the column-normalised matrix, the value, and the value under given
signs.  It works in any dtype and the value is differentiable in the image map: in float64 it is the reference, in float32
the yardstick the device's errors are held to."""
import torch

from remd_ref import rnorm, samples  # noqa: F401  (the sampling rule and the norms are the relaxed EMD term's)

EPS = 1e-5


def counts(h, w, stride):
    return ((h - 1) // stride + 1) * ((w - 1) // stride + 1)


def cosines(f, stride=1, eps=EPS):
    """(n, n): c(i, j) = <X_i, X_j> rp_i rp_j in f's dtype, f a (1,C,h,w) map."""
    x = samples(f, stride)
    r = rnorm(x, eps)
    return (x @ x.t()) * r[:, None] * r[None, :]


def distances(f, stride=1, eps=EPS):
    """(n, n): D_ii = 0, D_ij = max(0, 1 - c(i, j)).  A clamped entry passes no gradient (torch.clamp's rule at the bound
    differs from the device's only where 1 - c is exactly 0)."""
    c = cosines(f, stride, eps)
    d = torch.clamp(1.0 - c, min=0.0)
    return d * (1.0 - torch.eye(d.shape[0], dtype=d.dtype, device=d.device))


def clamped(f, stride=1, eps=EPS):
    """How many off-diagonal entries the clamp holds at 0."""
    c = cosines(f, stride, eps)
    off = ~torch.eye(c.shape[0], dtype=torch.bool, device=c.device)
    return int(((1.0 - c <= 0.0) & off).sum())


def normalised(d, eps=EPS):
    """N_ij = D_ij / (s_j + eps), s_j = sum_i D_ij: every column a distribution (up to eps)."""
    return d / (d.sum(dim=0, keepdim=True) + eps)


def matrices(f, stride=1, eps=EPS):
    """(D, s, N) of one map."""
    d = distances(f, stride, eps)
    return d, d.sum(dim=0), normalised(d, eps)


def value(f, fc, stride=1, eps=EPS):
    """selfsim = (1/n) sum_ij |N_ij - M_ij|, differentiable in f."""
    n_img = normalised(distances(f, stride, eps), eps)
    m = normalised(distances(fc, stride, eps), eps).detach()
    return (n_img - m).abs().sum() / n_img.shape[0]


def signs(f, fc, stride=1, eps=EPS):
    """sign(N - M), int8, and N - M itself."""
    d = normalised(distances(f, stride, eps), eps) - normalised(distances(fc, stride, eps), eps)
    return torch.sign(d).to(torch.int8), d


def value_under(f, fc, sg, stride=1, eps=EPS, live=None):
    """sum_ij sg_ij (N_ij - M_ij) / n at the given signs: its autograd is the gradient under those decisions.  `live` (n, n
    bool, optional): the entries the device's clamp lets a gradient through (its D != 0); the others are held constant."""
    d = distances(f, stride, eps)
    if live is not None:
        d = torch.where(live, d, d.detach())
    n_img = normalised(d, eps)
    m = normalised(distances(fc, stride, eps), eps).detach()
    return (sg.to(n_img.dtype) * (n_img - m)).sum() / n_img.shape[0]
