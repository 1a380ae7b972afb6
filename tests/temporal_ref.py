"""fp64 restatements of the three definitions of the temporal feature in include/nst_hip.h (nst_level_set_anchor has them):
the anchor term, the bilinear warp and the flow weights - written from the header, in numpy / torch, for
tests/test_hip_temporal.py (GPU) and tests/test_temporal_host.py (CPU).  Also the synthetic flow pair both use."""
import numpy as np
import torch


# ---- the anchor term --------------------------------------------------------------------------------------------------------
def anchor_term(y, a, c):
    """tmp = sum_{ch,p} c(p) (y - a)^2 / (C h w) of (1,C,h,w) tensors and an (h,w) plane (None: ones), in y's dtype."""
    d = y - a
    sq = d * d if c is None else c.to(y.dtype) * d * d
    return sq.sum() / y.numel()


def anchor_piece(y, a, c, dtype):
    """(value, gradient) of the term by autograd in `dtype`."""
    y = y.detach().to(dtype).clone().requires_grad_(True)
    v = anchor_term(y, a.to(dtype), c)
    v.backward()
    return float(v.detach()), y.grad.detach()


# ---- the position rule, the warp ------------------------------------------------------------------------------------------------
def _taps(n, idx, d):
    """Per axis: integer part and fraction of the displacement alone; (first tap, second tap, both clamped; fraction; both
    taps inside before clamping).  d: float64, finite."""
    f = np.floor(d)
    t = d - f                                   # exact in fp64 for an fp32 d
    a = idx + np.clip(f, -(n + 1), n + 1).astype(np.int64)      # (beyond the image on either side every tap clamps to the border)
    b = a + 1
    inside = (a >= 0) & (b <= n - 1)
    return np.clip(a, 0, n - 1), np.clip(b, 0, n - 1), t, inside


def sample(planes, dx, dy):
    """planes (C,h,w) sampled bilinearly at (x + dx, y + dy), all in fp64; returns (out (C,h,w), valid (h,w) bool).  A
    non-finite displacement: the pixel itself, not valid."""
    planes = np.asarray(planes, np.float64)
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    _, h, w = planes.shape
    fin = np.isfinite(dx) & np.isfinite(dy)
    dx0, dy0 = np.where(fin, dx, 0.0), np.where(fin, dy, 0.0)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x0, x1, tx, inx = _taps(w, xx, dx0)
    y0, y1, ty, iny = _taps(h, yy, dy0)
    top = planes[:, y0, x0] * (1 - tx) + planes[:, y0, x1] * tx
    bot = planes[:, y1, x0] * (1 - tx) + planes[:, y1, x1] * tx
    out = top * (1 - ty) + bot * ty
    out = np.where(fin[None], out, planes)
    return out, inx & iny & fin


# ---- the flow weights -----------------------------------------------------------------------------------------------------------
def _central(f):
    """(d/dx, d/dy) of an (h,w) plane: 0.5 (f(x+1) - f(x-1)) with replicated borders."""
    px = np.pad(f, ((0, 0), (1, 1)), mode="edge")
    py = np.pad(f, ((1, 1), (0, 0)), mode="edge")
    return 0.5 * (px[:, 2:] - px[:, :-2]), 0.5 * (py[2:, :] - py[:-2, :])


def flow_weights(fwd, bwd):
    """The plane c of Ruder et al. section 4 in fp64 from (2,h,w) fp32 flows, and the relative margins |lhs - rhs| / rhs of
    its two inequalities (disocclusion, motion boundary)."""
    fwd, bwd = np.asarray(fwd, np.float64), np.asarray(bwd, np.float64)
    bu, bv = bwd[0], bwd[1]
    wt, valid = sample(fwd, bu, bv)
    wu, wv = wt[0], wt[1]
    bb = bu * bu + bv * bv
    lhs1 = (wu + bu) ** 2 + (wv + bv) ** 2
    rhs1 = 0.01 * ((wu * wu + wv * wv) + bb) + 0.5
    ux, uy = _central(bu)
    vx, vy = _central(bv)
    lhs2 = (ux * ux + uy * uy) + (vx * vx + vy * vy)
    rhs2 = 0.01 * bb + 0.002
    c = valid & (lhs1 <= rhs1) & (lhs2 <= rhs2)
    return c.astype(np.float64), np.abs(lhs1 - rhs1) / rhs1, np.abs(lhs2 - rhs2) / rhs2


FLOW_H, FLOW_W, FLOW_SEED = 48, 64, 20161


def synthetic_flow_pair(h=FLOW_H, w=FLOW_W, seed=FLOW_SEED):
    """A global translation by (1.5, 0.5) pixels per frame with a 16 x 20 rectangle that moves by (6, 2) and uncovers
    background, plus 0.01-pixel noise: (fwd, bwd), (2,h,w) float32 each.  fwd lives on frame i-1 (the rectangle at rows
    14..29, columns 20..39), bwd on frame i (the rectangle moved)."""
    rng = np.random.RandomState(seed)
    fwd = np.empty((2, h, w), np.float32)
    bwd = np.empty((2, h, w), np.float32)
    fwd[0], fwd[1] = 1.5, 0.5
    bwd[0], bwd[1] = -1.5, -0.5
    fwd[:, 14:30, 20:40] = np.array([6.0, 2.0], np.float32)[:, None, None]
    bwd[:, 16:32, 26:46] = np.array([-6.0, -2.0], np.float32)[:, None, None]
    fwd += rng.uniform(-0.01, 0.01, fwd.shape).astype(np.float32)
    bwd += rng.uniform(-0.01, 0.01, bwd.shape).astype(np.float32)
    return fwd, bwd


def flow_caps(c, m1, m2, margin=1e-4):
    """(share of pixels left out for a margin below `margin` in either inequality, share of zeros, share of ones)."""
    out = (m1 <= margin) | (m2 <= margin)
    return float(out.mean()), float((c == 0).mean()), float((c == 1).mean())


def bicubic_half64(x):
    """F.interpolate(x, size=(h//2, w//2), mode='bicubic') in fp64: the closure's down-sampling, differentiable."""
    h, w = x.shape[-2:]
    return torch.nn.functional.interpolate(x, size=(h // 2, w // 2), mode="bicubic", align_corners=False)
