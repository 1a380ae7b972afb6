"""Restatement of the six definitions of the flow estimator in include/nst_hip.h (nst_flow_estimate has them: reduce, prolong,
gradient, linearise, sweep, driver) - written from the header, in numpy, parameterised by dtype: fp64 is the reference, fp32
(the header's order of operations, one rounding each) is the yardstick for a device bound.  Also the seeded synthetic pair
tests/test_flow_host.py (CPU) and tests/test_hip_flow.py (GPU) share.  The position rule is temporal_ref's restatement of the
warp's."""
import numpy as np

from temporal_ref import _central, _taps

MAX_SCALES = 12
DEFAULTS = dict(alpha=15.0, scales=0, warps=5, iterations=50)


# ---- reduce, prolong ----------------------------------------------------------------------------------------------------------
def _binomial(a, axis, idx):
    """sum_i k_i a[idx_i] along `axis`, the five products added in index order."""
    k = (np.array([1, 4, 6, 4, 1], a.dtype) / a.dtype.type(16))
    s = k[0] * np.take(a, idx[0], axis)
    for i in range(1, 5):
        s = s + k[i] * np.take(a, idx[i], axis)
    return s


def reduce(plane, dtype):
    a = np.asarray(plane, dtype)
    h, w = a.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    r = _binomial(a, 1, [np.clip(2 * np.arange(wc) + i - 2, 0, w - 1) for i in range(5)])       # along a row first
    return _binomial(r, 0, [np.clip(2 * np.arange(hc) + j - 2, 0, h - 1) for j in range(5)])


def prolong(coarse, h, w, dtype):
    c = np.asarray(coarse, dtype)
    _, hc, wc = c.shape
    assert (hc, wc) == ((h + 1) // 2, (w + 1) // 2)
    half, two = c.dtype.type(0.5), c.dtype.type(2)
    xa, ya = np.arange(w) >> 1, np.arange(h) >> 1
    xb, yb = np.minimum(xa + (np.arange(w) & 1), wc - 1), np.minimum(ya + (np.arange(h) & 1), hc - 1)
    r = half * (c[:, :, xa] + c[:, :, xb])
    return two * (half * (r[:, ya, :] + r[:, yb, :]))


# ---- linearise ----------------------------------------------------------------------------------------------------------------
def flip_distance(flow):
    """The smallest distance, in pixels, of any sample position p + flow(p) from a point where its inside flag flips (per axis
    the positions 0 and n - 1: inside is 0 <= position < n - 1), in fp64.  A flow that is zero everywhere reports inf: it is
    exactly zero in every precision (the coarsest scale's start), so every precision decides its flags alike."""
    flow = np.asarray(flow, np.float64)
    if not flow.any():
        return float("inf")
    _, h, w = flow.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    px, py = xx + flow[0], yy + flow[1]
    return float(min(np.abs(px).min(), np.abs(px - (w - 1)).min(), np.abs(py).min(), np.abs(py - (h - 1)).min()))


def _mix(p, y0, y1, x0, x1, tx, ty):
    top = p[y0, x0] * (1 - tx) + p[y0, x1] * tx
    bot = p[y1, x0] * (1 - tx) + p[y1, x1] * tx
    return top * (1 - ty) + bot * ty


def linearize(A, B, flow, dtype):
    """(Ix, Iy, rho) of the pair at the (2,h,w) flow."""
    A, B, flow = np.asarray(A, dtype), np.asarray(B, dtype), np.asarray(flow, dtype)
    h, w = A.shape
    u, v = flow[0], flow[1]
    fin = np.isfinite(u) & np.isfinite(v)
    u0, v0 = np.where(fin, u, 0).astype(dtype), np.where(fin, v, 0).astype(dtype)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    x0, x1, tx, inx = _taps(w, xx, u0)
    y0, y1, ty, iny = _taps(h, yy, v0)
    Bx, By = _central(B)
    inside = inx & iny & fin
    Bw, Ix, Iy = (_mix(p, y0, y1, x0, x1, tx, ty) for p in (B, Bx, By))
    rho = ((Bw - Ix * u0) - Iy * v0) - A
    zero = np.zeros_like(A)
    return np.where(inside, Ix, zero), np.where(inside, Iy, zero), np.where(inside, rho, zero)


# ---- sweep --------------------------------------------------------------------------------------------------------------------
def _mean(p):
    q = np.pad(p, 1, mode="edge")
    cross = ((q[:-2, 1:-1] + q[2:, 1:-1]) + q[1:-1, :-2]) + q[1:-1, 2:]          # N + S + W + E
    diag = ((q[:-2, :-2] + q[:-2, 2:]) + q[2:, :-2]) + q[2:, 2:]                  # NW + NE + SW + SE
    return cross / p.dtype.type(6) + diag / p.dtype.type(12)


def sweeps(Ix, Iy, rho, flow, alpha, n, dtype):
    """n Jacobi steps from the (2,h,w) flow."""
    Ix, Iy, rho, flow = (np.asarray(a, dtype) for a in (Ix, Iy, rho, flow))
    a = np.dtype(dtype).type(alpha)
    den = ((a * a) + Ix * Ix) + Iy * Iy
    u, v = flow[0], flow[1]
    for _ in range(n):
        um, vm = _mean(u), _mean(v)
        t = ((rho + Ix * um) + Iy * vm) / den
        u, v = um - Ix * t, vm - Iy * t
    return np.stack([u, v])


# ---- driver -------------------------------------------------------------------------------------------------------------------
def scales_used(h, w, scales):
    limit = MAX_SCALES if scales == 0 else scales
    n = 1
    while n < limit:
        h, w = (h + 1) // 2, (w + 1) // 2
        if min(h, w) < 8:
            break
        n += 1
    return n


def estimate(A, B, dtype, alpha=15.0, scales=0, warps=5, iterations=50):
    """(flow (2,h,w), pyramid scales used, smallest flip_distance over the linearise steps)."""
    pa, pb = [np.asarray(A, dtype)], [np.asarray(B, dtype)]
    for _ in range(1, scales_used(*pa[0].shape, scales)):
        pa.append(reduce(pa[-1], dtype))
        pb.append(reduce(pb[-1], dtype))
    flow = np.zeros((2,) + pa[-1].shape, dtype)
    near = float("inf")
    for s in range(len(pa) - 1, -1, -1):
        for _ in range(warps):
            near = min(near, flip_distance(flow))
            Ix, Iy, rho = linearize(pa[s], pb[s], flow, dtype)
            flow = sweeps(Ix, Iy, rho, flow, alpha, iterations, dtype)
        if s > 0:
            flow = prolong(flow, *pa[s - 1].shape, dtype)
    return flow, len(pa), near


def endpoint_error(flow, t):
    """Mean endpoint error of a (2,h,w) flow against the constant (tx, ty), in pixels."""
    f = np.asarray(flow, np.float64)
    return float(np.sqrt((f[0] - t[0]) ** 2 + (f[1] - t[1]) ** 2).mean())


# ---- the synthetic pair -------------------------------------------------------------------------------------------------------
PAD = 16
# (h, w), true flow (tx, ty), seed: the pairs of the host test and of the GPU pipeline test.  The first pair's seed is picked
# (by the fp64 restatement alone) among 600: its true flow has the integer component ty = 2.0 (1.0 at scale 1), which puts the
# samples of row h - 3 on row h - 1 - an inside-flag flip - to within the estimate's error, and on most seeds some column of
# that row comes within 1e-3 px of it in one of the linearise steps (tests/test_flow_host.py asserts that none does).
PAIRS = (((48, 64), (-3.25, 2.0), 3490), ((33, 47), (1.5, 0.5), 2013))


def _octave(rng, h, w, doublings):
    """White noise on a grid 2^doublings coarser, replicated 2x and binomial-smoothed `doublings` times: structure at
    2^doublings pixels."""
    a = rng.uniform(-1.0, 1.0, ((h >> doublings) + 2, (w >> doublings) + 2))
    for _ in range(doublings):
        a = np.kron(a, np.ones((2, 2)))
        n, m = a.shape
        a = _binomial(a, 1, [np.clip(np.arange(m) + i - 2, 0, m - 1) for i in range(5)])
        a = _binomial(a, 0, [np.clip(np.arange(n) + j - 2, 0, n - 1) for j in range(5)])
    return a[:h, :w]


def synthetic_pair(shape, t, seed):
    """(from, to), float32 (h,w) planes in 0 ... 255 with from(p) = to(p + t): a texture with structure at 4, 8 and 16 pixels
    on a canvas padded by PAD pixels, `to` the canvas sampled bilinearly at p - t, both frames the crop."""
    h, w = shape
    rng = np.random.RandomState(seed)
    H, W = h + 2 * PAD, w + 2 * PAD
    canvas = sum(_octave(rng, H, W, d) for d in (2, 3, 4))
    canvas = 255.0 * (canvas - canvas.min()) / (canvas.max() - canvas.min())
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x0, x1, tx, _ = _taps(W, xx, np.full((H, W), -float(t[0])))
    y0, y1, ty, _ = _taps(H, yy, np.full((H, W), -float(t[1])))
    moved = _mix(canvas, y0, y1, x0, x1, tx, ty)
    crop = (slice(PAD, PAD + h), slice(PAD, PAD + w))
    return canvas[crop].astype(np.float32), moved[crop].astype(np.float32)
