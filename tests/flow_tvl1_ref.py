"""Restatement of the TV-L1 flow estimator's definitions in include/nst_hip.h (nst_flow_tvl1_estimate) - written from the
header, in numpy, parameterised by dtype: fp64 is the reference, fp32 (the header's order of operations, one rounding each;
numpy's float32 division and square root are correctly rounded) is the yardstick for a device bound.  The pyramid, the
linearisation and the scale rule are flow_ref's restatements, imported.

Also the two-motion scenes tests/test_flow_tvl1_host.py (CPU) and tests/test_hip_flow_tvl1.py (GPU) share: a textured rectangle
that moves over a textured background that moves differently - a motion boundary, where the quadratic smoothness term of
Horn-Schunck blurs the flow.  The seeds were fixed before this generator was written and none was re-picked by its results: on
every scene the fp64 restatements put TV-L1's error at most at half of Horn-Schunck's, over the visible pixels and over the band
(tests/test_flow_tvl1_host.py has the figures)."""
import numpy as np

from flow_ref import PAD, _mix, _octave, linearize, prolong, reduce, scales_used
from temporal_ref import _taps

DEFAULTS = dict(lambda_=0.15, theta=0.3, tau=0.25, scales=0, warps=5, iterations=50)


# ---- one iteration ------------------------------------------------------------------------------------------------------------
def _back_x(p):
    """dx(p)(x) = p(x) - p(x-1) with p(-1) = 0."""
    q = np.pad(p, ((0, 0), (1, 0)))
    return q[:, 1:] - q[:, :-1]


def _back_y(p):
    q = np.pad(p, ((1, 0), (0, 0)))
    return q[1:, :] - q[:-1, :]


def _fwd_x(a):
    """a(x+1) - a(x), 0 in the last column."""
    d = np.zeros_like(a)
    d[:, :-1] = a[:, 1:] - a[:, :-1]
    return d


def _fwd_y(a):
    d = np.zeros_like(a)
    d[:-1, :] = a[1:, :] - a[:-1, :]
    return d


def read_duals(dual, dtype):
    """The (4,h,w) duals as the definitions read them: the last column of p11, p21 and the last row of p12, p22 are 0."""
    p = np.array(dual, dtype)
    p[0][:, -1] = 0
    p[2][:, -1] = 0
    p[1][-1, :] = 0
    p[3][-1, :] = 0
    return p


def iterate(Ix, Iy, rho, flow, dual, lambda_, theta, tau, n, dtype):
    """(flow (2,h,w), duals (4,h,w)) after n iterations from the flow and the duals (p11, p12, p21, p22)."""
    T = np.dtype(dtype).type
    Ix, Iy, rho, flow = (np.asarray(a, dtype) for a in (Ix, Iy, rho, flow))
    lam, theta, tau = T(lambda_), T(theta), T(tau)
    lt, taut, one, zero = lam * theta, tau / theta, T(1), T(0)
    g2 = Ix * Ix + Iy * Iy
    b = lt * g2
    has = g2 >= T(np.float32(1e-10))
    inner_den = np.where(has, g2, one)
    u, v = flow[0], flow[1]
    p11, p12, p21, p22 = read_duals(dual, dtype)
    for _ in range(n):
        r = (rho + Ix * u) + Iy * v
        k = np.where(r < -b, lt, np.where(r > b, -lt, np.where(has, (-r) / inner_den, zero))).astype(dtype)
        v1, v2 = u + k * Ix, v + k * Iy
        u = v1 + theta * (_back_x(p11) + _back_y(p12))
        v = v2 + theta * (_back_x(p21) + _back_y(p22))
        ux, uy, vx, vy = _fwd_x(u), _fwd_y(u), _fwd_x(v), _fwd_y(v)
        n1 = one + taut * np.sqrt(ux * ux + uy * uy)
        n2 = one + taut * np.sqrt(vx * vx + vy * vy)
        p11, p12 = (p11 + taut * ux) / n1, (p12 + taut * uy) / n1
        p21, p22 = (p21 + taut * vx) / n2, (p22 + taut * vy) / n2
    return np.stack([u, v]), np.stack([p11, p12, p21, p22])


# ---- driver -------------------------------------------------------------------------------------------------------------------
def estimate(A, B, dtype, lambda_=0.15, theta=0.3, tau=0.25, scales=0, warps=5, iterations=50):
    """(flow (2,h,w), pyramid scales used)."""
    pa, pb = [np.asarray(A, dtype)], [np.asarray(B, dtype)]
    for _ in range(1, scales_used(*pa[0].shape, scales)):
        pa.append(reduce(pa[-1], dtype))
        pb.append(reduce(pb[-1], dtype))
    flow = np.zeros((2,) + pa[-1].shape, dtype)
    for s in range(len(pa) - 1, -1, -1):
        dual = np.zeros((4,) + pa[s].shape, dtype)
        for _ in range(warps):
            Ix, Iy, rho = linearize(pa[s], pb[s], flow, dtype)
            flow, dual = iterate(Ix, Iy, rho, flow, dual, lambda_, theta, tau, iterations, dtype)
        if s > 0:
            flow = prolong(flow, *pa[s - 1].shape, dtype)
    return flow, len(pa)


# ---- the two-motion scenes ----------------------------------------------------------------------------------------------------
# (h, w, seed, background motion, foreground motion, rectangle y0, y1, x0, x1) - motions (tx, ty) in pixels
SCENES = ((48, 64, 11, (0.0, 0.0), (3.0, 1.0), (14, 34, 18, 44)),
          (64, 96, 5, (-1.5, 0.5), (4.0, -2.0), (16, 48, 24, 70)),
          (48, 64, 7, (1.0, 0.0), (-3.0, 1.5), (10, 36, 20, 50)))
BAND = 4          # pixels either side of the moved rectangle's edge


def _texture(rng, H, W):
    """flow_ref.synthetic_pair's canvas: structure at 4, 8 and 16 pixels, on the 0 ... 255 scale."""
    c = sum(_octave(rng, H, W, d) for d in (2, 3, 4))
    return 255.0 * (c - c.min()) / (c.max() - c.min())


def _moved(layer, t):
    """The layer moved by t = (tx, ty): sampled bilinearly at p - t (flow_ref.synthetic_pair's sampling)."""
    H, W = layer.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x0, x1, tx, _ = _taps(W, xx, np.full((H, W), -float(t[0])))
    y0, y1, ty, _ = _taps(H, yy, np.full((H, W), -float(t[1])))
    return _mix(layer, y0, y1, x0, x1, tx, ty)


def _spread(mask, r):
    """The mask grown by r pixels (a square neighbourhood)."""
    q = np.pad(mask, r)
    h, w = mask.shape
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= q[dy:dy + h, dx:dx + w]
    return out


def scene(h, w, seed, t_bg, t_fg, rect):
    """(from, to, truth (2,h,w), visible (h,w) bool, band (h,w) bool).  `to`: both layers unmoved; `from`: the background
    moved by t_bg, the foreground (and its rectangle mask, by the same sampling) by t_fg - so the true flow on the grid of
    `from`, from(p) ~ to(p + w(p)), is -t_fg inside the moved mask and -t_bg outside.  visible leaves out the pixels whose
    source lies under the foreground of `to` (background that the unmoved rectangle hides) or outside the image, and those
    where the moved mask is neither layer (a value in (0.02, 0.98)); band: the visible pixels within BAND of the moved
    rectangle's edge."""
    rng = np.random.RandomState(seed)
    H, W = h + 2 * PAD, w + 2 * PAD
    bg, fg = _texture(rng, H, W), _texture(rng, H, W)
    y0, y1, x0, x1 = rect
    mask = np.zeros((H, W))
    mask[PAD + y0: PAD + y1, PAD + x0: PAD + x1] = 1.0
    to = mask * fg + (1.0 - mask) * bg
    m = _moved(mask, t_fg)
    frm = m * _moved(fg, t_fg) + (1.0 - m) * _moved(bg, t_bg)
    crop = (slice(PAD, PAD + h), slice(PAD, PAD + w))
    m = m[crop]
    inside, outside = m >= 0.98, m <= 0.02
    truth = np.empty((2, h, w))
    for c in range(2):
        truth[c] = np.where(inside, -t_fg[c], -t_bg[c])
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sx, sy = xx + truth[0], yy + truth[1]
    in_image = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    hidden = outside & (_moved(mask, t_bg)[crop] > 0.02)           # the mask of `to` at the background's source position
    visible = (inside | outside) & in_image & ~hidden
    rect_now = m >= 0.5
    band = visible & _spread(rect_now, BAND) & _spread(~rect_now, BAND)
    return frm[crop].astype(np.float32), to[crop].astype(np.float32), truth, visible, band


def endpoint_error(flow, truth, where):
    """Mean endpoint error over the pixels `where`, in pixels."""
    f = np.asarray(flow, np.float64)
    return float(np.sqrt((f[0] - truth[0]) ** 2 + (f[1] - truth[1]) ** 2)[where].mean())
