"""An L-BFGS run followed from outside (test_lbfgs_mirror_host.py, test_hip_lbfgs_history.py).

The driver (nst_opt.cpp) shows x, nst_step_info and - because the closure is bitwise reproducible - the gradient at every
x_k, which a second engine evaluates.  From those alone the mirror keeps torch's curvature history (torch:optim/lbfgs.py:
396-442) in fp64 from fp32 data:
    y = g_k - g_{k-1}   the fp32 difference, as sub_kernel forms it
    s = x_k - x_{k-1}   the OBSERVED move: the driver's own s = t d is not observable, and x + t d stored in fp32 differs
                        from it by half an ulp of x per pixel
    ro = 1 / (y.s),  H = y.s / y.y
under torch's rules: a pair is kept only if y.s > 1e-10, the oldest pair is popped at 100, the history is reset at
n_iter == 1.  The direction it expects is the two-loop recursion in fp64 (as in test_lbfgs_direction_from_an_oracle_state).
Per step it reports
    e_k   = |(x_{k+1} - x_k) - t d_mirror| / |t d_mirror|     the step error (rel-L2)
    rho_k = |ulp(x_{k+1}) / 2| / |x_{k+1} - x_k|              what storing x + t d in fp32 costs (L2 norms; np.spacing)
and the bound the tests hold a driver to is e_k <= DIRECTION_TOL + K * rho_k.

Plain helper module; the premises it relies on are held by test_lbfgs_mirror_host.py (the mirror on the oracle's own driver,
and two deliberately wrong mirrors that the bound must tell apart)."""
import math

import numpy as np

HISTORY = 100                 # torch's history_size, nst_opt's `history`
CURVATURE_GUARD = 1e-10       # torch:optim/lbfgs.py:400
DIRECTION_TOL = 2e-5          # the project's direction tolerance (test_lbfgs_direction_from_an_oracle_state)
# K: the mirror on the oracle's own driver (cpu_ref.lbfgs_step, 125 steps of the 35x51 job, reference against reference;
# test_lbfgs_mirror_host.py prints the figure): the worst (e_k - DIRECTION_TOL) / rho_k over the run was 0.729.  Times 4 - the
# device walks another trajectory through the same landscape - and rounded up.  profiles/lbfgs_full_history.txt.
MEASURED_WORST_RATIO = 0.729
K = 3


def bound(rho):
    return DIRECTION_TOL + K * rho


def _f64(a):
    return np.asarray(a, dtype=np.float32).reshape(-1).astype(np.float64)


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rounding_scale(x_next, move):
    """rho: the L2 norm of half an ulp of every stored pixel over the L2 norm of the move."""
    half_ulp = 0.5 * np.spacing(np.abs(np.asarray(x_next, dtype=np.float32).reshape(-1))).astype(np.float64)
    return float(np.linalg.norm(half_ulp) / max(np.linalg.norm(move), 1e-300))


def two_loop(g, ys, ss, ro, h_diag):
    """d = -H g, torch:optim/lbfgs.py:444-460 in fp64; oldest pair first."""
    m = len(ys)
    q = -g
    al = [0.0] * m
    for i in range(m - 1, -1, -1):
        al[i] = float(ss[i].dot(q)) * ro[i]
        q = q - al[i] * ys[i]
    r = q * h_diag
    for i in range(m):
        be = float(ys[i].dot(r)) * ro[i]
        r = r + (al[i] - be) * ss[i]
    return r


def direction_from_inner_products(g, ys, ss, ro, h_diag, SY, YY):
    """nst_opt.cpp's direction_coefficients restated in fp64: the same recurrences on SY[i][j] = s_i.y_j and
    YY[i][j] = y_i.y_j (row-major, any leading dimension >= m), then d = H q0 + sum_j coef_j y_j + coef_{m+j} s_j."""
    m = len(ys)
    q0 = -g
    sq = [float(s.dot(q0)) for s in ss]
    yq = [float(y.dot(q0)) for y in ys]
    al, be = [0.0] * m, [0.0] * m
    for i in range(m - 1, -1, -1):
        v = sq[i]
        for j in range(i + 1, m):
            v -= al[j] * SY[i, j]
        al[i] = ro[i] * v
    for i in range(m):
        t = yq[i]
        for j in range(m):
            t -= al[j] * YY[j, i]
        v = h_diag * t
        for j in range(i):
            v += (al[j] - be[j]) * SY[j, i]
        be[i] = ro[i] * v
    d = h_diag * q0
    for j in range(m):
        d = d + (-h_diag * al[j]) * ys[j] + (al[j] - be[j]) * ss[j]
    return d


class Step:
    """What the mirror says about one observed step."""
    __slots__ = ("n_iter", "pairs", "kept", "evicted", "ys", "d", "e", "rho", "move")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class Mirror:
    """`sabotage=True` also keeps what two wrong drivers would hold: `ro` never shifted at one eviction (every entry one
    pair too old), and SY / YY that are not moved up-left when the oldest pair leaves, the newest row and column written
    over the last (see wrong_directions)."""

    def __init__(self, sabotage=False):
        self.ys, self.ss, self.ro = [], [], []
        self.h_diag = 1.0
        self.n_iter = 0
        self.prev_x = self.prev_g = None
        self.evictions = 0
        self.min_ys = math.inf           # smallest y.s of a kept pair
        self.dropped = 0
        self.sabotage = sabotage
        self.evicted_ro = None           # ro of the pair that left last
        self.SY_bad = np.zeros((HISTORY, HISTORY))
        self.YY_bad = np.zeros((HISTORY, HISTORY))

    @property
    def pairs(self):
        return len(self.ys)

    def _push(self, y, s, ys_dot):
        evicted = False
        if len(self.ys) == HISTORY:
            self.ys.pop(0); self.ss.pop(0)
            self.evicted_ro = self.ro.pop(0)
            self.evictions += 1
            evicted = True                                   # (SY_bad / YY_bad stay where they are: the sabotage)
        self.ys.append(y); self.ss.append(s); self.ro.append(1.0 / ys_dot)
        self.h_diag = ys_dot / float(y.dot(y))
        self.min_ys = min(self.min_ys, ys_dot)
        if self.sabotage:
            k = len(self.ys) - 1
            for j in range(k + 1):
                self.SY_bad[k, j] = float(s.dot(self.ys[j]))
                self.SY_bad[j, k] = float(self.ss[j].dot(y))
                self.YY_bad[k, j] = self.YY_bad[j, k] = float(y.dot(self.ys[j]))
        return evicted

    def direction(self, x_k, g32):
        """The direction torch's rules give at x_k with gradient g32 (fp32): updates the history first, as the driver does
        at the start of its step.  Returns (d in fp64, pair kept, pair evicted, y.s or None)."""
        x = _f64(x_k)
        g32 = np.asarray(g32, dtype=np.float32).reshape(-1)
        self.n_iter += 1
        kept = evicted = False
        ys_dot = None
        if self.n_iter == 1:
            self.ys, self.ss, self.ro = [], [], []
            self.h_diag = 1.0
            d = -g32.astype(np.float64)
        else:
            y = (g32 - self.prev_g).astype(np.float64)       # rounded to fp32 first, as sub_kernel stores it
            s = x - self.prev_x
            ys_dot = float(y.dot(s))
            if ys_dot > CURVATURE_GUARD:
                evicted = self._push(y, s, ys_dot)
                kept = True
            else:
                self.dropped += 1
            d = two_loop(g32.astype(np.float64), self.ys, self.ss, self.ro, self.h_diag)
        self.prev_x, self.prev_g = x, g32.copy()
        return d, kept, evicted, ys_dot

    def observe(self, x_k, x_next, g32, t):
        """One step of the followed run: the image before and after, the closure's fp32 gradient at x_k, info.t."""
        d, kept, evicted, ys_dot = self.direction(x_k, g32)
        move = _f64(x_next) - _f64(x_k)
        td = float(t) * d
        return Step(n_iter=self.n_iter, pairs=self.pairs, kept=kept, evicted=evicted, ys=ys_dot, d=d,
                    e=rel_l2(move, td), rho=rounding_scale(x_next, move), move=move)

    # ---- the two wrong drivers (sabotage=True), evaluated at the gradient of the step observed last
    def true_inner_products(self):
        Y, S = np.array(self.ys), np.array(self.ss)
        return S @ Y.T, Y @ Y.T

    def wrong_directions(self):
        """(direction with `ro` one eviction behind, direction from the unshifted SY / YY); meaningful once a pair has
        been evicted."""
        g = self.prev_g.astype(np.float64)
        ro_bad = [self.evicted_ro] + self.ro[:-1]
        d_ro = two_loop(g, self.ys, self.ss, ro_bad, self.h_diag)
        d_gram = direction_from_inner_products(g, self.ys, self.ss, self.ro, self.h_diag, self.SY_bad, self.YY_bad)
        return d_ro, d_gram
