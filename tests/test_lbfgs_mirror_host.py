"""CPU: the premises of tests/lbfgs_mirror.py, reference against reference.  The mirror follows the ORACLE's own L-BFGS driver
(cpu_ref.lbfgs_step, max_eval 26, lr 1 decayed by 0.999 per closure, on cpu_ref.closure_eval) through 125 steps of the 35x51
one-level job of test_lbfgs_update_arithmetic_teacher_forced: past a full history of 100 pairs and through 24 evictions.
The run is made once and shared; K of lbfgs_mirror is four times the worst ratio printed here, rounded up."""
import math

import numpy as np
import pytest

import lbfgs_mirror as lm
from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, levels, oracle_targets, report

STEPS = 125
H, W = 35, 51


@pytest.fixture(scope="module")
def run(vgg_weights):
    c, s = levels(H, W, 1, 1), levels(H, W, 1, 2)
    tg = oracle_targets(c, s, vgg_weights)
    x0 = cpu_ref.prepare_img((0.6 * c[0] + 0.4 * s[0]).astype(np.float32)).contiguous()
    calls = []

    def closure(flat):
        loss, g, _ = cpu_ref.closure_eval(flat.view_as(x0), tg, vgg_weights, CW, SW, TVW)
        calls.append(g.reshape(-1).clone())
        return float(loss), calls[-1].clone()

    st = cpu_ref.LbfgsState(max_eval=26)
    mirror = lm.Mirror(sabotage=True)
    x = x0.clone().reshape(-1)
    lr = 1.0
    out = []
    for k in range(STEPS):
        first = len(calls)
        xk = x.numpy().copy()
        cpu_ref.lbfgs_step(st, x, lr, closure)
        lr *= 0.999 ** (len(calls) - first)
        g_k = calls[first].numpy()                            # the step's first closure: the gradient at x_k
        step = mirror.observe(xk, x.numpy(), g_k, float(st.t))
        rec = dict(step=step, accepted=bool(st.last_accept), t=float(st.t), pairs_driver=len(st.old_dirs))
        # the direction from the driver's TRUE history (its own s = t d), in fp64, and torch's fp32 direction against it
        d_true = lm.two_loop(g_k.astype(np.float64), [v.double().numpy() for v in st.old_dirs],
                             [v.double().numpy() for v in st.old_stps], [float(r) for r in st.ro], float(st.H_diag))
        rec["mirror_vs_true"] = lm.rel_l2(step.d, d_true)
        rec["torch_vs_fp64"] = lm.rel_l2(st.d.double().numpy(), d_true)
        if mirror.evictions > 0:
            d_ro, d_gram = mirror.wrong_directions()
            SY, YY = mirror.true_inner_products()
            d_ip = lm.direction_from_inner_products(g_k.astype(np.float64), mirror.ys, mirror.ss, mirror.ro, mirror.h_diag, SY, YY)
            rec["wrong_ro"] = lm.rel_l2(d_ro, step.d)
            rec["wrong_gram"] = lm.rel_l2(d_gram, step.d)
            rec["inner_products_vs_two_loop"] = lm.rel_l2(d_ip, step.d)
        out.append(rec)
    return dict(steps=out, mirror=mirror, closures=len(calls))


def test_the_run_meets_its_conditions(run):
    """Conditions, not measurements: every step accepted, the history fills and at least 20 pairs are evicted, every kept
    pair is far from torch's 1e-10 rule - and the mirror's pair count is the driver's at every step."""
    m = run["mirror"]
    report(f"lbfgs mirror on the oracle's driver: {STEPS} steps, {run['closures']} closures, {m.evictions} evictions, "
           f"{m.dropped} dropped pairs, smallest kept y.s {m.min_ys:.3e}")
    assert all(r["accepted"] and r["t"] > 0 and math.isfinite(r["t"]) for r in run["steps"])
    assert [r["step"].pairs for r in run["steps"]] == [r["pairs_driver"] for r in run["steps"]]
    assert [r["step"].pairs for r in run["steps"]] == [min(k, lm.HISTORY) for k in range(STEPS)]
    assert m.evictions >= 20 and m.dropped == 0
    assert m.min_ys > 1e-8


def test_step_error_within_the_rounding_bound(run):
    """e_k <= 2e-5 + K rho_k at every step from the second on; prints the worst ratio K was taken from."""
    rs = run["steps"][1:]
    ratio = max((r["step"].e - lm.DIRECTION_TOL) / r["step"].rho for r in rs)
    report(f"lbfgs mirror on the oracle's driver: worst (e_k - 2e-5) / rho_k = {ratio:.3f} (K = {lm.K}); worst e_k "
           f"{max(r['step'].e for r in rs):.2e}, rho_k {min(r['step'].rho for r in rs):.1e} ... {max(r['step'].rho for r in rs):.1e}; "
           f"mirror vs the direction from the driver's true history {max(r['mirror_vs_true'] for r in rs):.2e}; "
           f"torch's fp32 direction vs the fp64 recursion {max(r['torch_vs_fp64'] for r in rs):.1e}")
    for k, r in enumerate(rs, start=2):
        assert r["step"].e <= lm.bound(r["step"].rho), (k, r["step"].e, r["step"].rho)
    # torch's own fp32 recursion is no further from the fp64 one than the project's direction tolerance
    assert max(r["torch_vs_fp64"] for r in rs) < lm.DIRECTION_TOL


def test_the_bound_discriminates(run):
    """At every post-eviction step a driver whose `ro` missed one shift, and one whose SY / YY were not moved up-left (the
    newest row and column written over the last), give a direction at least ten times the bound away; with the right SY / YY
    the inner-product form is the two-loop recursion."""
    post = [r for r in run["steps"] if "wrong_ro" in r]
    assert len(post) >= 20
    report(f"lbfgs mirror, sabotaged: smallest direction error with ro one eviction behind {min(r['wrong_ro'] for r in post):.2e}, "
           f"with unshifted SY / YY {min(r['wrong_gram'] for r in post):.2e}; largest bound there "
           f"{max(lm.bound(r['step'].rho) for r in post):.2e}; inner-product form vs two-loop "
           f"{max(r['inner_products_vs_two_loop'] for r in post):.1e}")
    for r in post:
        b = lm.bound(r["step"].rho)
        assert r["wrong_ro"] >= 10 * b, (r["step"].n_iter, r["wrong_ro"], b)
        assert r["wrong_gram"] >= 10 * b, (r["step"].n_iter, r["wrong_gram"], b)
        assert r["inner_products_vs_two_loop"] < 1e-13
