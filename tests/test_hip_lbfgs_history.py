"""GPU: the L-BFGS driver (nst_opt.cpp) past a full history, and its vector kernels (vector_ops.hip) at the lengths where
their loops loop.

* The driver is followed from outside by tests/lbfgs_mirror.py through 125 steps of a small job on which every step is
  accepted: the history reaches its 100 pairs and the eviction branch of form_direction (erase of old_dirs / old_stps / ro,
  the two slices recycled through `spare`, the up-left shift of SY / YY, the re-uploaded pointer table) runs at every later
  step; one step in between presents y = 0, the "no new pair" branch on a full history.  The bound on the step error,
  2e-5 + K rho_k, and the two broken drivers it tells apart are the subject of tests/test_lbfgs_mirror_host.py.
* nst_lbfgs_direction, nst_adam_step and nst_scale on vectors long enough for the second pass of every fixed grid, and a
  one-level 837x839 job (n = 2106729 floats: n mod 4 = 1, 526682 16-byte vectors) through the driver, including the image
  compare of the closure reuse with single words changed in every region of its grid."""
import math

import numpy as np
import pytest
import torch

import lbfgs_mirror as lm
from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels, rel_l2, report, setup

pytestmark = pytest.mark.gpu

STEPS = 125
DROP_AFTER = 110


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def _flat(x):
    return x.detach().cpu().numpy().reshape(-1)


class Follower:
    """One optimiser followed by the mirror: per step the fields of nst_step_info that do not depend on the trajectory, and
    the mirror's step record.  `ref` is a second engine carrying the same job: it evaluates the gradient at x_k, so that the
    driver's context is left alone."""

    def __init__(self, opt, ref, x, lr):
        self.opt, self.ref, self.x = opt, ref, x
        self.mirror = lm.Mirror()
        self.lr = float(lr)
        self.total = 0
        self.steps = 0
        self.records = []

    def step(self, check_bound=True):
        xk = self.x.clone()
        g, l = self.ref.closure(xk, CW, SW, TVW)
        g_k = _flat(g)
        info, _ = self.opt.step(self.x, CW, SW, TVW)
        self.steps += 1
        k = self.steps
        # the closure is reproducible across contexts: if this fails the cause is not the optimiser
        assert _bits(info.loss) == _bits(_flat(l)[-1]), k
        for _ in range(info.closures):
            self.lr *= 0.999                                  # a double, once per closure, as the driver does
        self.total += info.closures
        assert info.total_closures == self.total, k
        assert _bits(info.lr) == _bits(np.float32(self.lr)), k
        assert info.accepted == 1 and info.t > 0 and math.isfinite(info.t), (k, info.accepted, info.t)
        rec = self.mirror.observe(_flat(xk), _flat(self.x), g_k, info.t)
        pairs, n_iter = self.opt.history()
        assert info.history == pairs == rec.pairs, (k, info.history, pairs, rec.pairs)
        assert n_iter == k
        if check_bound and k >= 2:
            assert rec.e <= lm.bound(rec.rho), (k, rec.e, rec.rho)
        self.records.append((rec, info, xk))
        return rec, info, xk


@pytest.mark.parametrize("gram", [True, False])
def test_driver_through_a_full_history_and_a_dropped_pair(vgg_weights, gram):
    """The 35x51 one-level job of test_lbfgs_update_arithmetic_teacher_forced (n = 5355, n mod 4 = 3), max_eval 26, lr 1,
    125 steps; step 111 starts from x_110 again, so its pair is y = 0 and is dropped with the history full."""
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine
    eng = StyleEngine(vgg_weights, 0, lbfgs_gram=gram)
    ref = StyleEngine(vgg_weights, 0, lbfgs_gram=gram)
    opt = None
    try:
        c, s = levels(35, 51, 1, 1), levels(35, 51, 1, 2)
        setup(eng, c, s)
        setup(ref, c, s)
        x = dev(cpu_ref.prepare_img((0.6 * c[0] + 0.4 * s[0]).astype(np.float32)).contiguous())
        opt = PixelOptimizer(eng, "lbfgs", 1.0, 26)
        bytes_start = eng.bytes()
        f = Follower(opt, ref, x, 1.0)
        for _ in range(DROP_AFTER):
            f.step()
        m = f.mirror
        assert m.pairs == lm.HISTORY and m.evictions == DROP_AFTER - 1 - lm.HISTORY and m.dropped == 0

        # ---- the dropped pair: x_110 again.  The gradient is bitwise step 110's, y = 0, the pair is dropped
        rec110, info110, x110 = f.records[-1]
        oldest = m.ys[0]
        ev0, sv0 = opt.closure_stats()
        x.copy_(x110)                                         # (the caller may write x between steps: nst_hip.h)
        rec, info, _ = f.step()
        ev1, sv1 = opt.closure_stats()
        assert info.history == lm.HISTORY
        assert not rec.kept and not rec.evicted and rec.ys == 0.0 and m.dropped == 1
        assert m.pairs == lm.HISTORY and m.ys[0] is oldest and m.evictions == DROP_AFTER - 1 - lm.HISTORY
        e_dir = lm.rel_l2(rec.move / float(info.t), rec110.move / float(info110.t))
        report(f"lbfgs history gram={gram}: dropped pair on a full history: direction vs step {DROP_AFTER}'s {e_dir:.2e} "
               f"(bound {lm.bound(rec.rho + rec110.rho):.2e}), t {info.t:.4g} vs {info110.t:.4g}")
        assert e_dir <= lm.bound(rec.rho + rec110.rho)
        # x differs from the image the optimiser remembers (x_111): the first closure was evaluated, not served
        assert sv1 == sv0 and ev1 == ev0 + info.closures

        while f.steps < STEPS:
            f.step()
        # ---- over the run: the conditions under which the above says anything
        assert all(i.accepted == 1 for _, i, _ in f.records)
        assert m.evictions >= 20
        assert m.min_ys > 1e-8
        assert [r.pairs for r, _, _ in f.records] == [min(k, lm.HISTORY) for k in range(STEPS)]
        assert eng.bytes() == bytes_start                     # the pool is recycled; nothing is allocated per step
        first_ev = next(i for i, (r, _, _) in enumerate(f.records) if r.evicted)
        pre = max(r.e / r.rho for r, _, _ in f.records[1:first_ev])
        post = max(r.e / r.rho for r, _, _ in f.records[first_ev:])
        worst = max((r.e - lm.DIRECTION_TOL) / r.rho for r, _, _ in f.records[1:])
        report(f"lbfgs history gram={gram}: {STEPS} steps, {f.total} closures, {m.evictions} evictions, smallest kept y.s "
               f"{m.min_ys:.3e}; worst e_k / rho_k before the first eviction {pre:.3f}, from it on {post:.3f}; worst "
               f"(e_k - 2e-5) / rho_k {worst:.3f} (K = {lm.K}); rho_k {min(r.rho for r, _, _ in f.records[1:]):.1e} ... "
               f"{max(r.rho for r, _, _ in f.records[1:]):.1e}")
    finally:
        if opt is not None:
            opt.close()
        ref.close()
        eng.close()


# ---------------------------------------------------------------- the vector kernels where their loops loop
@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


# the pair kernel runs 256 workgroups of 1024 threads, two vectors in flight: its unrolled loop starts at n4 > 262144; the
# multi-dot pass gives 1024 vectors to a workgroup and its finish kernel sums 256 workgroups per pass.  n4 = 327680 puts a
# quarter of the vectors through the unrolled loop and 64 of the 320 workgroups into the finish kernel's second pass; + 3:
# the scalar tail
N_DIRECTION = 4 * (262144 + 65536) + 3
# adam / scale / sub / axpy: 2048 workgroups of 256 threads, one float each: the second grid-stride pass starts at n > 524288
N_ELEMENTWISE = 524288 + 70001


@pytest.fixture(scope="module")
def long_history():
    """Five curvature pairs and a gradient of N_DIRECTION floats, built as test_lbfgs_direction_from_an_oracle_state builds
    them (random, positive y.s); made once."""
    g = torch.Generator().manual_seed(105)
    grad = torch.randn(N_DIRECTION, generator=g)
    ys, ss = [], []
    for _ in range(5):
        s_i = torch.randn(N_DIRECTION, generator=g) * 0.1
        y_i = 2.0 * s_i + 0.3 * torch.randn(N_DIRECTION, generator=g) * 0.1
        ys.append(y_i); ss.append(s_i)
    return grad, ys, ss


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("m", [2, 5])
def test_lbfgs_direction_on_a_long_vector(eng, long_history, m, form):
    """nst_lbfgs_direction against the fp64 two-loop recursion on the same fp32 vectors, rel-L2 <= 2e-5, at a length where the
    pair kernel's unrolled loop, the second pass of multi_dot_finish_kernel and the scalar tails all run."""
    grad, ys, ss = long_history
    ys, ss = ys[:m], ss[:m]
    ro = [float(1.0 / y.dot(s)) for y, s in zip(ys, ss)]
    h_diag = float(ys[-1].dot(ss[-1]) / ys[-1].dot(ys[-1]))
    r = lm.two_loop(grad.double().numpy(), [y.double().numpy() for y in ys], [s.double().numpy() for s in ss], ro, h_diag)
    d = eng.lbfgs_direction(dev(grad), [dev(t) for t in ys], [dev(t) for t in ss], ro, h_diag, form)
    err = rel_l2(d.cpu().numpy(), r)
    report(f"lbfgs direction n={N_DIRECTION} m={m} form={form}: rel-L2 vs fp64 recursion {err:.2e}")
    assert err < 2e-5


def test_adam_update_kernel_second_grid_stride_pass(eng):
    """nst_adam_step as in test_adam_update_kernel_vs_torch, on a vector longer than the kernel's grid: m and v bitwise, x to
    rtol 3e-7 / atol 1e-6, more than 95 % of x identical.

    The second moments are kept away from zero (v in [4, 8)), so that every update term stays below 4.  The x tolerance
    presumes that: torch's sqrt / division chain (sqrt, / sqrt(bc2), + eps, m / denom) is not correctly rounded in every lane
    and lands up to two ulps of the UPDATE TERM from the kernel's correctly rounded chain, each of them about one ulp from the
    fp64 value.  Two ulps of a term below 4 are 9.5e-7 < atol; the final addition adds one ulp of x, 1.2e-7 |x| < rtol |x|.
    With v drawn from [0, 4) as in the short test, 0.02 % of the update terms at this length exceed 16 (the largest 47):
    measured on the device, 4 of the 594289 entries were then 1.9e-6 from torch's (one ulp of a term in [16, 32), two of
    one in [8, 16)); a host restatement of the kernel with correctly rounded fp32 operations differs from torch in the same way (one entry, a
    term of -9.11: 1.1 ulp from the fp64 value where torch is 0.9 ulp on the other side)."""
    n = N_ELEMENTWISE
    g = torch.Generator().manual_seed(1)
    grad = torch.randn(n, generator=g) * 3
    st = cpu_ref.AdamState(n)
    st.m = torch.randn(n, generator=g) * 0.5
    st.v = torch.rand(n, generator=g) * 4 + 4
    x = torch.randn(n, generator=g) * 50
    k, lr = 7, 9.93
    st.k = k - 1
    xd, md, vd = dev(x.clone()), dev(st.m.clone()), dev(st.v.clone())
    eng.adam_step(xd, dev(grad), md, vd, k, lr)
    xr = x.clone()
    st.update(xr, grad, lr)
    update = (lr / (1 - 0.9 ** k)) * st.m.double() / (st.v.double().sqrt() / math.sqrt(1 - 0.999 ** k) + 1e-8)
    assert float(update.abs().max()) < 4.0                     # the condition the x tolerance presumes
    assert torch.equal(md.cpu(), st.m)
    assert torch.equal(vd.cpu(), st.v)
    np.testing.assert_allclose(xd.cpu().numpy(), xr.numpy(), rtol=3e-7, atol=1e-6)
    same = float((xd.cpu() == xr).float().mean())
    report(f"adam kernel n={n} k={k}: x bit-identical in {same:.4%} of the entries")
    assert same > 0.95


def test_scale_second_grid_stride_pass(eng):
    """nst_scale bitwise against numpy's fp32 product."""
    src = torch.randn(N_ELEMENTWISE, generator=torch.Generator().manual_seed(2)) * 7
    alpha = np.float32(0.37)
    out = eng.scale(dev(src), float(alpha))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(src.numpy() * alpha))


# ---- a long-vector job through the driver
LONG_H, LONG_W = 837, 839
STYLE_H, STYLE_W = 419, 623
# L-BFGS' first step is lr / |g|_1 along -g: of the order lr / n per pixel.  Under lr = 1 that is a tenth of an ulp of a
# pixel value at this n: x_1 = x_0 almost everywhere and the first pair is rounding noise (the oracle's own driver on this job:
# largest move 3.8e-6, y.s = 3.8e-12, the pair dropped - profiles/r03_lbfgs_first_pair_noise.txt is the same effect).  Under
# lr = 1000 the first step moves pixels by up to 0.56 and steps 2 and 3 keep their pairs (the oracle's driver: y.s = 20 and 2.6e3)
LONG_LR = 1000.0


@pytest.fixture(scope="module")
def long_job(vgg_weights):
    """One level, 837x839, with a style of another size: n = 2106729 (n mod 4 = 1, n4 = 526682) - past the second pass
    of add_scaled / copy / zero (n4 > 524288) and of the one-float-per-thread kernels.  The images are prepared once; `ref`
    is the second engine that evaluates gradients for the mirror."""
    from artstyletransfer_amd.engine import StyleEngine
    content = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(LONG_H, LONG_W, 1)))
    style = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(STYLE_H, STYLE_W, 2)))

    def configure(e):
        e.configure(1, LONG_H, LONG_W)
        e.set_targets(0, content, style)

    ref = StyleEngine(vgg_weights, 0)
    configure(ref)
    n = 3 * LONG_H * LONG_W
    assert n == 2106729 and n % 4 == 1 and n // 4 == 526682
    yield dict(configure=configure, ref=ref, x0=content.reshape(1, 3, LONG_H, LONG_W), n=n)
    ref.close()


@pytest.mark.parametrize("gram", [True, False])
def test_long_vector_job_three_steps(vgg_weights, long_job, gram):
    """max_eval 26, lr LONG_LR, three steps.  Step 1: x_1 against x_0 - t g_0 element by element (scale_copy, copy and
    add_scaled past their second pass and in their tails); steps 2 and 3: the mirror's bound with one and two pairs (sub,
    dot2, the multi-dot / pair kernels and the multi-axpy at this length inside the driver)."""
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine
    eng = StyleEngine(vgg_weights, 0, lbfgs_gram=gram)
    opt = None
    try:
        long_job["configure"](eng)
        x = long_job["x0"].clone()
        opt = PixelOptimizer(eng, "lbfgs", LONG_LR, 26)
        f = Follower(opt, long_job["ref"], x, LONG_LR)
        rec, info, x0 = f.step()
        # x_1 = x_0 + t d with d = -g_0 exactly and t the fp32 value in info.t, against the exact value in fp64 (the product of
        # two floats is exact there): within one ulp of it - add_scaled_kernel may fuse the multiply-add (one rounding, half
        # an ulp) or round the product first
        a, t, d = _flat(x0), np.float32(info.t), rec.d.astype(np.float32)           # (rec.d = -g_0 in fp64, from fp32: exact)
        got = _flat(x)
        exact = a.astype(np.float64) + float(t) * d.astype(np.float64)
        ulps = np.abs(got.astype(np.float64) - exact) / np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        report(f"long job gram={gram}: step 1 t = {info.t:.4g}, {info.closures} closures; x_1 vs x_0 - t g_0: worst "
               f"{ulps.max():.2f} ulp, {float((_bits(got) == _bits(a + t * d)).mean()):.4%} equal to the unfused form, "
               f"{float((got == exact.astype(np.float32)).mean()):.4%} to the fused one; moved entries "
               f"{float((got != a).mean()):.2%}")
        assert ulps.max() <= 1.0, (float(ulps.max()), int(ulps.argmax()))
        assert (got != a).any()
        for k in (2, 3):
            rec, info, _ = f.step(check_bound=False)
            report(f"long job gram={gram}: step {k}: {rec.pairs} pair(s), t = {info.t:.4g}, e_k {rec.e:.2e}, rho_k {rec.rho:.2e}, "
                   f"bound {lm.bound(rec.rho):.2e}")
            assert rec.pairs == k - 1 and rec.kept
            assert rec.e <= lm.bound(rec.rho), (k, rec.e, rec.rho)
    finally:
        if opt is not None:
            opt.close()
        eng.close()


def test_closure_reuse_compare_sees_one_word_anywhere(vgg_weights, long_job):
    """count_diff_partial_kernel runs 256 workgroups of 256 threads with four 16-byte vectors in flight per thread: thread i
    compares vectors i, i + S, i + 2S, i + 3S (S = 65536) per turn of its unrolled loop while i + 3S < n4, the rest one by
    one in a remainder loop, and thread 0 of workgroup 0 the n mod 4 tail words.  One flipped mantissa bit in each of those
    regions must turn a served closure into an evaluated one."""
    from artstyletransfer_amd.engine import PixelOptimizer
    eng = long_job["ref"]
    n = long_job["n"]
    n4, S, U = n // 4, 256 * 256, 4

    def region(v):
        """('unrolled', slot) or ('remainder', None): where vector v of the compare is handled."""
        i = v % S
        while i + (U - 1) * S < n4:
            if (v - i) % S == 0 and 0 <= (v - i) // S < U:
                return "unrolled", (v - i) // S
            i += U * S
        assert v >= i and (v - i) % S == 0 and v < n4
        return "remainder", None

    words = {"word 1": 1,
             "fourth slot of the unrolled loop": 4 * (10 + 3 * S) + 2,
             "remainder loop": 4 * (n4 - 100) + 1,
             "tail word": n - 1}
    assert region(0) == ("unrolled", 0) and region(10 + 3 * S) == ("unrolled", 3) and region(n4 - 100) == ("remainder", None)
    assert n % 4 == 1 and words["tail word"] == 4 * n4

    x = long_job["x0"].clone()
    opt = PixelOptimizer(eng, "lbfgs", 10.0, 1)
    try:
        def step():
            ev0, sv0 = opt.closure_stats()
            info, _ = opt.step(x, CW, SW, TVW)
            ev1, sv1 = opt.closure_stats()
            assert (ev1 - ev0) + (sv1 - sv0) == info.closures
            return ev1 - ev0, sv1 - sv0, info.closures

        def served_step(what):
            ev, sv, closures = step()
            assert sv == 1 and ev == closures - 1, what

        def evaluated_step(what):
            ev, sv, closures = step()
            assert sv == 0 and ev == closures >= 1, what

        bits = x.view(-1).view(torch.int32)
        evaluated_step("the first step")
        served_step("control: x untouched")
        for what, w in words.items():
            bits[w] ^= 1
            evaluated_step(what)
            bits[w] ^= 1                                      # the remembered image is the flipped one: evaluated again
            evaluated_step(what + ", restored")
            served_step("control after " + what)
    finally:
        opt.close()
