"""GPU: the temporal feature (nst_level_set_anchor, nst_anchor_loss, nst_warp_bilinear, nst_flow_weights; Ruder, Dosovitskiy &
Brox 2016) against the fp64 restatements of the definitions in include/nst_hip.h (tests/temporal_ref.py), and the video driver.

Bounds.  The term's value: 1e-6 relative to fp64.  Its gradient: rel-L2 to fp64 at most 3 x the distance of the same formula in
torch fp32 from fp64 (the project's rule for a kernel).  The warp: 8 fp32 ulps of max|src| (two weights, four products and
three sums along the longest chain are at most eight roundings of values bounded by max|src|; the fraction comes from the
flow alone and carries at most 2^-25).  The flow weights: equal to the fp64 plane wherever both inequalities have a relative margin above 1e-4.  The
closure: totals 1e-5, gradients hip_helpers.assert_grad_close, everything else bitwise.

The kernels' geometry (temporal.hip through nst_anchor_geometry): a block covers 256 threads x 4 pixels per pass; the
block-boundary case has one element more than one block's pass."""
import asyncio

import numpy as np
import pytest
import torch

import temporal_ref as ref
from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, assert_grad_close, dev, levels, rel_l2, report

pytestmark = pytest.mark.gpu

H, W, HS, WS, NLEV = 32, 48, 32, 40, 2          # the smallest two-level job nst_job_configure accepts (test_hip_ctx_bytes.py)
SCHEDULES = {"batched": {}, "per_level": {"batched": False}}
E_ARG, E_STATE = -1, -2


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


# ================================================================================================ the term alone
def _weights(h, w, seed):
    """Random in [0,1] with exact 0 and 1 runs."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(0.0, 1.0, h * w).astype(np.float32)
    n = h * w
    c[n // 5: n // 5 + max(n // 7, 1)] = 0.0
    c[n // 2: n // 2 + max(n // 6, 1)] = 1.0
    return torch.from_numpy(c.reshape(h, w))


def _piece_shapes(eng):
    blocks, elems = eng.anchor_geometry()
    assert blocks == 256 and elems == 1024
    return [(1, 1), (3, 5), (50, 77), (33, 128), (25, 41)], elems      # 25 * 41 = elems + 1: one more than a block's pass


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("C", [1, 3])
def test_anchor_term_against_fp64(eng, C, weighted):
    shapes, elems = _piece_shapes(eng)
    assert shapes[-1][0] * shapes[-1][1] == elems + 1
    for k, (h, w) in enumerate(shapes):
        g = torch.Generator().manual_seed(100 * C + k)
        y = (torch.rand((1, C, h, w), generator=g) * 255.0 - 120.0).float()
        a = (y + torch.randn((1, C, h, w), generator=g) * 20.0).float()
        c = _weights(h, w, 7 + k) if weighted else None
        v64, g64 = ref.anchor_piece(y, a, c, torch.float64)
        v32, g32 = ref.anchor_piece(y, a, c, torch.float32)
        val, grad = eng.anchor_loss(dev(y), dev(a), dev(c) if weighted else None, want_grad=True)
        val_only = eng.anchor_loss(dev(y), dev(a), dev(c) if weighted else None)
        assert np.array_equal(_bits(val), _bits(val_only))
        e_v = abs(float(val.cpu()) - v64) / abs(v64)
        e_g, e_32 = rel_l2(grad.cpu().numpy(), g64.numpy()), rel_l2(g32.numpy(), g64.numpy())
        report(f"anchor term C={C} {h}x{w} weighted={weighted}: value rel {e_v:.2e}; gradient rel-L2 {e_g:.2e}, torch fp32 {e_32:.2e} "
               f"(bound {3 * e_32:.2e})")
        assert e_v <= 1e-6, (h, w, e_v)
        assert e_g <= 3 * e_32, (h, w, e_g, e_32)


@pytest.mark.parametrize("C", [1, 3])
def test_anchor_term_of_the_anchor_itself_is_exactly_zero(eng, C):
    for h, w in ((3, 5), (50, 77), (33, 128)):
        y = dev((torch.rand((1, C, h, w)) * 255.0 - 120.0).float())
        for c in (None, dev(_weights(h, w, 3))):
            val, grad = eng.anchor_loss(y, y.clone(), c, want_grad=True)
            assert not _bits(val).any() and not _bits(grad).any()


# ================================================================================================ the warp
def _ulps(src):
    return 8 * float(np.spacing(np.float32(np.abs(src).max())))


def _src(C, h, w, seed):
    return (np.random.RandomState(seed).uniform(-120.0, 135.0, (C, h, w))).astype(np.float32)


def test_warp_zero_flow_is_the_identity(eng):
    src = _src(3, 37, 53, 1)
    out, valid = eng.warp_bilinear(dev(torch.from_numpy(src)), dev(torch.zeros((2, 37, 53))))
    assert np.array_equal(_bits(out), src.view(np.int32))
    v = valid.cpu().numpy()
    assert v[:-1, :-1].all() and not v[-1].any() and not v[:, -1].any()      # (the second tap of the last row / column is outside)


def test_warp_integer_flows_gather_exactly(eng):
    h, w = 37, 53
    src = _src(3, h, w, 2)
    rng = np.random.RandomState(3)
    flow = rng.randint(-3, 4, (2, h, w)).astype(np.float32)
    out, valid = eng.warp_bilinear(dev(torch.from_numpy(src)), dev(torch.from_numpy(flow)))
    out, valid = out.cpu().numpy(), valid.cpu().numpy()
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sx, sy = xx + flow[0].astype(int), yy + flow[1].astype(int)
    inside = (sx >= 0) & (sx + 1 <= w - 1) & (sy >= 0) & (sy + 1 <= h - 1)
    assert np.array_equal(valid, inside.astype(np.float32))
    assert inside[4:-4, 4:-4].all()
    gathered = src[:, np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
    assert np.array_equal(out[:, inside].view(np.int32), gathered[:, inside].view(np.int32))


def test_warp_fractional_flows_against_fp64(eng):
    h, w = 37, 53
    src = _src(3, h, w, 4)
    flow = np.random.RandomState(5).uniform(-3.0, 3.0, (2, h, w)).astype(np.float32)
    out, valid = eng.warp_bilinear(dev(torch.from_numpy(src)), dev(torch.from_numpy(flow)))
    want, want_valid = ref.sample(src, flow[0], flow[1])
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - want).max())
    report(f"warp 37x53, flows in [-3,3]: max abs error {err:.3e}, bound {_ulps(src):.3e}")
    assert err <= _ulps(src)
    assert np.array_equal(valid.cpu().numpy(), want_valid.astype(np.float32))
    v = want_valid
    assert not v[0].all() and not v[-1].all() and not v[:, 0].all() and not v[:, -1].all() and v[5:-5, 5:-5].all()


@pytest.mark.parametrize("side,dx,dy", [("left", -7.25, 0.5), ("right", 9.5, -0.25), ("top", 0.75, -6.5), ("bottom", -0.5, 8.25),
                                        ("far", 1e9, -3e38)])
def test_warp_samples_leaving_the_image(eng, side, dx, dy):
    h, w = 12, 20
    src = _src(3, h, w, 6)
    flow = np.stack([np.full((h, w), dx, np.float32), np.full((h, w), dy, np.float32)])
    out, valid = eng.warp_bilinear(dev(torch.from_numpy(src)), dev(torch.from_numpy(flow)))
    want, want_valid = ref.sample(src, flow[0], flow[1])
    assert float(np.abs(out.cpu().numpy().astype(np.float64) - want).max()) <= _ulps(src)
    assert np.array_equal(valid.cpu().numpy(), want_valid.astype(np.float32))
    assert not want_valid.all() and (side == "far") == (not want_valid.any())


def test_warp_non_finite_flow_keeps_the_pixel(eng):
    h, w = 6, 9
    src = _src(3, h, w, 7)
    flow = np.zeros((2, h, w), np.float32)
    flow[0, 2, 3], flow[1, 4, 5], flow[0, 1, 1] = np.nan, np.inf, -np.inf
    out, valid = eng.warp_bilinear(dev(torch.from_numpy(src)), dev(torch.from_numpy(flow)))
    assert np.array_equal(_bits(out), src.view(np.int32))
    v = valid.cpu().numpy()
    assert v[2, 3] == 0 and v[4, 5] == 0 and v[1, 1] == 0 and v[2, 2] == 1


def test_warp_far_column_keeps_the_error_bound(eng):
    """Column 4099 of a 2 x 4100 image with dx = 0.3: x + dx in fp32 would round the fraction to 1 / 4096 steps; the position
    rule takes integer part and fraction of the flow alone."""
    h, w = 2, 4100
    src = _src(1, h, w, 8)
    flow = np.zeros((2, h, w), np.float32)
    flow[0] = 0.3
    flow[0, :, 4090:] = -0.3                      # (the last columns sample to the left, so that column 4099 is valid)
    out, valid = eng.warp_bilinear(dev(torch.from_numpy(src)), dev(torch.from_numpy(flow)))
    want, want_valid = ref.sample(src, flow[0], flow[1])
    err = np.abs(out.cpu().numpy().astype(np.float64) - want)[0]
    report(f"warp 2x4100: max abs error at columns >= 4090 {err[:, 4090:].max():.3e}, everywhere {err.max():.3e}, bound {_ulps(src):.3e}")
    assert err.max() <= _ulps(src)
    assert want_valid[0, 4099] and valid.cpu().numpy()[0, 4099] == 1 and want_valid[0, 4000]
    # what forming x + dx in fp32 would have cost there: a fraction off by 5e-5, far beyond the bound on a difference of taps
    naive_t = np.float64(np.float32(4000.0) + np.float32(0.3)) - 4000.0
    assert abs(naive_t - 0.3) > 1e-5


# ================================================================================================ the flow weights
def test_flow_weights_against_fp64(eng):
    fwd, bwd = ref.synthetic_flow_pair()
    want, m1, m2 = ref.flow_weights(fwd, bwd)
    out, zeros, ones = ref.flow_caps(want, m1, m2)
    assert out <= 0.01 and zeros >= 0.05 and ones >= 0.05, (out, zeros, ones)
    got = eng.flow_weights(dev(torch.from_numpy(fwd)), dev(torch.from_numpy(bwd))).cpu().numpy()
    assert set(np.unique(got)) <= {0.0, 1.0}
    keep = (m1 > 1e-4) & (m2 > 1e-4)
    report(f"flow weights 48x64: {zeros:.1%} zeros, {ones:.1%} ones, {out:.2%} of the pixels within the margin; "
           f"{int((got != want).sum())} pixels differ, {int((got != want)[keep].sum())} of them outside the margin")
    assert np.array_equal(got[keep], want[keep].astype(np.float32))


def test_flow_weights_non_finite_backward_flow_is_unreliable(eng):
    fwd, bwd = ref.synthetic_flow_pair()
    bwd = bwd.copy()
    bwd[0, 10, 10] = np.nan
    got = eng.flow_weights(dev(torch.from_numpy(fwd)), dev(torch.from_numpy(bwd))).cpu().numpy()
    assert got[10, 10] == 0 and got[10, 9] == 0 and got[10, 11] == 0 and got[9, 10] == 0      # (its neighbours' differences are NaN)
    assert got[5, 5] == 1


# ================================================================================================ the closure
def _job(luminance=False):
    contents, styles = levels(H, W, NLEV, 1), levels(HS, WS, NLEV, 2)
    x = (0.6 * contents[0] + 0.4 * cpu_ref.synthetic_image(H, W, 9)).astype(np.float32)
    return contents, styles, x


def _setup(e, luminance=False):
    """Configure the two-level job, make its targets, return the start image on the device."""
    from artstyletransfer_amd import host_image
    contents, styles, x = _job()
    e.configure(NLEV, H, W)
    if luminance:
        e.set_color("luminance")
        for i in range(NLEV):
            e.set_targets(i, dev(torch.from_numpy(host_image.luminance(contents[i]))), dev(torch.from_numpy(host_image.luminance(styles[i]))))
        return dev(torch.from_numpy(host_image.luminance(x)).reshape(1, 1, H, W))
    for i in range(NLEV):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))
    return dev(cpu_ref.prepare_img(x))


def _make(vgg_weights, schedule, luminance=False):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, **SCHEDULES[schedule])
    return e, _setup(e, luminance)


def _random_anchor(x, seed):
    """(anchors, weights) of both levels: the level image moved by noise of 20 units, weights with exact 0 and 1 runs."""
    g = torch.Generator().manual_seed(seed)
    out_a, out_c = [], []
    xl = x.cpu()
    for l in range(NLEV):
        if l:
            xl = cpu_ref.bicubic_half(xl)
        out_a.append((xl + torch.randn(xl.shape, generator=g) * 20.0).float())
        out_c.append(_weights(xl.shape[-2], xl.shape[-1], seed + l))
    return out_a, out_c


def _launches(e):
    return [tuple(sorted(d.items())) for d in e.last_closure_launches()]


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_a_cleared_anchor_and_a_zero_weight_leave_no_trace(vgg_weights, schedule):
    """(1) set_anchor + clear_anchor, and a gamma = 0 call, against an engine that never made the call: rows, gradient bits
    and the launch record."""
    a, xa = _make(vgg_weights, schedule)
    b, xb = _make(vgg_weights, schedule)
    try:
        anchors, weights = _random_anchor(xa, 11)
        a.set_timing(2)
        b.set_timing(2)
        gb, lb = b.closure(xb, CW, SW, TVW)
        rec_b = _launches(b)
        for l in range(NLEV):
            a.set_anchor(l, dev(anchors[l]), dev(weights[l]), gamma=5.0)
        assert a.anchor(0) == (5.0, True) and a.anchor(1) == (5.0, True)
        a.clear_anchor()
        assert a.anchor(0) == (0.0, False) and a.anchor(1) == (0.0, False)
        ga, la = a.closure(xa, CW, SW, TVW)
        assert np.array_equal(_bits(ga), _bits(gb)) and np.array_equal(_bits(la), _bits(lb))
        assert _launches(a) == rec_b and len(rec_b) > 20
        a.set_anchor(0, dev(anchors[0]), None, gamma=0.0)
        assert a.anchor(0) == (0.0, False)
        ga, la = a.closure(xa, CW, SW, TVW)
        assert np.array_equal(_bits(ga), _bits(gb)) and np.array_equal(_bits(la), _bits(lb))
        assert _launches(a) == rec_b
        assert not a.temporal_losses().cpu().numpy().any()
        # with an anchor the record grows by the two passes of each level that carries one
        a.set_anchor(1, dev(anchors[1]), dev(weights[1]), gamma=5.0)
        a.closure(xa, CW, SW, TVW)
        assert len(_launches(a)) == len(rec_b) + 2
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_an_image_that_equals_its_anchors_has_no_term(vgg_weights, schedule):
    """(2) anchor = x on level 0 and bicubic_half(x) on level 1: tmp exactly 0, the gradient bits of the job without."""
    e, x = _make(vgg_weights, schedule)
    try:
        g0, l0 = e.closure(x, CW, SW, TVW)
        g0, l0 = g0.clone(), l0.clone()
        c1 = dev(_weights(H // 2, W // 2, 5))
        e.set_anchor(0, x.clone(), None, gamma=1e6)
        e.set_anchor(1, e.bicubic_half(x), c1, gamma=1e6)
        g1, l1 = e.closure(x, CW, SW, TVW)
        assert not _bits(e.temporal_losses()).any()
        assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    finally:
        e.close()


def _term_check(e, x, what):
    """(3) random anchors and weights on both levels, gamma per level so that the term is 10 to 50 % of the level total."""
    g0, l0 = e.closure(x, CW, SW, TVW)
    g0 = g0.cpu().numpy().astype(np.float64)
    rows0 = l0.cpu().numpy()[:-1].reshape(NLEV, 4).astype(np.float64)
    anchors, weights = _random_anchor(x, 21)
    # the fp64 term of each level on the fp64 pyramid of x, and the chain back to x
    x64 = x.cpu().double().clone().requires_grad_(True)
    lv, tmp64 = x64, []
    for l in range(NLEV):
        if l:
            lv = ref.bicubic_half64(lv)
        tmp64.append(ref.anchor_term(lv, anchors[l].double(), weights[l].double()))
    gammas = [float(np.float32(0.3 * rows0[l, 0] / float(tmp64[l].detach()))) for l in range(NLEV)]
    sum(g * t for g, t in zip(gammas, tmp64)).backward()
    for l in range(NLEV):
        e.set_anchor(l, dev(anchors[l]), dev(weights[l]), gamma=gammas[l])
    g1, l1 = e.closure(x, CW, SW, TVW)
    rows1 = l1.cpu().numpy()[:-1].reshape(NLEV, 4).astype(np.float64)
    tmp = e.temporal_losses().cpu().numpy().astype(np.float64)
    for l in range(NLEV):
        share = gammas[l] * tmp[l] / rows1[l, 0]
        e_t = abs(tmp[l] - float(tmp64[l].detach())) / float(tmp64[l].detach())
        e_d = abs((rows1[l, 0] - rows0[l, 0]) - gammas[l] * tmp[l]) / (gammas[l] * tmp[l])
        report(f"closure {what} level {l}: gamma {gammas[l]:.3e}, tmp {tmp[l]:.4e} (fp64 rel {e_t:.1e}), share of the total {share:.1%}, "
               f"total_with - total_without vs gamma tmp rel {e_d:.1e}")
        assert 0.10 <= share <= 0.50
        assert e_t <= 1e-6
        assert e_d <= 1e-5
        assert np.array_equal(rows1[l, 1:], rows0[l, 1:])                 # content, style, tv: the row keeps its four entries
    assert float(l1[-1].cpu()) == pytest.approx(float(rows1[:, 0].sum()), rel=1e-6)
    assert_grad_close(g1.cpu().numpy(), g0 + x64.grad.numpy(), what=f"{what}: with anchors vs without + the fp64 term chain")
    return gammas, anchors, weights


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_the_term_in_the_closure_against_fp64(vgg_weights, schedule):
    e, x = _make(vgg_weights, schedule)
    try:
        _term_check(e, x, f"rgb {schedule}")
    finally:
        e.close()


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_the_term_in_the_luminance_closure_against_fp64(vgg_weights, schedule):
    """(5) C = 1: one-plane anchors in the units of the optimised plane."""
    e, x = _make(vgg_weights, schedule, luminance=True)
    try:
        assert tuple(x.shape) == (1, 1, H, W)
        _term_check(e, x, f"luminance {schedule}")
        # an image that equals its anchors, one plane
        e.set_anchor(0, x.clone(), None, gamma=10.0)
        e.set_anchor(1, e.bicubic_half(x), None, gamma=10.0)
        e.closure(x, CW, SW, TVW)
        assert not _bits(e.temporal_losses()).any()
    finally:
        e.close()


def test_halves_masks_and_optimisers_give_the_bits_of_one_closure(vgg_weights):
    """(4) closure_forward + closure_backward; closure_levels per one-level mask, summed; optimiser steps."""
    from artstyletransfer_amd.engine import PixelOptimizer
    e, x = _make(vgg_weights, "batched")
    twin, _ = _make(vgg_weights, "batched")
    try:
        anchors, weights = _random_anchor(x, 31)
        for eng_ in (e, twin):
            for l in range(NLEV):
                eng_.set_anchor(l, dev(anchors[l]), dev(weights[l]) if l else None, gamma=3e3)
        g, ls = e.closure(x, CW, SW, TVW)
        g, ls = g.clone(), ls.clone()
        tmp = e.temporal_losses().clone()
        assert (tmp > 0).all()
        # the halves
        lf = e.closure_forward(x, CW, SW, TVW)
        assert np.array_equal(_bits(lf), _bits(ls)) and np.array_equal(_bits(e.temporal_losses()), _bits(tmp))
        gh = torch.full_like(g, -12345.0)
        e.closure_backward(x, CW, SW, TVW, grad=gh)
        assert np.array_equal(_bits(gh), _bits(g))
        # one-level masks: a level not owned contributes zeros, rows and gradients add up
        gsum, rows, tsum = torch.zeros_like(g, dtype=torch.float64), [], []
        for l in range(NLEV):
            gm, lm = e.closure_levels(x, CW, SW, TVW, 1 << l)
            gsum += gm.double()
            r = lm[:-1].reshape(NLEV, 4)
            t = e.temporal_losses()
            assert not _bits(r[1 - l]).any() and not _bits(t[1 - l]).any()
            assert np.array_equal(_bits(r[l]), _bits(ls[:-1].reshape(NLEV, 4)[l])) and np.array_equal(_bits(t[l]), _bits(tmp[l]))
        assert rel_l2(gsum.cpu().numpy(), g.cpu().numpy()) < 2e-6
        # optimiser steps: closure reuse and the lazy backward on (the default) against both off, and against the closure
        for name, max_eval in (("lbfgs", 4), ("adam", 1)):
            runs = []
            for eng_, plain in ((e, False), (twin, True)):
                xs = x.clone()
                opt = PixelOptimizer(eng_, name, 10.0, max_eval)
                if plain and name == "lbfgs":
                    opt.set_closure_reuse(False)
                    opt.set_lazy_backward(False)
                out = []
                for _ in range(3):
                    before = xs.clone()
                    info, r = opt.step(xs, CW, SW, TVW)
                    out.append((before, r.copy(), xs.clone(), info.closures))
                if name == "lbfgs" and not plain:
                    report(f"L-BFGS with anchors: closures served {opt.closure_stats()}, forward-only {opt.backward_stats()}")
                opt.close()
                runs.append(out)
            for (b0, r0, x0, n0), (b1, r1, x1, n1) in zip(*runs):
                assert n0 == n1 and np.array_equal(r0.view(np.int32), r1.view(np.int32)) and np.array_equal(_bits(x0), _bits(x1))
            for before, r, _, _ in runs[0]:
                _, lc = twin.closure(before, CW, SW, TVW)
                assert np.array_equal(r[0].view(np.int32), _bits(lc)), name      # a step's first closure is the closure at its image
    finally:
        e.close()
        twin.close()


def test_the_stripe_closure_refuses_a_level_with_an_anchor(vgg_weights):
    """(6) nst_window_begin returns NST_E_STATE."""
    from artstyletransfer_amd import _lib
    from artstyletransfer_amd.engine import NstError, StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        c, s = levels(64, 96, 1, 1), levels(64, 96, 1, 2)
        e.configure(1, 64, 96)
        e.set_targets(0, dev(cpu_ref.prepare_img(c[0])), dev(cpu_ref.prepare_img(s[0])))
        x = dev(cpu_ref.prepare_img(c[0]))
        zeros = lambda: torch.zeros(e.window_sums_count(), dtype=torch.float32, device=x.device)      # noqa: E731
        sums = e.window_begin(x, 0, 64, 64, zeros())           # (the call does not write every slot of the buffer)
        e.set_anchor(0, x.clone(), None, gamma=1.0)
        with pytest.raises(NstError, match=r"\(-2\).*temporal term"):
            e.window_begin(x, 0, 64, 64)
        assert _lib.NST_E_STATE == E_STATE
        e.clear_anchor()
        again = e.window_begin(x, 0, 64, 64, zeros())
        assert np.array_equal(_bits(again), _bits(sums))
    finally:
        e.close()


def test_bytes_are_exact_and_a_new_job_comes_back_clean(vgg_weights):
    """(7) nst_ctx_bytes after set_anchor on both levels and clear_anchor() is that of a fresh configured engine; after
    release_job and a new configure no level carries an anchor.  And the refusals change nothing."""
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        assert e.lib.nst_level_set_anchor(e.ctx, 0, None, None, 1.0, None) == E_STATE        # no configured job
        x = _setup(e)
        fresh = e.bytes()
        anchors, weights = _random_anchor(x, 41)
        e.set_anchor(0, dev(anchors[0]), dev(weights[0]), gamma=2.0)
        one = e.bytes()
        assert one == fresh + 4 * (3 * H * W + H * W) + 8 * 256 + 4                         # anchor, weights, partials, the value
        e.set_anchor(1, dev(anchors[1]), None, gamma=2.0)
        both = e.bytes()
        assert both == one + 4 * 3 * (H // 2) * (W // 2) + 8 * 256 + 4
        # refusals: nothing changes
        a0 = dev(anchors[0])
        stream = torch.cuda.current_stream().cuda_stream
        for level, gamma in ((-1, 1.0), (2, 1.0), (0, -1.0), (0, float("nan")), (0, float("inf"))):
            assert e.lib.nst_level_set_anchor(e.ctx, level, a0.data_ptr(), None, gamma, stream) == E_ARG
            assert e.bytes() == both and e.anchor(0) == (2.0, True) and e.anchor(1) == (2.0, False)
        # replacing an anchor charges nothing more
        e.set_anchor(0, dev(anchors[0]), dev(weights[0]), gamma=4.0)
        assert e.bytes() == both and e.anchor(0) == (4.0, True)
        e.clear_anchor(1)
        assert e.bytes() == one
        e.clear_anchor()
        assert e.bytes() == fresh
        # a pooled engine comes back clean with no Python-side reset
        e.set_anchor(0, dev(anchors[0]), None, gamma=2.0)
        e.closure(x, CW, SW, TVW)
        assert float(e.temporal_losses()[0].cpu()) > 0
        e.release_job()
        assert e.anchor(0) == (0.0, False)
        x = _setup(e)
        assert e.bytes() == fresh and e.anchor(0) == (0.0, False) and e.anchor(1) == (0.0, False)
        e.closure(x, CW, SW, TVW)
        assert not _bits(e.temporal_losses()).any()
    finally:
        e.close()


# ================================================================================================ the driver
def test_video_driver_holds_frame_one_to_the_warped_frame_zero(vgg_weights):
    """Two 64x96 frames, the second the first moved one pixel to the right (8 pixels at the 512x768 the two-level job yields:
    a constant integer backward flow of (-8, 0)), Adam, four iterations.  With a temporal weight the mean squared difference
    between frame 1's result and the warped frame-0 result over the pixels with c = 1 is smaller than without; frame 0 is
    bitwise neural_style_transfer()'s."""
    from artstyletransfer_amd import config, neural_nets, video
    from artstyletransfer_amd.neural_nets import shared_engine
    import neural_style_transfer as nst
    neural_nets.set_weights(vgg_weights)
    f0 = cpu_ref.synthetic_image(64, 96, seed=1)
    f1 = np.roll(f0, 1, axis=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=2, iters_num=4, optimizer="adam", init_method="content")
    hh, ww = video.result_size(f0.shape, 2)
    assert (hh, ww) == (512, 768)
    flow = np.zeros((hh, ww, 2), np.float32)
    flow[..., 0] = -8.0

    def run(tw):
        async def go():
            return [(i, p, img) async for i, p, img in video.neural_style_transfer_video([f0, f1], style, [flow], temporal_weight=tw, cfg=cfg)]
        return asyncio.run(go())

    async def plain():
        return [img async for _, img in nst.neural_style_transfer(
            nst.ContentStylePair(("frame", f0), ("style", style)), cfg.content_weight, cfg.style_weight, cfg.tv_weight, cfg.optimizer,
            cfg.model, cfg.init_method, cfg.iters_num, cfg.levels_num, cfg.noise_factor, cfg.noise_levels,
            cfg.noise_levels_central_amplitude, cfg.noise_levels_peripheral_amplitude, cfg.noise_levels_dispersion)]

    held, free, alone = run(1e9), run(0.0), asyncio.run(plain())
    assert [(i, p) for i, p, _ in held] == [(0, 25.0), (0, 50.0), (0, 75.0), (0, 100.0), (1, 25.0), (1, 50.0), (1, 75.0), (1, 100.0)]
    for k in range(4):
        assert np.array_equal(held[k][2], alone[k]) and np.array_equal(free[k][2], alone[k])
    e = shared_engine(torch.device("cuda", torch.cuda.current_device()))
    src = dev(torch.from_numpy(held[3][2]).permute(2, 0, 1))
    omega, valid = e.warp_bilinear(src, dev(torch.from_numpy(flow).permute(2, 0, 1)))
    omega = omega.permute(1, 2, 0).cpu().numpy().astype(np.float64)
    c = valid.cpu().numpy() == 1
    assert 0.9 < c.mean() < 1.0 and not c[:, :8].any()
    assert np.array_equal(omega[:, 8:], held[3][2][:, :-8].astype(np.float64))          # an exact gather
    d_held = float(((held[-1][2].astype(np.float64) - omega) ** 2)[c].mean())
    d_free = float(((free[-1][2].astype(np.float64) - omega) ** 2)[c].mean())
    report(f"video driver 512x768, 4 Adam steps: msd(frame 1, warped frame 0) over c = 1: {d_held:.4e} with temporal_weight 1e9, {d_free:.4e} with 0")
    assert np.isfinite(held[-1][2]).all() and d_held < d_free
