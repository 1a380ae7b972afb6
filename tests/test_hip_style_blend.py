"""GPU: per-layer style weights (nst_job_set_style_weights) and style targets blended from several style images
(nst_level_set_targets_blend), as include/nst_hip.h defines them:

    style term of a level = (sum_i w_i MSE(G_i, Gt_i)) / nstyle                 over the maps of the style set, ascending
    Gt_i = sum_k b^_ki G_i(style_k),  b^_ki = float(B_ki / sum_k B_ki)          fp32 sum in ascending k, B_ki = 0 skipped

The reference here is a torch restatement of those two lines (`restated_targets`, `restated_closure`) built from the CPU
oracle's pieces (vgg19_features, gram_matrix, total_variation, bicubic_half) and evaluated under the device pass's ReLU /
pooling / TV-sign decisions (cpu_ref.Decisions), as test_hip_taps.test_relu_taps_vs_oracle_under_equal_decisions does.

Bounds (none of them taken from what the code under test gives):
  gradient against the restatement under equal decisions: rel-L2 < 5e-6 (test_hip_taps.py's outright gradient bound);
  loss totals against the restatement 1e-5, rows 2e-5 by hip_helpers.check_rows (what test_hip_taps.py holds the closure to
  against the oracle); rows of two DEVICE evaluations that must agree: rtol 1e-6 (test_level_sharded_closure_adds_up);
  what must be the same bits is compared as bits.
Geometries: two levels 64x96 + 32x48 (batched schedule) and one level 50x76 (per-level walker, odd sizes); style images
48x80, 50x76 and 37x53."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, check_rows, dev, levels as _levels, rel_l2, report

pytestmark = pytest.mark.gpu

MODES = {"f16x2": {}, "per_level": {"batched": False}, "bf16x3": {"conv_mode": "bf16x3"}, "f32": {"conv_mode": "f32"}}
TAP_LAYER = (0, 2, 4, 8, 9, 12)          # Vgg19 output index -> conv layer
DEFAULT = (4, (0, 1, 2, 3, 5))
WEIGHTINGS = (("content", (CW, 0.0, 0.0)), ("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW)))
GRAD_TOL = 5e-6
ONES = (1.0,) * 6
W_MIXED = (1.0, 0.5, 0.0, 2.0, 1.0, 0.25)
# image A on maps 0-1, image B on maps 2-5, column 1 mixed (and a third image on the deepest map alone)
B2_UNIFORM = ((0.25,) * 6, (0.75,) * 6)
B3_PER_MAP = ((1.0, 0.6, 0.0, 0.0, 0.0, 0.0), (0.0, 0.4, 1.0, 1.0, 1.0, 0.5), (0.0, 0.0, 0.0, 0.0, 0.0, 1.5))
STYLE_SIZES = ((48, 80), (50, 76), (37, 53))


@pytest.fixture(scope="module")
def engines(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = StyleEngine(vgg_weights, 0, **MODES[mode])
        return made[mode]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture()
def eng(engines):
    e = engines("f16x2")
    yield e
    e.reset_style_weights()
    e.reset_taps()
    e.reset_color()
    e.reset_pooling()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- inputs, made once ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def job2():
    """Two levels 64x96 + 32x48 (the geometry of the *_64x96_L1 fixtures); three style pyramids of their own sizes."""
    c = _levels(64, 96, 2, 1)
    styles = [_levels(h, w, 2, 20 + k) for k, (h, w) in enumerate(STYLE_SIZES)]
    styles[2] = [styles[2][0], cpu_ref.synthetic_image(19, 27, 29)]          # (37x53 halves to 18x26; any size >= 16 will do)
    x = cpu_ref.prepare_img((0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(64, 96, seed=9)).astype(np.float32))
    return c, styles, x


@pytest.fixture(scope="module")
def job1():
    """One odd level 50x76."""
    c = [cpu_ref.synthetic_image(50, 76, 3)]
    styles = [[cpu_ref.synthetic_image(h, w, 30 + k)] for k, (h, w) in enumerate(STYLE_SIZES)]
    x = cpu_ref.prepare_img((0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(50, 76, seed=8)).astype(np.float32))
    return c, styles, x


def _prep(img):
    return dev(cpu_ref.prepare_img(img))


def _configure(e, c):
    e.configure(len(c), *c[0].shape[:2])


def _set_blend(e, c, styles, B):
    """styles: K pyramids; B: K x 6."""
    for l in range(len(c)):
        e.set_targets_blend(l, _prep(c[l]), [_prep(s[l]) for s in styles], B)


def _set_plain(e, c, s):
    for l in range(len(c)):
        e.set_targets(l, _prep(c[l]), _prep(s[l]))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def avg_features(x, weights, decisions=None, record=None):
    """cpu_ref.vgg19_features with the four pools averaging (the header's NST_POOL_AVG)."""
    outs = []
    for li, ((name, _, _), (w, b)) in enumerate(zip(cpu_ref.VGG19_CONVS, weights)):
        pre = F.conv2d(x, w, b, stride=1, padding=1)
        if record is not None:
            record.append(pre.detach())
        x = F.relu(pre) if decisions is None else pre * decisions.relu[li].to(pre.dtype)
        if name in cpu_ref.TAPS:
            outs.append(x)
        if name in cpu_ref.POOL_AFTER:
            x = F.avg_pool2d(x, kernel_size=2, stride=2)
    return outs


def b_hat(B):
    """b^_ki = B_ki / sum_k B_ki in fp64, cast to float (columns without weight stay 0: maps outside the style set)."""
    B = np.asarray(B, dtype=np.float32).astype(np.float64)
    col = B.sum(axis=0)
    return np.array([[np.float32(B[k, i] / col[i]) if col[i] > 0 else np.float32(0) for i in range(6)] for k in range(len(B))],
                    dtype=np.float32)


class Targets:
    pass


def restated_targets(content_t, styles_t, B, weights, taps=DEFAULT, feats=cpu_ref.vgg19_features):
    """Targets of one level: the content map of the content image and Gt_i = sum_k b^_ki G_i(style_k), accumulated in fp32
    in ascending k, the first contributing k written as b^ G, a k with B_ki = 0 skipped."""
    content_i, style_set = taps
    bh = b_hat(B)
    t = Targets()
    with torch.no_grad():
        t.content = feats(content_t, weights)[content_i].squeeze(0)
        sf = [feats(s, weights) if any(B[k][i] > 0 for i in style_set) else None for k, s in enumerate(styles_t)]
        t.grams = {}
        for i in style_set:
            gt = None
            for k in range(len(styles_t)):
                if not B[k][i] > 0:
                    continue
                term = torch.tensor(bh[k, i]) * cpu_ref.gram_matrix(sf[k][i])
                gt = term if gt is None else gt + term
            t.grams[i] = gt
    return t


def restated_closure(x, targets, weights, cw, sw, tvw, w6=ONES, taps=DEFAULT, decisions=None, feats=cpu_ref.vgg19_features):
    """cpu_ref.closure_eval with style = (sum_i w_i MSE_i) / nstyle over the style set in ascending order: (total, gradient,
    rows)."""
    content_i, style_set = taps
    x = x.detach().clone().requires_grad_(True)
    lv, total, rows = [x], None, []
    for l, tg in enumerate(targets):
        if l > 0:
            lv.append(cpu_ref.bicubic_half(lv[l - 1]))
        dec = decisions[l] if decisions is not None else None
        f = feats(lv[l], weights, dec)
        content = F.mse_loss(tg.content, f[content_i].squeeze(0), reduction="mean")
        style = 0.0
        for i in style_set:
            style = style + torch.tensor(np.float32(w6[i])) * F.mse_loss(tg.grams[i][0], cpu_ref.gram_matrix(f[i])[0], reduction="mean")
        style = style / len(style_set)
        tv = cpu_ref.total_variation(lv[l], dec.tv if dec is not None else None)
        t = cw * content + sw * style + tvw * tv
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
    total.backward()
    return total.detach(), x.grad.detach(), rows


def device_decisions(e, xd, weights, taps=DEFAULT, feats=cpu_ref.vgg19_features, expand=None):
    """cpu_ref.Decisions of the closure the engine evaluated last.  Layers above the deepest map in use were not written by
    it: their decisions are the restatement's own on the device's level image (they feed no loss term)."""
    top = max(TAP_LAYER[taps[0]], *(TAP_LAYER[i] for i in taps[1]))
    out = []
    for l in range(e.levels):
        img = (xd if l == 0 else e.level_image(l)).cpu().reshape(1, -1, *e.level_shape(l))
        if expand is not None:
            img = expand(img)
        acts = [a.cpu() for a in e.level_activations(l)]
        if top < len(acts) - 1:
            rec = []
            with torch.no_grad():
                feats(img, weights, record=rec)
            acts = [a if k <= top else torch.relu(rec[k]) for k, a in enumerate(acts)]
        out.append(cpu_ref.Decisions(acts, img))
    return out


def held_to_restatement(e, xt, targets, weights, what, w6=ONES, taps=DEFAULT, feats=cpu_ref.vgg19_features, weightings=WEIGHTINGS):
    """The device closure against the restatement under the device's decisions, for each weighting: total 1e-5, rows 2e-5
    (check_rows), gradient rel-L2 < GRAD_TOL; every figure is printed before it is asserted."""
    xd = dev(xt)
    nlev = e.levels
    for name, (cw, sw, tvw) in weightings:
        grad, losses = e.closure(xd, cw, sw, tvw)
        dec = device_decisions(e, xd, weights, taps, feats)
        losses = losses.cpu().numpy()
        loss, g_ref, rows = restated_closure(xt, targets, weights, cw, sw, tvw, w6, taps, dec, feats)
        e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
        e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
        report(f"style blend {what} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_l < 1e-5, (what, name, e_l)
        check_rows(losses[:-1].reshape(nlev, 4), np.array(rows), 2e-5, cw, sw, tvw)
        assert e_g < GRAD_TOL, (what, name, e_g)


# ---- 1. default weights and K = 1 are today's bits ----------------------------------------------------------------------
def _launch_list(e, x):
    e.set_timing(2)
    try:
        e.closure(x, CW, SW, TVW)
        torch.cuda.synchronize()
        return e.last_closure_launches()
    finally:
        e.set_timing(0)


@pytest.mark.parametrize("mode", list(MODES))
def test_unit_weights_and_one_style_are_bitwise_the_plain_closure(engines, golden, mode):
    """set_style_weights([1]*6) and set_targets_blend(..., [style], [[c]*6]) for c in {1, 0.37}: loss row and gradient are the
    bits of the closure after plain set_targets; and the closure's launch list (count, order, kernel shapes) is unchanged."""
    fx = golden("closure_64x96_L1")
    e = engines(mode)
    c, s = [fx["content0"], fx["content1"]], [fx["style0"], fx["style1"]]
    x = _prep(fx["x_img"])
    _configure(e, c)
    _set_plain(e, c, s)
    g0, l0 = (t.clone() for t in e.closure(x, CW, SW, TVW))
    plain = _launch_list(e, x)
    e.set_style_weights([1] * 6)
    assert e.style_weights() == ONES
    g, l = e.closure(x, CW, SW, TVW)
    assert _same_bits(g, g0) and _same_bits(l, l0)
    for cval in (1.0, 0.37):
        _set_blend(e, c, [s], [[cval] * 6])
        g, l = e.closure(x, CW, SW, TVW)
        assert _same_bits(g, g0) and _same_bits(l, l0), (mode, cval)
    after = _launch_list(e, x)
    assert after == plain and len(after) > 0
    if mode == "f16x2":
        assert sum(1 for r in after if r["cls"] == 0) == 24             # 12 forward + 12 input-gradient launches, all levels each


# ---- 2. blend against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["K2_uniform_L1", "K3_per_map_L1", "K2_uniform_50x76", "K3_per_map_50x76"])
def test_blend_vs_restatement(eng, vgg_weights, job1, job2, case):
    c, styles, xt = job2 if case.endswith("L1") else job1
    K, B = (2, B2_UNIFORM) if case.startswith("K2") else (3, B3_PER_MAP)
    styles = styles[:K]
    _configure(eng, c)
    _set_blend(eng, c, styles, B)
    tg = [restated_targets(cpu_ref.prepare_img(c[l]), [cpu_ref.prepare_img(s[l]) for s in styles], B, vgg_weights)
          for l in range(len(c))]
    held_to_restatement(eng, xt, tg, vgg_weights, case)


# ---- 3. linearity, on the device alone ---------------------------------------------------------------------------------------
def test_blend_gradient_is_linear_in_the_blend(eng, job2):
    """cw = tvw = 0: S = coef (G - Gt) is affine in Gt, so the gradient under blend (a, 1 - a) of A and B is
    a g_A + (1 - a) g_B (same image, same decisions: one forward)."""
    c, styles, xt = job2
    A, Bs = styles[0], styles[1]
    x = dev(xt)
    _configure(eng, c)
    g = {}
    for name, (st, B) in {"A": ([A], [1.0]), "B": ([Bs], [1.0]), "mix": ([A, Bs], [0.3, 0.7])}.items():
        _set_blend(eng, c, st, B)
        g[name] = eng.closure(x, 0.0, SW, 0.0)[0].double().cpu().numpy()
    err = rel_l2(g["mix"], 0.3 * g["A"] + 0.7 * g["B"])
    report(f"style blend linearity: |g(0.3 A + 0.7 B) - (0.3 g_A + 0.7 g_B)| / |.| = {err:.2e}")
    assert err < GRAD_TOL
    assert rel_l2(g["A"], g["B"]) > 1e-2                 # (the two styles do pull differently)


def test_blending_an_image_with_itself_gives_its_targets(eng, job2):
    """0.3 A + 0.7 A: the targets are A's to rounding - seen through the closure (the context does not hand its targets
    out): style rows to rtol 1e-6, gradient to the gradient bound."""
    c, styles, xt = job2
    x = dev(xt)
    _configure(eng, c)
    _set_plain(eng, c, styles[0])
    g0, l0 = (t.clone() for t in eng.closure(x, 0.0, SW, 0.0))
    _set_blend(eng, c, [styles[0], styles[0]], [0.3, 0.7])
    g, l = eng.closure(x, 0.0, SW, 0.0)
    np.testing.assert_allclose(l.cpu().numpy(), l0.cpu().numpy(), rtol=1e-6)
    assert rel_l2(g.cpu().numpy(), g0.cpu().numpy()) < GRAD_TOL


# ---- 4. layer weights against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [DEFAULT, (2, (2, 3))], ids=["default_taps", "c2_s23"])
def test_layer_weights_vs_restatement(eng, vgg_weights, job2, taps):
    c, styles, xt = job2
    s = styles[0]
    _configure(eng, c)
    eng.set_taps(taps[0], list(taps[1]))
    eng.set_style_weights(W_MIXED)
    _set_plain(eng, c, s)
    tg = [restated_targets(cpu_ref.prepare_img(c[l]), [cpu_ref.prepare_img(s[l])], [ONES], vgg_weights, taps) for l in range(2)]
    held_to_restatement(eng, xt, tg, vgg_weights, f"layer weights, taps {taps}", W_MIXED, taps)


# ---- 5. layer-weight identities ---------------------------------------------------------------------------------------------
def test_doubled_weights_are_a_doubled_style_weight(eng, job2):
    c, styles, xt = job2
    x = dev(xt)
    _configure(eng, c)
    _set_plain(eng, c, styles[0])
    g1, l1 = (t.clone() for t in eng.closure(x, CW, 2.0 * SW, TVW))
    eng.set_style_weights([2.0] * 6)
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert _same_bits(g1, g2)
    assert float(l2[-1]) == pytest.approx(float(l1[-1]), rel=1e-6)


@pytest.mark.parametrize("i", [0, 5])
def test_one_hot_weights_are_a_one_map_style_set(eng, job2, i):
    """w = nstyle e_i on the default taps = taps style=(i,) with w = 1, under the job's weighting (CW, SW, TVW): the content
    and TV terms are the same on both sides.  (Not with the style term alone: with cw = 0 and map 0 the only map that counts,
    the gradient that reaches conv1_2 from above is exactly zero on BOTH sides, and the f16x2 input-gradient launch that
    carries a Gram term on top of an all-zero main gradient returns non-finite values - so does the parent commit under
    nst_job_set_taps(ctx, 5, 0x01, 1) with the style term alone.  conv_h2.hip is outside this change; DESIGN 4.5 records it.)"""
    c, styles, xt = job2
    x = dev(xt)
    _configure(eng, c)
    _set_plain(eng, c, styles[0])
    eng.set_style_weights([5.0 if k == i else 0.0 for k in range(6)])
    g_w, l_w = (t.clone() for t in eng.closure(x, CW, SW, TVW))
    eng.reset_style_weights()
    eng.set_taps(4, [i])
    _set_plain(eng, c, styles[0])
    g_t, l_t = eng.closure(x, CW, SW, TVW)
    assert bool(torch.isfinite(g_w).all()) and bool(torch.isfinite(g_t).all())
    err = rel_l2(g_w.cpu().numpy(), g_t.cpu().numpy())
    report(f"one-hot weights on map {i} vs style set ({i},): gradient rel-L2 {err:.2e}")
    assert err < GRAD_TOL
    rows_w, rows_t = l_w.cpu().numpy()[:-1].reshape(2, 4), l_t.cpu().numpy()[:-1].reshape(2, 4)
    np.testing.assert_allclose(rows_w[:, 2], rows_t[:, 2], rtol=1e-6)


# ---- 6. life cycle ------------------------------------------------------------------------------------------------------
def test_weight_change_between_lbfgs_steps_forces_an_evaluation(eng, vgg_weights, job2):
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine
    c, styles, xt = job2
    _configure(eng, c)
    _set_plain(eng, c, styles[0])
    x = dev(xt).clone()
    opt = PixelOptimizer(eng, "lbfgs", 10.0, 1)
    try:
        opt.step(x, CW, SW, TVW)
        before = opt.closure_stats()
        opt.step(x, CW, SW, TVW)
        ev, sv = opt.closure_stats()
        assert sv == before[1] + 1                         # nothing changed: the first closure of the step was served
        eng.set_style_weights(W_MIXED)
        x_at = x.clone()
        info, rows = opt.step(x, CW, SW, TVW)
        ev2, sv2 = opt.closure_stats()
        assert sv2 == sv and ev2 > ev                      # evaluated, not served
    finally:
        opt.close()
    fresh = StyleEngine(vgg_weights, 0)
    try:
        _configure(fresh, c)
        fresh.set_style_weights(W_MIXED)
        _set_plain(fresh, c, styles[0])
        _, l = fresh.closure(x_at, CW, SW, TVW)
        assert np.array_equal(np.asarray(rows[0], np.float32).view(np.uint32), l.cpu().numpy().view(np.uint32))
        assert info.loss == float(l[-1])
    finally:
        fresh.close()


def test_backward_half_is_stale_after_set_style_weights(eng, job2):
    from artstyletransfer_amd import _lib
    c, styles, xt = job2
    x = dev(xt)
    _configure(eng, c)
    _set_plain(eng, c, styles[0])
    g_ref, _ = eng.closure(x, CW, SW, TVW)
    g_ref = g_ref.clone()
    grad = torch.full_like(g_ref, -7.0)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_style_weights(ONES)                            # even the same weights
    rc = eng.lib.nst_closure_backward(eng.ctx, C.c_void_p(x.data_ptr()), CW, SW, TVW, 0xFFFFFFFF, C.c_void_p(grad.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.NST_E_STATE and bool((grad == -7.0).all())
    # targets survived the setter, and the context goes on working
    g, _ = eng.closure(x, CW, SW, TVW)
    assert _same_bits(g, g_ref)


def test_bad_arguments_are_refused_and_the_context_stays_usable(eng, job2):
    from artstyletransfer_amd import _lib
    c, styles, xt = job2
    x = dev(xt)
    _configure(eng, c)
    _set_plain(eng, c, styles[0])
    g_ref, l_ref = (t.clone() for t in eng.closure(x, CW, SW, TVW))
    lib, stream = eng.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    content, sA, sB = _prep(c[0]).reshape(3, 64, 96), _prep(styles[0][0]).reshape(3, 48, 80), _prep(styles[1][0]).reshape(3, 50, 76)

    def blend(K, B):
        n = max(K, 1)
        imgs = [sA, sB] + [sA] * 7
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in imgs[:n]])
        hs = (C.c_int * n)(*[t.shape[1] for t in imgs[:n]])
        ws = (C.c_int * n)(*[t.shape[2] for t in imgs[:n]])
        flat = (C.c_float * (n * 6))(*np.asarray(B, np.float32).reshape(-1)[:n * 6])
        return lib.nst_level_set_targets_blend(eng.ctx, 0, C.c_void_p(content.data_ptr()), K, ptrs, hs, ws, flat, stream)

    def weights(w):
        return lib.nst_job_set_style_weights(eng.ctx, (C.c_float * 6)(*w))

    zero_col = [[1, 1, 0, 1, 1, 1], [1, 1, 0, 1, 1, 1]]                      # map 2 is in the style set
    assert blend(2, zero_col) == _lib.NST_E_ARG
    assert blend(0, [[1] * 6]) == _lib.NST_E_ARG
    assert blend(9, [[1] * 6] * 9) == _lib.NST_E_ARG
    assert blend(2, [[1] * 6, [1, -1, 1, 1, 1, 1]]) == _lib.NST_E_ARG
    assert blend(2, [[1] * 6, [1, float("nan"), 1, 1, 1, 1]]) == _lib.NST_E_ARG
    assert weights([1, 1, -0.5, 1, 1, 1]) == _lib.NST_E_ARG
    assert weights([0] * 6) == _lib.NST_E_ARG
    assert weights([0, 0, 0, 0, 3.0, 0]) == _lib.NST_E_ARG                   # map 4 is not in the default style set
    assert weights([1, float("inf"), 1, 1, 1, 1]) == _lib.NST_E_ARG
    assert eng.style_weights() == ONES
    # a column of a map OUTSIDE the style set may be zero
    assert blend(2, [[1, 1, 1, 1, 0, 1], [1, 1, 1, 1, 0, 1]]) == 0
    _set_plain(eng, c, styles[0])
    g, l = eng.closure(x, CW, SW, TVW)
    assert _same_bits(g, g_ref) and _same_bits(l, l_ref)
    with pytest.raises(ValueError):
        eng.set_style_weights([1] * 5)
    with pytest.raises(ValueError):
        eng.set_targets_blend(0, content, [sA, sB], [1.0])
    # a style set without a positive weight is refused by set_taps too, and the weights survive a set_taps
    eng.set_style_weights([1, 0, 0, 1, 1, 1])
    assert lib.nst_job_set_taps(eng.ctx, 4, 0b000110, 1) == _lib.NST_E_ARG
    eng.set_taps(4, [0, 1])
    assert eng.style_weights() == (1.0, 0.0, 0.0, 1.0, 1.0, 1.0)


def test_pooled_engine_comes_back_with_unit_weights(vgg_weights):
    from artstyletransfer_amd import neural_nets
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 64, 96)
    e.set_style_weights([0, 0, 0, 2.0, 1, 0])
    e.set_taps(4, [3])
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.style_weights() == ONES and again.layer_weights == ONES
    finally:
        neural_nets.return_engine(again)


def test_stripe_closure_refuses_weights_and_honours_a_blend(vgg_weights, job2):
    """nst_window_*: NST_E_STATE under any weight != 1; its Gram targets are the level's, so a blend is honoured - the
    whole image as one stripe gives the closure's style row."""
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine
    c, styles, xt = job2
    x = dev(xt)
    e = StyleEngine(vgg_weights, 0)
    try:
        e.configure(1, 64, 96)
        e.set_targets_blend(0, _prep(c[0]), [_prep(styles[0][0]), _prep(styles[1][0])], [0.25, 0.75])
        _, l = e.closure(x, CW, SW, TVW)
        row = l.cpu().numpy()[:4]
        sums = e.window_begin(x, 0, 64, 64)
        _, lw = e.window_end(x, 0, 64, 64, CW, SW, TVW, sums)
        np.testing.assert_allclose(lw.cpu().numpy()[2], row[2], rtol=1e-5)
        e.set_targets(0, _prep(c[0]), _prep(styles[0][0]))
        _, l_single = e.closure(x, CW, SW, TVW)
        assert abs(float(l_single[2]) - row[2]) > 1e-2 * row[2]
        e.set_style_weights([1, 1, 1, 2, 1, 1])
        with pytest.raises(NstError, match=r"\(-2\).*unit style layer weights"):
            e.window_begin(x, 0, 64, 64)
        opt = PixelOptimizer(e, "adam", 10.0)
        try:
            with pytest.raises(ValueError):
                opt.shard_stripes(0, 1, vgg_weights, _prep(c[0]), _prep(styles[0][0]))
        finally:
            opt.close()
    finally:
        e.close()


# ---- 7. composition ----------------------------------------------------------------------------------------------------
def test_blend_and_weights_under_avg_pooling(eng, vgg_weights, job2):
    c, styles, xt = job2
    styles = styles[:2]
    _configure(eng, c)
    eng.set_pooling("avg")
    eng.set_style_weights(W_MIXED)
    _set_blend(eng, c, styles, B2_UNIFORM)
    tg = [restated_targets(cpu_ref.prepare_img(c[l]), [cpu_ref.prepare_img(s[l]) for s in styles], B2_UNIFORM, vgg_weights,
                           feats=avg_features) for l in range(2)]
    held_to_restatement(eng, xt, tg, vgg_weights, "avg pooling", W_MIXED, feats=avg_features, weightings=WEIGHTINGS[2:])


def test_blend_and_weights_in_luminance_mode(eng, vgg_weights, job2):
    """One plane u: the closure is the RGB restatement at E(u) = u - mean_c, the gradient summed over the channels."""
    from artstyletransfer_amd import host_image
    mean = torch.tensor(cpu_ref.IMAGENET_MEAN_255, dtype=torch.float32).view(1, 3, 1, 1)
    E = lambda u: u.reshape(1, 1, *u.shape[-2:]).float().cpu() - mean      # noqa: E731
    c, styles, _ = job2
    styles = styles[:2]
    lum = lambda img: torch.from_numpy(host_image.luminance(img))           # noqa: E731
    _configure(eng, c)
    eng.set_color("luminance")
    eng.set_style_weights(W_MIXED)
    for l in range(2):
        eng.set_targets_blend(l, dev(lum(c[l])), [dev(lum(s[l])) for s in styles], B2_UNIFORM)
    tg = [restated_targets(E(lum(c[l])), [E(lum(s[l])) for s in styles], B2_UNIFORM, vgg_weights) for l in range(2)]
    u = lum((0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(64, 96, seed=9)).astype(np.float32)).reshape(1, 1, 64, 96)
    ud = dev(u)
    grad, losses = eng.closure(ud, CW, SW, TVW)
    assert tuple(grad.shape) == (1, 1, 64, 96)
    dec = device_decisions(eng, ud, vgg_weights, expand=E)
    loss, g_ref, rows = restated_closure(E(u), tg, vgg_weights, CW, SW, TVW, W_MIXED, decisions=dec)
    losses = losses.cpu().numpy()
    e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_ref.sum(dim=1).numpy().reshape(64, 96))
    report(f"style blend luminance: total rel {abs(float(losses[-1]) - float(loss)) / float(loss):.2e}, gradient rel-L2 {e_g:.2e}")
    assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
    check_rows(losses[:-1].reshape(2, 4), np.array(rows), 2e-5)
    assert e_g < GRAD_TOL


def test_blend_and_weights_level_sharded_closure_adds_up(eng, job2):
    c, styles, xt = job2
    x = dev(xt)
    _configure(eng, c)
    eng.set_style_weights(W_MIXED)
    _set_blend(eng, c, styles, B3_PER_MAP)
    g, l = (t.clone() for t in eng.closure(x, CW, SW, TVW))
    g0, l0 = (t.clone() for t in eng.closure_levels(x, CW, SW, TVW, 0b01))
    g1, l1 = eng.closure_levels(x, CW, SW, TVW, 0b10)
    assert rel_l2((g0 + g1).cpu().numpy(), g.cpu().numpy()) < 1e-6
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    np.testing.assert_allclose(l0.cpu().numpy()[:4], rows[0], rtol=1e-6)
    np.testing.assert_allclose(l1.cpu().numpy()[4:8], rows[1], rtol=1e-6)
    assert not l0.cpu().numpy()[4:8].any() and not l1.cpu().numpy()[:4].any()


# ---- 8. the job driver ---------------------------------------------------------------------------------------------------
def test_job_driver_with_a_blend_and_layer_weights(vgg_weights):
    """Six Adam steps at the smallest job geometry the driver tests use (levels_num = 1: 256x384): finite, not the
    single-style run's image, and run twice the same bits."""
    from artstyletransfer_amd import config, neural_nets
    import neural_style_transfer as nst
    neural_nets.set_weights(vgg_weights)
    content = cpu_ref.synthetic_image(64, 96, seed=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    other = cpu_ref.synthetic_image(50, 76, seed=3)
    cfg = config.Config(levels_num=1, iters_num=6, optimizer="adam")

    def run(**kw):
        async def go():
            out = []
            async for percent, img in nst.neural_style_transfer(
                    nst.ContentStylePair(("c", content), ("s", style)), cfg.content_weight, cfg.style_weight, cfg.tv_weight,
                    cfg.optimizer, cfg.model, "content", cfg.iters_num, cfg.levels_num, cfg.noise_factor,
                    cfg.noise_levels, cfg.noise_levels_central_amplitude, cfg.noise_levels_peripheral_amplitude,
                    cfg.noise_levels_dispersion, **kw):
                out.append((percent, img))
            return out
        return asyncio.run(go())

    kw = dict(extra_styles=[other], style_blend=[0.5, 0.5], style_layer_weights={0: 2.0})
    a, b, single = run(**kw), run(**kw), run()
    assert len(a) == 6 and round(a[-1][0]) == 100
    for _, img in a:
        assert img.shape == (256, 384, 3) and np.isfinite(img).all()
    assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for (_, p), (_, q) in zip(a, b))
    assert np.abs(a[-1][1] - single[-1][1]).max() > 1e-3
