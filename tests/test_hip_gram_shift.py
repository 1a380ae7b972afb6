"""GPU: the Gram shift option (nst_job_set_gram_shift) - activation-shifted and mean-centred Gram matrices.
1. the statistic alone (nst_gram_shifted) against an fp64 evaluation of the same formula, held to torch-fp32's own error;
2. the closure under equal decisions, per term and summed, against the oracle with cpu_ref.gram_matrix replaced by a
   test-local shifted / centred one (monkeypatch: no oracle edit), at hip_helpers' standing tolerances;
3. the paths a style gradient takes (per-level walker, average pooling, pre-ReLU taps, content map = style map, layer
   weights, luminance, blends); 4. identities; 5. off means off, life cycle, refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hip_helpers import (CW, SW, TVW, check_rows, closure_vs_oracle_under_equal_decisions, dev,
                         levels as _levels, oracle_targets, rel_l2, report)
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

MAP_C = (64, 128, 256, 512, 512, 512)          # channels of the six maps of Vgg19.layer_names
TAP_LAYER = (0, 2, 4, 8, 9, 12)
MEAN = "mean"


# ---- the statistic restated ----------------------------------------------------------------------------------------------
def shifted_gram(x, setting, should_normalize=True):
    """G = (F + o)(F + o)^T / (C N) of a (b,C,h,w) map in x's dtype; setting: a number (o = that) or "mean" (o = -mu(F))."""
    b, ch, h, w = x.shape
    f = x.reshape(b, ch, h * w)
    f = f - f.mean(dim=2, keepdim=True) if setting == MEAN else f + float(setting)
    g = f.bmm(f.transpose(1, 2))
    return g / (ch * h * w) if should_normalize else g


class PatchedGram:
    """cpu_ref.gram_matrix with a per-map setting.  LevelTargets and level_loss call it once per map of cpu_ref.STYLE_INDICES,
    in that order, so the call count gives the map (three maps have 512 channels: the channel count alone does not).
    `order`: the cycle of map indices of a caller that walks the maps differently (expect(order) restarts the count)."""

    def __init__(self, settings):
        self.settings, self.n, self.order = tuple(settings), 0, None

    def expect(self, order=None):
        self.order, self.n = (tuple(order) if order is not None else None), 0

    def __call__(self, x, should_normalize=True):
        idx = self.order or cpu_ref.STYLE_INDICES
        i = idx[self.n % len(idx)]
        self.n += 1
        assert x.shape[1] == MAP_C[i], (i, tuple(x.shape))
        return shifted_gram(x, self.settings[i], should_normalize)


def engine_setting(settings):
    return [0.0 if s == MEAN else float(s) for s in settings], sum(1 << i for i, s in enumerate(settings) if s == MEAN)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_per_level(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, batched=False)
    yield e
    e.close()


# ---- 1. the statistic alone ----------------------------------------------------------------------------------------------
def _map(c, h, w, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((1, c, h, w), generator=g)
    if kind == "relu":                      # post-ReLU-like: non-negative, sparse, channel means that differ
        x = torch.relu(x - 0.5) * (1.0 + torch.arange(c, dtype=torch.float32).view(1, c, 1, 1) / c) * 3.0
    else:                                   # signed, with an offset per channel
        x = x * 2.0 + torch.linspace(-1.5, 1.5, c).view(1, c, 1, 1)
    return x.contiguous()


# 181x183 = 33123 pixels: more than one chunk per split at every channel count; every N is off a multiple of 8
SHAPES = [(1, 4), (5, 7), (17, 65), (31, 63), (181, 183)]


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_statistic_vs_fp64(eng, c, h, w):
    """Device and torch-fp32 against fp64, same formula: device <= max(3 x torch's own error, 2e-6) rel-L2; offsets against the
    fp64 means to 1e-6 (absolute); exact symmetry."""
    assert (h * w) % 8 != 0
    for kind in ("relu", "signed"):
        x = _map(c, h, w, kind, seed=c + h)
        xd = dev(x)
        for setting in (-1.0, MEAN):
            ref = shifted_gram(x.double(), setting)[0]
            e32 = rel_l2(shifted_gram(x, setting)[0].numpy(), ref.numpy())
            g, o = eng.gram_shifted(xd, 0.0 if setting == MEAN else setting, center=setting == MEAN)
            g = g[0].cpu()
            e_dev = rel_l2(g.numpy(), ref.numpy())
            report(f"gram_shifted C={c} {h}x{w} {kind} {setting}: device {e_dev:.2e}, torch fp32 {e32:.2e} (vs fp64)")
            assert torch.isfinite(g).all()
            assert e_dev <= max(3.0 * e32, 2e-6), (c, h, w, kind, setting, e_dev, e32)
            assert torch.equal(g, g.t())
            o_ref = -x.double().mean(dim=(0, 2, 3)) if setting == MEAN else torch.full((c,), float(setting), dtype=torch.float64)
            assert float((o.cpu().double() - o_ref).abs().max()) <= 1e-6


@pytest.mark.parametrize("c,h,w", [(64, 17, 65), (128, 5, 7), (512, 31, 63)])
def test_zero_shift_is_bitwise_the_plain_gram(eng, c, h, w):
    xd = dev(_map(c, h, w, "relu", seed=5))
    g, o = eng.gram_shifted(xd, 0.0, center=False)
    assert np.array_equal(_bits(g), _bits(eng.gram(xd))) and torch.count_nonzero(o) == 0


@pytest.mark.parametrize("amp", [1.0, 4.0, 64.0, 1024.0])
def test_shifted_operand_bound_crosses_an_exponent(eng, amp):
    """Signed data whose absmax sits just below a power of two: F's own record is one exponent short of |F + o| for the
    shift and of |F - mu| for centring.  No inf / NaN, and the accuracy of the other cases."""
    g = torch.Generator().manual_seed(11)
    x = (torch.rand((1, 128, 17, 65), generator=g) * 2.0 - 1.0) * (amp * 0.999)
    x[0, :, 0, 0] = amp * 0.999                       # the absmax itself, on every channel
    # every other channel sits at -absmax on 19 pixels of 20 and at +absmax on the rest: mu is near -absmax, |F - mu| near
    # twice absmax(F) - one exponent beyond what F's own record says
    low = (torch.arange(17 * 65).view(17, 65) % 20 != 0)
    x[0, ::2] = torch.where(low, torch.tensor(-amp * 0.999), torch.tensor(amp * 0.999))
    xd = dev(x)
    for setting in (-0.6 * amp, MEAN):
        ref = shifted_gram(x.double(), setting)[0]
        e32 = rel_l2(shifted_gram(x, setting)[0].numpy(), ref.numpy())
        got, _ = eng.gram_shifted(xd, 0.0 if setting == MEAN else setting, center=setting == MEAN)
        got = got[0].cpu()
        assert torch.isfinite(got).all(), (amp, setting)
        e_dev = rel_l2(got.numpy(), ref.numpy())
        report(f"gram_shifted bound amp={amp} {setting}: device {e_dev:.2e}, torch fp32 {e32:.2e}")
        assert e_dev <= max(3.0 * e32, 2e-6), (amp, setting, e_dev, e32)


def test_statistic_refusals(eng):
    from artstyletransfer_amd._lib import NstError
    xd = dev(_map(64, 5, 7, "relu", seed=1))
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.gram_shifted(xd, float("nan"))
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.gram_shifted(xd, 1.0, center=True)
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.gram_shifted(dev(_map(96, 5, 7, "relu", seed=1)), -1.0)


# ---- 2. the closure under equal decisions ---------------------------------------------------------------------------------
JOBS = {"50x76_L0": (50, 76, 1), "64x96_L1": (64, 96, 2), "68x260_L2": (68, 260, 3)}


def _job(name):
    h, w, nlev = JOBS[name]
    if name == "50x76_L0":
        # the one-level job of the closure_50x76_L0 fixture (content, style and start image of the reference's own run): the
        # plain closure is held on these inputs by test_hip_parity, near-tie caps included
        fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "closure_50x76_L0.npz"), allow_pickle=False)
        return [fx["content0"]], [fx["style0"]], cpu_ref.prepare_img(fx["x_img"])
    c, s = _levels(h, w, nlev, 1), _levels(h + 6, w + 14, nlev, 2)
    xt = cpu_ref.prepare_img((0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32))
    return c, s, xt


def _half_mean_shifts(xt, weights, feats=cpu_ref.vgg19_features):
    """Setting (a): per map -1/2 x that map's mean on the start image, from the oracle's features."""
    with torch.no_grad():
        return tuple(-0.5 * float(f.double().mean()) for f in feats(xt, weights))


def _settings(kind, xt, weights):
    if kind == "a":
        return _half_mean_shifts(xt, weights)
    if kind == "b":
        return (MEAN,) * 6
    return (MEAN, 0.0, -1.0, MEAN, 0.0, 0.0)          # (c): two maps centred, one shifted, the rest 0


def _style_loss(xt, contents, styles, weights, nlev):
    tg = oracle_targets(contents, styles, weights)
    _, _, rows = cpu_ref.closure_eval(xt, tg, weights, 0.0, SW, 0.0)
    return tg, float(sum(r[2] for r in rows[:nlev]))


def _shift_setup(e, contents, styles, settings, targets=True):
    h, w = contents[0].shape[:2]
    e.configure(len(contents), h, w)
    e.set_gram_shift(*engine_setting(settings))
    for i in range(len(contents)):
        if targets:
            e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))


def _differs_from_plain(monkeypatch, xt, c, s, weights, settings):
    """On the CPU: the patched oracle's style loss differs from the plain one by more than 10 % - a build that ignores the
    setting cannot pass.  Leaves cpu_ref.gram_matrix patched and returns the patched targets."""
    _, plain = _style_loss(xt, c, s, weights, len(c))
    monkeypatch.setattr(cpu_ref, "gram_matrix", PatchedGram(settings))
    tg, shifted = _style_loss(xt, c, s, weights, len(c))
    report(f"style loss plain {plain:.4e}, under the setting {shifted:.4e}")
    assert abs(shifted - plain) > 0.1 * plain, (plain, shifted)
    return tg


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("name", list(JOBS))
def test_closure_vs_patched_oracle_under_equal_decisions(eng, vgg_weights, monkeypatch, name, kind):
    """Losses 1e-5, gradient 2e-5 under the device's decisions, near-ties 2e-5 of rms: hip_helpers' standing tolerances.
    50x76 L0 runs the per-level walker (one small level), the others the batched one; 68x260 L2 has maps 17x65 ... 1x4."""
    c, s, xt = _job(name)
    settings = _settings(kind, xt, vgg_weights)
    tg = _differs_from_plain(monkeypatch, xt, c, s, vgg_weights, settings)
    _shift_setup(eng, c, s, settings)
    closure_vs_oracle_under_equal_decisions(eng, xt, tg, vgg_weights, f"gram shift ({kind}) {name}")


# ---- 3. paths --------------------------------------------------------------------------------------------------------------
def _strict(e, monkeypatch, vgg_weights, what, settings=None, prepare=None):
    c, s, xt = _job("64x96_L1")
    settings = settings or _settings("c", xt, vgg_weights)
    tg = _differs_from_plain(monkeypatch, xt, c, s, vgg_weights, settings)
    h, w = c[0].shape[:2]
    e.configure(2, h, w)
    if prepare:
        prepare(e)
    e.set_gram_shift(*engine_setting(settings))
    for i in range(2):
        e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, what)


def test_path_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _strict(eng_per_level, monkeypatch, vgg_weights, "gram shift (c) per-level walker")


def test_path_average_pooling(eng, vgg_weights, monkeypatch):
    from test_hip_pooling import avg_vgg19_features
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "gram shift (c) avg pooling", prepare=lambda e: e.set_pooling("avg"))
    finally:
        eng.reset_pooling()


def prerelu_vgg19_features(x, weights, decisions=None, record=None):
    """cpu_ref.vgg19_features of the use_relu=False flavour as the job taps it: map 5 is conv5_1 BEFORE its ReLU."""
    outs = []
    for li, ((name, _, _), (w, b)) in enumerate(zip(cpu_ref.VGG19_CONVS, weights)):
        pre = F.conv2d(x, w, b, stride=1, padding=1)
        if record is not None:
            record.append(pre.detach())
        x = F.relu(pre) if decisions is None else pre * decisions.relu[li].to(pre.dtype)
        if name in cpu_ref.TAPS:
            outs.append(pre if li == len(cpu_ref.VGG19_CONVS) - 1 else x)
        if name in cpu_ref.POOL_AFTER:
            if decisions is None:
                x = F.max_pool2d(x, kernel_size=2, stride=2)
            else:
                idx = decisions.pool[name]
                x = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    return outs


def test_path_pre_relu_taps(eng, vgg_weights, monkeypatch):
    """use_relu = False: the top map is conv5_1 before its ReLU, signed - its style gradient, r included, joins unmasked,
    and centring it needs the bound of the shifted operand."""
    monkeypatch.setattr(cpu_ref, "vgg19_features", prerelu_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "gram shift pre-ReLU taps", settings=(MEAN, 0.0, -1.0, 0.0, 0.0, MEAN),
                prepare=lambda e: e.set_taps(4, [0, 1, 2, 3, 5], use_relu=False))
    finally:
        eng.reset_taps()


def _held_to_restatement(e, xt, targets, weights, patched, what, w6, taps, expand=None):
    """The device closure against test_hip_style_blend's restatement (blended targets, layer weights, any taps) under the
    device's decisions, with its gram_matrix patched: total 1e-5, rows 2e-5, the whole gradient 2e-5."""
    from test_hip_style_blend import device_decisions as decisions_of, restated_closure
    xd = dev(xt)
    for name, (cw, sw, tvw) in (("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW))):
        grad, losses = e.closure(xd, cw, sw, tvw)
        dec = decisions_of(e, xd, weights, taps)
        losses = losses.cpu().numpy()
        patched.expect(taps[1])
        loss, g_ref, rows = restated_closure(xt, targets, weights, cw, sw, tvw, w6, taps, dec)
        e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
        e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
        report(f"gram shift {what} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_l < 1e-5, (what, name, e_l)
        check_rows(losses[:-1].reshape(e.levels, 4), np.array(rows), 2e-5, cw, sw, tvw)
        assert e_g < 2e-5, (what, name, e_g)


def test_path_content_map_is_a_style_map_and_unequal_layer_weights(eng, vgg_weights, monkeypatch):
    """style_mask = 0x3F: the content map conv4_2 is a style map too (second K source, row bias and content addend on one
    launch), centred here; with unequal layer weights, against the weighted restatement of the style tests."""
    from test_hip_style_blend import restated_targets
    lw = (0.5, 2.0, 1.0, 0.25, 3.0, 1.5)
    taps = (4, (0, 1, 2, 3, 4, 5))
    settings = (MEAN, 0.0, -1.0, 0.0, MEAN, -0.5)
    c, s, xt = _job("64x96_L1")
    patched = PatchedGram(settings)
    monkeypatch.setattr(cpu_ref, "gram_matrix", patched)
    prep = cpu_ref.prepare_img
    try:
        eng.configure(2, 64, 96)
        eng.set_taps(4, [0, 1, 2, 3, 4, 5])
        eng.set_style_weights(lw)
        eng.set_gram_shift(*engine_setting(settings))
        tg = []
        for i in range(2):
            eng.set_targets(i, dev(prep(c[i])), dev(prep(s[i])))
            patched.expect(taps[1])
            tg.append(restated_targets(prep(c[i]), [prep(s[i])], ((1.0,) * 6,), vgg_weights, taps))
        _held_to_restatement(eng, xt, tg, vgg_weights, patched, "0x3F + layer weights", lw, taps)
    finally:
        eng.reset_style_weights()
        eng.reset_taps()


def test_path_luminance(eng, vgg_weights, monkeypatch):
    """The luminance closure with the setting = the patched oracle's closure at E(u), gradient summed over the channels."""
    from artstyletransfer_amd import host_image
    from test_hip_color import expand, lum_decisions, lum_targets, start_u
    c, s = _levels(64, 96, 2, 1), _levels(70, 110, 2, 2)
    settings = (MEAN, 0.0, -1.0, MEAN, 0.0, 0.0)
    monkeypatch.setattr(cpu_ref, "gram_matrix", PatchedGram(settings))
    try:
        eng.configure(2, 64, 96)
        eng.set_color("luminance")
        eng.set_gram_shift(*engine_setting(settings))
        alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
        cu, su = lum_targets(c, s, alpha, beta)
        for i in range(2):
            eng.set_targets(i, dev(torch.from_numpy(cu[i])), dev(torch.from_numpy(su[i])))
        tg = [cpu_ref.LevelTargets(expand(torch.from_numpy(a)), expand(torch.from_numpy(b)), vgg_weights) for a, b in zip(cu, su)]
        u = start_u(c[0])
        ud = dev(u.reshape(1, 1, 64, 96))
        xt = expand(u)
        grad, losses = eng.closure(ud, CW, SW, TVW)
        dec = lum_decisions(eng, ud)
        losses = losses.cpu().numpy()
        loss, _, rows = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW)
        assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
        check_rows(losses[:-1].reshape(2, 4), np.array(rows), 1e-5, CW, SW, TVW)
        _, g_eq, _ = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_eq.sum(dim=1).numpy().reshape(64, 96))
        report(f"gram shift luminance: gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_g < 2e-5
    finally:
        eng.reset_color()


def test_path_two_style_blend(eng, vgg_weights, monkeypatch):
    """The target of a blend is the blend of the single-style shifted targets, each style with its own means: the closure
    against the restatement of the style tests (Gt_i = sum_k b^_ki G_i(style_k)) with its gram_matrix patched; and blend
    weights (1, 0) are the single-style job bitwise."""
    from test_hip_style_blend import restated_targets
    c, s1, xt = _job("64x96_L1")
    s2 = _levels(58, 120, 2, 7)
    B = ((0.25,) * 6, (0.75,) * 6)
    taps = (4, (0, 1, 2, 3, 5))
    settings = (MEAN, 0.0, -1.0, MEAN, 0.0, 0.0)
    patched = PatchedGram(settings)
    monkeypatch.setattr(cpu_ref, "gram_matrix", patched)
    prep = cpu_ref.prepare_img
    eng.configure(2, 64, 96)
    eng.set_gram_shift(*engine_setting(settings))
    tg = []
    for i in range(2):
        eng.set_targets_blend(i, dev(prep(c[i])), [dev(prep(s1[i])), dev(prep(s2[i]))], B)
        patched.expect([m for m in taps[1] for _ in range(2)])          # (restated_targets: per map, every style)
        tg.append(restated_targets(prep(c[i]), [prep(s1[i]), prep(s2[i])], B, vgg_weights, taps))
    _held_to_restatement(eng, xt, tg, vgg_weights, patched, "two-style blend", (1.0,) * 6, taps)
    out = []
    for blend in (None, ((1.0,) * 6, (0.0,) * 6)):
        for i in range(2):
            if blend is None:
                eng.set_targets(i, dev(prep(c[i])), dev(prep(s1[i])))
            else:
                eng.set_targets_blend(i, dev(prep(c[i])), [dev(prep(s1[i])), dev(prep(s2[i]))], blend)
        g, l = eng.closure(dev(xt), CW, SW, TVW)
        out.append((_bits(g), _bits(l)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# ---- 4. identities ---------------------------------------------------------------------------------------------------------
def _mixed_job(e, name="64x96_L1"):
    c, s, xt = _job(name)
    _shift_setup(e, c, s, (MEAN, 0.0, -1.0, MEAN, 0.0, 0.0))
    return dev(xt), c, s


def test_halves_equal_the_whole_and_run_to_run_bitwise(eng):
    x, _, _ = _mixed_job(eng)
    g, l = eng.closure(x, CW, SW, TVW)
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_level_masks_add_up(eng, eng_per_level, which):
    e = eng if which == "batched" else eng_per_level
    x, _, _ = _mixed_job(e)
    g, l = e.closure(x, CW, SW, TVW)
    g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    gs, ls = np.zeros_like(g), np.zeros_like(l)
    for mask in (1, 2):
        gm, lm = e.closure_levels(x, CW, SW, TVW, mask)
        gs += gm.cpu().numpy()
        ls += lm.cpu().numpy()
    np.testing.assert_allclose(ls, l, rtol=1e-6)
    err = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
    report(f"gram shift level masks [{which}]: |sum - unsharded| / |.| = {err:.1e}")
    assert err <= 1e-6


def test_lbfgs_is_the_same_with_reuse_and_lazy_backward_on_or_off(eng):
    from artstyletransfer_amd.engine import PixelOptimizer
    x0, _, _ = _mixed_job(eng)
    runs = {}
    for reuse, lazy in ((False, False), (True, True)):
        opt = PixelOptimizer(eng, "lbfgs")
        try:
            opt.set_closure_reuse(reuse)
            opt.set_lazy_backward(lazy)
            x = x0.clone()
            out = []
            for _ in range(5):
                info, rows = opt.step(x, CW, SW, TVW)
                out.append((info.closures, info.total_closures, info.accepted, info.history, rows.view(np.uint32).copy(), _bits(x)))
            runs[(reuse, lazy)] = (out, opt.closure_stats(), opt.backward_stats())
        finally:
            opt.close()
    base = runs[(False, False)][0]
    out, stats, bw = runs[(True, True)]
    for k, (a, b) in enumerate(zip(out, base)):
        assert a[:4] == b[:4], (k, a[:4], b[:4])
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), k
    assert np.isfinite(base[-1][4].view(np.float32)).all()
    # the served / forward-only paths did run under the setting, and only where they are switched on
    assert sum(stats) == base[-1][1] and stats[1] > 0 and bw[0] > 0, (stats, bw)
    _, stats0, bw0 = runs[(False, False)]
    assert stats0[1] == 0 and bw0[0] == 0, (stats0, bw0)


def test_level_gram_offsets_are_the_means_of_the_devices_own_maps(eng):
    """To 1e-6, relative where a mean exceeds 1: o is an fp32 value, and the means of the synthetic network's maps reach
    magnitudes whose half ulp alone is above 1e-6 absolute."""
    x, _, _ = _mixed_job(eng)
    eng.closure(x, CW, SW, TVW)
    for level in range(2):
        for slot, i in enumerate((0, 1, 2, 3, 5)):
            o = eng.level_gram_offsets(level, slot).cpu().double()
            setting = (MEAN, 0.0, -1.0, MEAN, 0.0, 0.0)[i]
            if setting == MEAN:
                act = eng.level_activation(level, TAP_LAYER[i]).cpu().double()
                ref = -act.mean(dim=(0, 2, 3))
            else:
                ref = torch.full((MAP_C[i],), float(setting), dtype=torch.float64)
            assert float((o - ref).abs().max()) <= 1e-6 * max(float(ref.abs().max()), 1.0), (level, slot)


def test_reconfigured_and_pooled_engines_carry_no_setting(eng, vgg_weights):
    from artstyletransfer_amd import neural_nets
    _mixed_job(eng)
    assert eng.gram_shift == ((0.0, 0.0, -1.0, 0.0, 0.0, 0.0), 0b001001) == eng.gram_shift_setting()
    eng.configure(2, 64, 96)
    assert eng.gram_shift is None and eng.gram_shift_setting() is None
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 64, 96)
    e.set_gram_shift("mean")
    assert e.gram_shift == ((0.0,) * 6, 63)
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.gram_shift is None and again.gram_shift_setting() is None
    finally:
        neural_nets.return_engine(again)


# ---- 5. off means off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [True, False])
def test_zero_setting_is_bitwise_an_engine_that_never_called_the_setter(vgg_weights, batched):
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt = _job("64x96_L1")
    out = []
    for call in (False, True):
        e = StyleEngine(vgg_weights, 0, batched=batched)
        try:
            e.set_timing(2)
            e.configure(2, 64, 96)
            if call:
                assert e.lib.nst_job_set_gram_shift(e.ctx, (C.c_float * 6)(), 0) == 0
                assert e.gram_shift_setting() is None
            for i in range(2):
                e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            out.append((_bits(g), _bits(l), e.last_closure_launches()))
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    strip = lambda rec: [{k: v for k, v in d.items() if k not in ("ms",)} for d in rec]        # noqa: E731
    assert strip(out[0][2]) == strip(out[1][2]) and len(out[0][2]) > 0


def test_life_cycle_and_refusals(eng, vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import StyleEngine
    x, c, s = _mixed_job(eng)
    g0, l0 = eng.closure(x, CW, SW, TVW)
    before = eng.gram_shift_setting()

    def raw(shift, mask):
        return eng.lib.nst_job_set_gram_shift(eng.ctx, (C.c_float * 6)(*shift), mask)

    # refusals change nothing: a non-finite value, a shift on a centred map, mask bits above 5, a null array
    assert raw([float("nan")] + [0.0] * 5, 0) == -1 and raw([float("inf")] * 6, 0) == -1
    assert raw([1.0] + [0.0] * 5, 1) == -1 and raw([0.0] * 6, 64) == -1
    assert eng.lib.nst_job_set_gram_shift(eng.ctx, None, 0) == -1
    assert eng.gram_shift_setting() == before
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # a guided level and the stripe closure are refused while the setting is non-trivial
    planes = torch.ones((2, 64, 96), device="cuda:0") * 0.5
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_guidance(0, planes)
    from artstyletransfer_amd.engine import _ptr, _stream
    assert eng.lib.nst_level_set_targets_guided(eng.ctx, 0, _ptr(x), _ptr(x), 64, 96, _ptr(planes), _stream(eng.device)) == -2
    # a new setting drops the targets: the closure returns the state error until they are set again
    eng.set_gram_shift(-1.0)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure(x, CW, SW, TVW)
    eng.reset_gram_shift()
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure(x, CW, SW, TVW)
    # the setter on a guided job
    eng.set_guidance(0, planes)
    assert raw([-1.0] * 6, 0) == -2 and eng.gram_shift_setting() is None
    eng.clear_guidance()
    # the stripe closure
    e1 = StyleEngine(vgg_weights, 0)
    try:
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        e1.configure(1, 64, 96)
        e1.set_gram_shift(-1.0)
        e1.set_targets(0, xs, xs)
        with pytest.raises(NstError, match=r"\(-2\)"):
            e1.window_begin(xs, 0, 64, 64)
        e1.reset_gram_shift()
        e1.set_targets(0, xs, xs)
        e1.window_begin(xs, 0, 64, 64)
    finally:
        e1.close()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_other_arithmetic_modes_refuse_the_setting(vgg_weights, mode):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, conv_mode=mode)
    try:
        e.configure(1, 64, 96)
        assert e.lib.nst_job_set_gram_shift(e.ctx, (C.c_float * 6)(*([-1.0] * 6)), 0) == -2
        assert e.lib.nst_job_set_gram_shift(e.ctx, (C.c_float * 6)(), 0) == 0           # switching it off is no setting
        assert e.gram_shift_setting() is None
    finally:
        e.close()


def test_setter_needs_a_configured_job(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        assert e.lib.nst_job_set_gram_shift(e.ctx, (C.c_float * 6)(*([-1.0] * 6)), 0) == -2
        assert e.lib.nst_job_set_gram_shift(e.ctx, (C.c_float * 6)(), 0) == 0
    finally:
        e.close()
