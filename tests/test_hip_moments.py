"""GPU: the moment loss (nst_job_set_moments) - channel means and deviations of the style maps matched to the style's.
1. the statistic alone (nst_moments) against an fp64 evaluation of the definition, held to torch-fp32's own error;
2. the closure under equal decisions, per weighting and summed, against the oracle with cpu_ref.level_loss and
   cpu_ref.LevelTargets replaced by test-local ones that add the term (monkeypatch: no oracle edit), at hip_helpers' standing
   tolerances;
3. the paths the term's gradient takes (per-level walker, average pooling, pre-ReLU taps, content map = style map, a map
   with Gram layer weight 0, "mean" beside a centred Gram, luminance, blends); 4. identities; 5. off means off; 6. life
   cycle and refusals."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hip_helpers import (CW, SW, TVW, TERMS, check_rows, closure_vs_oracle_under_equal_decisions, dev, levels as _levels,
                         oracle_targets, rel_l2, report)
from oracle import cpu_ref
from test_hip_gram_shift import JOBS, SHAPES, _bits, _job, _map, prerelu_vgg19_features

pytestmark = pytest.mark.gpu

EPS = 1e-5
DEFAULT_STYLE = (0, 1, 2, 3, 5)
ZEROS = (0.0,) * 6


def on_maps(w, maps=DEFAULT_STYLE):
    return tuple(float(w) if i in maps else 0.0 for i in range(6))


# ---- the term restated ---------------------------------------------------------------------------------------------------
def moments_of(f, eps=EPS):
    """(mu, sigma) of a (1,C,h,w) map in its dtype: the oracle subtracts the mean first (two passes)."""
    x = f.reshape(f.shape[1], -1)
    mu = x.mean(dim=1)
    var = ((x - mu[:, None]) ** 2).mean(dim=1)
    return mu, torch.sqrt(var + eps)


def moment_values(f, target, eps=EPS):
    """(mean_i, std_i) of map f against the target (mu^t, sigma^t)."""
    mu, sd = moments_of(f, eps)
    return ((mu - target[0]) ** 2).mean(), ((sd - target[1]) ** 2).mean()


def moment_sum(feats, targets, wm, ws, maps, eps=EPS):
    """mom = sum_i (wm_i mean_i + ws_i std_i) over `maps` in ascending order, and the unweighted values {i: (mean_i, std_i)}."""
    mom, vals = None, {}
    for i in maps:
        if not (wm[i] > 0 or ws[i] > 0):
            continue
        m, s = moment_values(feats[i], targets[i], eps)
        vals[i] = (float(m.detach()), float(s.detach()))
        term = torch.tensor(np.float32(wm[i])) * m + torch.tensor(np.float32(ws[i])) * s
        mom = term if mom is None else mom + term
    return mom, vals


class PatchedOracle:
    """cpu_ref.level_loss and cpu_ref.LevelTargets with the moment term: level_loss calls the original, adds mom to the total
    and returns the same four-entry row; LevelTargets gains the style moments.  The term is in EVERY weighting of a closure -
    its weights are its own, as on the device - so the patched oracle sees the sum the device sees.  `log` keeps, per
    level_loss call, (mom, {map: (mean_i, std_i)})."""

    def __init__(self, monkeypatch, wm, ws, eps=EPS, maps=DEFAULT_STYLE):
        self.wm, self.ws, self.eps, self.maps = tuple(wm), tuple(ws), eps, tuple(maps)
        self.level_loss0, self.targets0 = cpu_ref.level_loss, cpu_ref.LevelTargets
        self.log = []
        monkeypatch.setattr(cpu_ref, "level_loss", self.level_loss)
        monkeypatch.setattr(cpu_ref, "LevelTargets", self.targets)

    def targets(self, content_t, style_t, weights):
        tg = self.targets0(content_t, style_t, weights)
        with torch.no_grad():
            sf = cpu_ref.vgg19_features(style_t, weights)
            tg.moments = {i: moments_of(sf[i], self.eps) for i in self.maps}
        return tg

    def level_loss(self, x, tg, weights, cw, sw, tvw, decisions=None, record=None):
        seen = []
        inner = cpu_ref.vgg19_features

        def keep(*a, **k):
            seen.append(inner(*a, **k))
            return seen[-1]

        cpu_ref.vgg19_features = keep             # (the features the original computes, not a second forward pass)
        try:
            total, content, style, tv = self.level_loss0(x, tg, weights, cw, sw, tvw, decisions, record)
        finally:
            cpu_ref.vgg19_features = inner
        mom, vals = moment_sum(seen[0], tg.moments, self.wm, self.ws, self.maps, self.eps)
        self.log.append((float(mom.detach()), vals))
        return total + mom, content, style, tv


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
def _stat_errors(x, eps):
    """(mu, sigma) of the definition in fp64, and the rel-L2 error of torch fp32 (mean, then the mean of squared
    differences) against it, for mu and sigma."""
    mu64, sd64 = moments_of(x.double(), eps)
    mu32, sd32 = moments_of(x, eps)
    return mu64, sd64, rel_l2(mu32.numpy(), mu64.numpy()), rel_l2(sd32.numpy(), sd64.numpy())


def _held(eng, x, what, eps=EPS):
    mu64, sd64, e_mu32, e_sd32 = _stat_errors(x, eps)
    mu, sd = eng.moments(dev(x), eps)
    mu, sd = mu.cpu(), sd.cpu()
    e_mu, e_sd = rel_l2(mu.numpy(), mu64.numpy()), rel_l2(sd.numpy(), sd64.numpy())
    report(f"moments {what}: mu device {e_mu:.2e} / torch fp32 {e_mu32:.2e}, sigma device {e_sd:.2e} / torch fp32 {e_sd32:.2e} (vs fp64)")
    assert torch.isfinite(mu).all() and torch.isfinite(sd).all()
    assert e_mu <= max(3.0 * e_mu32, 2e-6), (what, e_mu, e_mu32)
    assert e_sd <= max(3.0 * e_sd32, 2e-6), (what, e_sd, e_sd32)
    return mu, sd


@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("c", [64, 128, 256, 512])
def test_statistic_vs_fp64(eng, c, h, w):
    """Device and torch-fp32 against fp64: device <= max(3 x torch's own error, 2e-6) rel-L2, for mu and sigma each."""
    assert (h * w) % 8 != 0
    for kind in ("relu", "signed"):
        _held(eng, _map(c, h, w, kind, seed=c + h), f"C={c} {h}x{w} {kind}")


@pytest.mark.parametrize("c,h,w", [(64, 17, 65), (512, 31, 63), (128, 181, 183)])
def test_statistic_dead_and_near_dead_channels(eng, c, h, w):
    """8 exactly-zero channels (sigma = sqrt(epsilon) exactly) and 8 channels constant at 3.0 plus noise of 1e-3, where the
    one-pass variance is a difference of 9.0's: sigma ~ sqrt(epsilon + 1e-6)."""
    x = _map(c, h, w, "relu", seed=3)
    x[0, :8] = 0.0
    g = torch.Generator().manual_seed(4)
    x[0, 8:16] = 3.0 + 1e-3 * torch.randn((8, h, w), generator=g)
    mu, sd = _held(eng, x, f"dead / near-dead C={c} {h}x{w}")
    assert torch.count_nonzero(mu[:8]) == 0
    assert torch.equal(sd[:8], torch.full((8,), np.float32(np.sqrt(np.float64(np.float32(EPS))))))
    near = moments_of(x.double())[1][8:16]
    report(f"moments near-dead C={c}: sigma rel err per channel {((sd[8:16].double() - near).abs() / near).max():.2e}")
    assert float(((sd[8:16].double() - near).abs() / near).max()) <= 2e-6


def test_statistic_refusals(eng):
    from artstyletransfer_amd._lib import NstError
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.moments(dev(_map(96, 5, 7, "relu", seed=1)))
    xd = dev(_map(64, 5, 7, "relu", seed=1))
    from artstyletransfer_amd.engine import _ptr, _stream
    out = torch.empty((64,), device="cuda:0")
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert eng.lib.nst_moments(eng.ctx, _ptr(xd), 64, 5, 7, eps, _ptr(out), _ptr(out), _stream(eng.device)) == -1


# ---- 2. the closure under equal decisions ---------------------------------------------------------------------------------
# 1e3 on each of the five default style maps, both terms, epsilon 1e-5.  Measured on the CPU with the tests' synthetic
# weights (torch fp32, the patched oracle): the term's share of every level total is what test_the_term_counts asserts.
JOB_WEIGHT = {"50x76_L0": 1e3, "64x96_L1": 1e3, "68x260_L2": 1e3}
NO_TV = TERMS[:3]
TV_ONLY = TERMS[3:]


def _setup(e, contents, styles, wm, ws, eps=EPS, prepare=None):
    h, w = contents[0].shape[:2]
    e.configure(len(contents), h, w)
    if prepare:
        prepare(e)
    e.set_moments(wm, ws, eps)
    for i in range(len(contents)):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))


def _the_term_counts(patched, xt, tg, weights, what, cache=None):
    """On the CPU, before the engine is touched: the term is between 10 % and 50 % of every level total - a build that
    ignores it cannot pass, and it does not drown the rest.  Fills `cache` with the oracle's own evaluation of the weighted
    sum (hip_helpers' own_cache)."""
    rec = []
    patched.log.clear()
    loss, grad, rows = cpu_ref.closure_eval(xt, tg, weights, CW, SW, TVW, record=rec)
    if cache is not None:
        cache["all"] = (loss, grad, rows, rec)
    assert len(patched.log) == len(rows)
    for l, ((mom, vals), row) in enumerate(zip(patched.log, rows)):
        share = mom / row[0]
        report(f"moments {what} level {l}: mom {mom:.4e} of total {row[0]:.4e} = {share:.1%}; "
               f"sum(mean_i + std_i) = {sum(m + s for m, s in vals.values()):.3f}")
        assert 0.10 <= share <= 0.50, (what, l, share)


def _additivity(e, xt, what):
    """hip_helpers' additivity check (5) sums the gradients of the content, style and tv weightings and compares with the
    weighted sum's.  The moment term is in every weighting with its own weights, so that sum holds it three times and the
    weighted sum once.  The closure with cw = sw = tvw = 0 is the term alone (same forward pass, same decisions):
    g(all) = g(content) + g(style) + g(tv) - 2 g(0, 0, 0), to the helper's 2e-6.  (The helper is called with the weightings
    in two groups so that its own check, which does not know the term, stays out; every other check of it runs.)"""
    xd = dev(xt)
    g = {name: e.closure(xd, *w3)[0].cpu().numpy().astype(np.float64) for name, w3 in TERMS + (("moments", (0.0, 0.0, 0.0)),)}
    s = g["content"] + g["style"] + g["tv"] - 2.0 * g["moments"]
    add = float(np.linalg.norm(g["all"] - s) / np.linalg.norm(s))
    share = float(np.linalg.norm(g["moments"]) / np.linalg.norm(g["all"]))
    report(f"moments {what}: |g(all) - (sum of the weightings - 2 g(term alone))| / |.| = {add:.1e}; |g(term alone)| / |g(all)| = {share:.2f}")
    assert add < 2e-6, (what, add)
    assert share > 0.01, (what, share)              # (the identity is about something)


def _held_to_patched_oracle(e, xt, tg, weights, what, cache=None):
    """Losses 1e-5, rows 2e-5, gradient 2e-5 under the device's decisions (hip_helpers' standing tolerances), additivity 2e-6."""
    closure_vs_oracle_under_equal_decisions(e, xt, tg, weights, f"moments {what}", terms=NO_TV, own_cache=cache)
    closure_vs_oracle_under_equal_decisions(e, xt, tg, weights, f"moments {what}", terms=TV_ONLY)
    _additivity(e, xt, what)


@pytest.mark.parametrize("name", list(JOBS))
def test_closure_vs_patched_oracle_under_equal_decisions(eng, vgg_weights, monkeypatch, name):
    """50x76 L0 runs the per-level walker (one small level), the others the batched one; 68x260 L2 has maps 17x65 ... 1x4 and
    up to 188 exactly-dead channels per map.

    Measured on the GPU (profiles/r15_moments.txt): gradient 2.0e-7 ... 9.3e-7 under equal decisions, additivity 1.7e-7 ...
    2.3e-7; the near-constant channels of the known-risk note cost nothing at these tolerances."""
    c, s, xt = _job(name)
    wm = ws = on_maps(JOB_WEIGHT[name])
    patched = PatchedOracle(monkeypatch, wm, ws)
    tg = oracle_targets(c, s, vgg_weights)
    cache = {}
    _the_term_counts(patched, xt, tg, vgg_weights, name, cache)
    _setup(eng, c, s, wm, ws)
    _held_to_patched_oracle(eng, xt, tg, vgg_weights, name, cache)


# ---- 3. paths --------------------------------------------------------------------------------------------------------------
def _strict(e, monkeypatch, vgg_weights, what, wm=None, ws=None, prepare=None):
    c, s, xt = _job("64x96_L1")
    wm = on_maps(1e3) if wm is None else wm
    ws = on_maps(1e3) if ws is None else ws
    patched = PatchedOracle(monkeypatch, wm, ws)
    tg = oracle_targets(c, s, vgg_weights)
    cache = {}
    _the_term_counts(patched, xt, tg, vgg_weights, what, cache)
    _setup(e, c, s, wm, ws, prepare=prepare)
    _held_to_patched_oracle(e, xt, tg, vgg_weights, what, cache)


def test_path_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _strict(eng_per_level, monkeypatch, vgg_weights, "per-level walker")


def test_path_average_pooling(eng, vgg_weights, monkeypatch):
    from test_hip_pooling import avg_vgg19_features
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "avg pooling", prepare=lambda e: e.set_pooling("avg"))
    finally:
        eng.reset_pooling()


def test_path_pre_relu_taps(eng, vgg_weights, monkeypatch):
    """use_relu = False: the top map is conv5_1 before its ReLU, signed - the term's gradient, bias included, joins unmasked."""
    monkeypatch.setattr(cpu_ref, "vgg19_features", prerelu_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "pre-ReLU taps", prepare=lambda e: e.set_taps(4, [0, 1, 2, 3, 5], use_relu=False))
    finally:
        eng.reset_taps()


def test_path_mean_term_beside_a_centred_gram(eng, vgg_weights, monkeypatch):
    """The use the term was asked for: gram_shift = "mean" removes the first moment from the statistic, the "mean" term puts
    it back.  The oracle's gram_matrix is test_hip_gram_shift's centred one; the row bias carries o S and a both."""
    from test_hip_gram_shift import MEAN, PatchedGram
    monkeypatch.setattr(cpu_ref, "gram_matrix", PatchedGram((MEAN,) * 6))
    _strict(eng, monkeypatch, vgg_weights, "'mean' + centred Gram", wm=on_maps(1e3), ws=ZEROS,
            prepare=lambda e: e.set_gram_shift("mean"))


# -- taps, layer weights and blends beyond cpu_ref.level_loss: test_hip_style_blend's restatement with the term added
def _restated_closure(x, targets, weights, cw, sw, tvw, w6, taps, decisions, wm, ws, eps=EPS):
    """test_hip_style_blend.restated_closure (style = (sum_i w_i MSE_i) / nstyle over the style set) with mom added to every
    level total: (total, gradient, rows, [mom per level], [{map: (mean_i, std_i)} per level])."""
    content_i, style_set = taps
    x = x.detach().clone().requires_grad_(True)
    lv, total, rows, moms, vals = [x], None, [], [], []
    for l, tg in enumerate(targets):
        if l > 0:
            lv.append(cpu_ref.bicubic_half(lv[l - 1]))
        dec = decisions[l] if decisions is not None else None
        f = cpu_ref.vgg19_features(lv[l], weights, dec)
        content = F.mse_loss(tg.content, f[content_i].squeeze(0), reduction="mean")
        style = 0.0
        for i in style_set:
            style = style + torch.tensor(np.float32(w6[i])) * F.mse_loss(tg.grams[i][0], cpu_ref.gram_matrix(f[i])[0], reduction="mean")
        style = style / len(style_set)
        tv = cpu_ref.total_variation(lv[l], dec.tv if dec is not None else None)
        mom, v = moment_sum(f, tg.moments, wm, ws, style_set, eps)
        t = cw * content + sw * style + tvw * tv + mom
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
        moms.append(float(mom.detach()))
        vals.append(v)
    total.backward()
    return total.detach(), x.grad.detach(), rows, moms, vals


def _restated_targets(content_t, styles_t, B, weights, taps):
    """test_hip_style_blend.restated_targets plus the moment targets: the b^-weighted mean of each style's moments, accumulated
    in fp32 in ascending k as the Gram targets are."""
    from test_hip_style_blend import b_hat, restated_targets
    tg = restated_targets(content_t, styles_t, B, weights, taps)
    bh = b_hat(B)
    with torch.no_grad():
        sf = [cpu_ref.vgg19_features(s, weights) for s in styles_t]
        tg.moments = {}
        for i in taps[1]:
            mt = None
            for k in range(len(styles_t)):
                if not B[k][i] > 0:
                    continue
                mu, sd = moments_of(sf[k][i])
                term = (torch.tensor(bh[k, i]) * mu, torch.tensor(bh[k, i]) * sd)
                mt = term if mt is None else (mt[0] + term[0], mt[1] + term[1])
            tg.moments[i] = mt
    return tg


def _held_to_restatement(e, xt, targets, weights, what, w6, taps, wm, ws):
    """The device closure against the restatement under the device's decisions: the term between 10 % and 50 % of every level
    total, total 1e-5, rows 2e-5, the whole gradient 2e-5; moment_losses() against the restatement's values."""
    from test_hip_style_blend import device_decisions as decisions_of
    xd = dev(xt)
    for name, (cw, sw, tvw) in (("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW))):
        grad, losses = e.closure(xd, cw, sw, tvw)
        dec = decisions_of(e, xd, weights, taps)
        got = e.moment_losses().cpu().numpy()
        losses = losses.cpu().numpy()
        loss, g_ref, rows, moms, vals = _restated_closure(xt, targets, weights, cw, sw, tvw, w6, taps, dec, wm, ws)
        e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
        e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
        report(f"moments {what} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}; "
               f"share of the level totals {[round(m / r[0], 3) for m, r in zip(moms, rows)]}")
        if name == "all":
            assert all(0.10 <= m / r[0] <= 0.50 for m, r in zip(moms, rows)), (what, moms, rows)
        assert e_l < 1e-5, (what, name, e_l)
        check_rows(losses[:-1].reshape(e.levels, 4), np.array(rows), 2e-5, cw, sw, tvw)
        assert e_g < 2e-5, (what, name, e_g)
        for l, v in enumerate(vals):
            for i in range(6):
                ref = v.get(i, (0.0, 0.0))
                np.testing.assert_allclose(got[l, i], ref, rtol=2e-5, atol=0.0, err_msg=f"{what} level {l} map {i}")


def test_path_content_map_is_a_style_map_and_a_map_without_gram_weight(eng, vgg_weights, monkeypatch):
    """style_mask = 0x3F: the content map conv4_2 is a style map too (second K source, row bias and content addend on one
    launch).  Map 2 has Gram layer weight 0 and a moment weight: its S is the diagonal alone, and its launch still runs."""
    lw = (0.5, 2.0, 0.0, 0.25, 3.0, 1.5)
    taps = (4, (0, 1, 2, 3, 4, 5))
    wm = (3e2, 3e2, 2e3, 3e2, 3e2, 3e2)
    ws = (3e2, 0.0, 2e3, 3e2, 3e2, 3e2)
    c, s, xt = _job("64x96_L1")
    prep = cpu_ref.prepare_img
    try:
        eng.configure(2, 64, 96)
        eng.set_taps(4, [0, 1, 2, 3, 4, 5])
        eng.set_style_weights(lw)
        eng.set_moments(wm, ws)
        tg = []
        for i in range(2):
            eng.set_targets(i, dev(prep(c[i])), dev(prep(s[i])))
            tg.append(_restated_targets(prep(c[i]), [prep(s[i])], ((1.0,) * 6,), vgg_weights, taps))
        _held_to_restatement(eng, xt, tg, vgg_weights, "0x3F + layer weights, one of them 0", lw, taps, wm, ws)
        # the map without a Gram weight alone carries a gradient: its term is not lost with its S
        eng.set_moments({2: 2e3}, {2: 2e3})
        for i in range(2):
            eng.set_targets(i, dev(prep(c[i])), dev(prep(s[i])))
        g_with = eng.closure(dev(xt), 0.0, 0.0, 0.0)[0]
        assert float(g_with.abs().max()) > 0.0
    finally:
        eng.reset_style_weights()
        eng.reset_taps()


def test_path_luminance(eng, vgg_weights, monkeypatch):
    """The luminance closure with the term = the patched oracle's closure at E(u), gradient summed over the channels."""
    from artstyletransfer_amd import host_image
    from test_hip_color import expand, lum_decisions, lum_targets, start_u
    c, s = _levels(64, 96, 2, 1), _levels(70, 110, 2, 2)
    wm = ws = on_maps(1e3)
    patched = PatchedOracle(monkeypatch, wm, ws)
    try:
        eng.configure(2, 64, 96)
        eng.set_color("luminance")
        eng.set_moments(wm, ws)
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
        patched.log.clear()
        loss, _, rows = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW)
        shares = [m / r[0] for (m, _), r in zip(patched.log, rows)]
        report(f"moments luminance: share of the level totals {[round(v, 3) for v in shares]}")
        assert all(0.10 <= v <= 0.50 for v in shares), shares
        assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
        check_rows(losses[:-1].reshape(2, 4), np.array(rows), 1e-5, CW, SW, TVW)
        _, g_eq, _ = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_eq.sum(dim=1).numpy().reshape(64, 96))
        report(f"moments luminance: gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_g < 2e-5
    finally:
        eng.reset_color()


def test_path_two_style_blend(eng, vgg_weights, monkeypatch):
    """The moment targets of a blend are the b^-weighted mean of the styles' moments, with the b^ of the map's Gram target
    (unequal per map here); and blend weights (1, 0) are the single-style job bitwise."""
    c, s1, xt = _job("64x96_L1")
    s2 = _levels(58, 120, 2, 7)
    B = ((0.25, 1.0, 0.5, 0.0, 1.0, 3.0), (0.75, 1.0, 0.5, 2.0, 1.0, 1.0))
    taps = (4, DEFAULT_STYLE)
    wm = ws = on_maps(1e3)
    prep = cpu_ref.prepare_img
    eng.configure(2, 64, 96)
    eng.set_moments(wm, ws)
    tg = []
    for i in range(2):
        eng.set_targets_blend(i, dev(prep(c[i])), [dev(prep(s1[i])), dev(prep(s2[i]))], B)
        tg.append(_restated_targets(prep(c[i]), [prep(s1[i]), prep(s2[i])], B, vgg_weights, taps))
    _held_to_restatement(eng, xt, tg, vgg_weights, "two-style blend", (1.0,) * 6, taps, wm, ws)
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
MIXED_WM = (1e3, 0.0, 5e2, 1e3, 0.0, 2e3)
MIXED_WS = (1e3, 7e2, 0.0, 1e3, 0.0, 2e3)


def _mixed_job(e, name="64x96_L1", shift=None):
    c, s, xt = _job(name)
    _setup(e, c, s, MIXED_WM, MIXED_WS, prepare=(lambda q: q.set_gram_shift(shift)) if shift is not None else None)
    return dev(xt), c, s


@pytest.mark.parametrize("shift", [None, "mean"])
def test_halves_equal_the_whole_and_run_to_run_bitwise(eng, shift):
    x, _, _ = _mixed_job(eng, shift=shift)
    g, l = eng.closure(x, CW, SW, TVW)
    m = eng.moment_losses()
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    assert np.array_equal(_bits(m), _bits(eng.moment_losses()))
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_level_masks_add_up(eng, eng_per_level, which):
    e = eng if which == "batched" else eng_per_level
    x, _, _ = _mixed_job(e)
    g, l = e.closure(x, CW, SW, TVW)
    m = e.moment_losses().cpu().numpy()
    g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    gs, ls, ms = np.zeros_like(g), np.zeros_like(l), np.zeros_like(m)
    for mask in (1, 2):
        gm, lm = e.closure_levels(x, CW, SW, TVW, mask)
        mm = e.moment_losses().cpu().numpy()
        assert not mm[[lv for lv in range(2) if not (mask >> lv) & 1]].any()          # zeros for levels outside the mask
        gs += gm.cpu().numpy()
        ls += lm.cpu().numpy()
        ms += mm
    np.testing.assert_allclose(ls, l, rtol=1e-6)
    assert np.array_equal(ms, m)
    err = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
    report(f"moments level masks [{which}]: |sum - unsharded| / |.| = {err:.1e}")
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


def test_moment_losses_times_the_weights_plus_the_other_terms_are_the_row_totals(eng):
    """total = (cw content + sw style + tvw tv) + mom with mom = sum_i (wm_i mean_i + ws_i std_i) in ascending map order, every
    product and sum rounded to fp32: bitwise from what the closure returns; and zeros for the map without the term."""
    x, _, _ = _mixed_job(eng)
    _, l = eng.closure(x, CW, SW, TVW)
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    m = eng.moment_losses().cpu().numpy()
    # (a map with one of its two weights carries both unweighted values; map 4 is no style map: zeros)
    assert m.shape == (2, 6, 2) and not m[:, 4].any() and (m[:, list(DEFAULT_STYLE)] > 0).all()
    f32 = np.float32
    for lv in range(2):
        total = (f32(CW) * rows[lv, 1] + f32(SW) * rows[lv, 2]) + f32(TVW) * rows[lv, 3]
        mom = None
        for i in DEFAULT_STYLE:
            term = f32(MIXED_WM[i]) * m[lv, i, 0] + f32(MIXED_WS[i]) * m[lv, i, 1]
            mom = term if mom is None else f32(mom + term)
        assert f32(total + mom) == rows[lv, 0], (lv, total, mom, rows[lv, 0])


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
                assert e.lib.nst_job_set_moments(e.ctx, (C.c_float * 6)(), (C.c_float * 6)(), 1e-5) == 0
                assert e.moments_setting() is None
            for i in range(2):
                e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            assert not e.moment_losses().cpu().numpy().any()
            out.append((_bits(g), _bits(l), e.last_closure_launches()))
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    strip = lambda rec: [{k: v for k, v in d.items() if k not in ("ms",)} for d in rec]        # noqa: E731
    assert strip(out[0][2]) == strip(out[1][2]) and len(out[0][2]) > 0


def test_reconfigured_and_pooled_engines_carry_no_setting(eng, vgg_weights):
    from artstyletransfer_amd import neural_nets
    _mixed_job(eng)
    assert eng.moment_loss == (MIXED_WM, MIXED_WS, float(np.float32(EPS))) == eng.moments_setting()
    eng.configure(2, 64, 96)
    assert eng.moment_loss is None and eng.moments_setting() is None
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 64, 96)
    e.set_moments(5.0, None)
    assert e.moment_loss == (on_maps(5.0), ZEROS, float(np.float32(EPS)))
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.moment_loss is None and again.moments_setting() is None
    finally:
        neural_nets.return_engine(again)


# ---- 6. life cycle and refusals --------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(eng, vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import StyleEngine, _ptr, _stream
    x, c, s = _mixed_job(eng)
    g0, l0 = eng.closure(x, CW, SW, TVW)
    before = eng.moments_setting()
    one = [1.0, 1.0, 1.0, 1.0, 0.0, 1.0]

    def raw(wm, ws, eps=1e-5):
        return eng.lib.nst_job_set_moments(eng.ctx, (C.c_float * 6)(*wm), (C.c_float * 6)(*ws), eps)

    # refusals change nothing: negative or non-finite weights or epsilon, a null array, a positive weight on a map that is
    # not one of the job's style taps (map 4, conv4_2, under the default taps)
    for bad in (-1.0, float("nan"), float("inf")):
        assert raw([bad] + [0.0] * 5, one) == -1 and raw(one, [0.0] * 5 + [bad]) == -1
    for eps in (0.0, -1e-5, float("nan"), float("inf")):
        assert raw(one, one, eps) == -1
    assert eng.lib.nst_job_set_moments(eng.ctx, None, (C.c_float * 6)(), 1e-5) == -1
    assert raw([0.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.0] * 6) == -1 and raw([0.0] * 6, [1.0] * 6) == -1
    assert eng.moments_setting() == before
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # a guided level is refused while the term is on
    planes = torch.ones((2, 64, 96), device="cuda:0") * 0.5
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_guidance(0, planes)
    assert eng.lib.nst_level_set_targets_guided(eng.ctx, 0, _ptr(x), _ptr(x), 64, 96, _ptr(planes), _stream(eng.device)) == -2
    # a new setting drops the targets: the closure returns the state error until they are set again
    eng.set_moments(1.0, 1.0)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure(x, CW, SW, TVW)
    eng.reset_moments()
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure(x, CW, SW, TVW)
    # ... and a pending backward half
    _mixed_job(eng)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_moments(MIXED_WM, MIXED_WS)
    for i in range(2):
        eng.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure_backward(x, CW, SW, TVW)
    eng.reset_moments()
    # the setter on a guided job: the other order
    eng.set_guidance(0, planes)
    assert raw(one, one) == -2 and eng.moments_setting() is None
    assert raw([0.0] * 6, [0.0] * 6) == 0                      # switching it off is no setting
    eng.clear_guidance()
    # the stripe closure
    e1 = StyleEngine(vgg_weights, 0)
    try:
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        e1.configure(1, 64, 96)
        e1.set_moments(1.0, 1.0)
        e1.set_targets(0, xs, xs)
        with pytest.raises(NstError, match=r"\(-2\)"):
            e1.window_begin(xs, 0, 64, 64)
        e1.reset_moments()
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
        one = (C.c_float * 6)(1.0, 1.0, 1.0, 1.0, 0.0, 1.0)
        assert e.lib.nst_job_set_moments(e.ctx, one, one, 1e-5) == -2
        assert e.lib.nst_job_set_moments(e.ctx, (C.c_float * 6)(), (C.c_float * 6)(), 1e-5) == 0      # switching it off is no setting
        assert e.moments_setting() is None
        mu, sd = e.moments(dev(_map(64, 5, 7, "relu", seed=1)))          # the statistic alone runs in every mode
        assert torch.isfinite(mu).all() and torch.isfinite(sd).all()
    finally:
        e.close()


def test_setter_needs_a_configured_job(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        one = (C.c_float * 6)(1.0, 1.0, 1.0, 1.0, 0.0, 1.0)
        assert e.lib.nst_job_set_moments(e.ctx, one, one, 1e-5) == -2
        assert e.lib.nst_job_set_moments(e.ctx, (C.c_float * 6)(), (C.c_float * 6)(), 1e-5) == 0
        out = torch.empty((12,), device="cuda:0")
        from artstyletransfer_amd.engine import _ptr, _stream
        assert e.lib.nst_job_moment_losses(e.ctx, _ptr(out), _stream(e.device)) == -2
    finally:
        e.close()
