"""GPU: caller-chosen content / style feature maps (nst_job_set_taps, StyleEngine.set_taps) against what the reference's
own LossBuilder / Vgg19 produced with the same arguments (tests/golden/make_fixtures_taps.py) and against the CPU oracle
with its tap constants set to the same maps.  Every arithmetic mode and schedule of the closure is held to the taps."""
import asyncio

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import (CW, SW, TERMS, TVW, assert_grad_close, check_rows, closure_vs_oracle_under_equal_decisions, dev,
                         rel_l2, setup as _setup)

pytestmark = pytest.mark.gpu

CASES = ("shallow", "same", "c5s4", "prerelu", "c0s3")
MODES = {"f16x2": {}, "per_level": {"batched": False}, "bf16x3": {"conv_mode": "bf16x3"}, "f32": {"conv_mode": "f32"}}
TAP_LAYER = (0, 2, 4, 8, 9, 12)          # Vgg19 output index -> conv layer


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


def _fixture_setup(eng, fx):
    eng.configure(2, 64, 96)
    eng.set_taps(int(fx["content_index"]), [int(i) for i in fx["style_indices"]], use_relu=bool(fx["use_relu"]))
    for i in range(2):
        eng.set_targets(i, dev(cpu_ref.prepare_img(fx[f"content{i}"])), dev(cpu_ref.prepare_img(fx[f"style{i}"])))
    return dev(cpu_ref.prepare_img(fx["x_img"]))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", CASES)
def test_taps_vs_reference_fixture(engines, golden, case, mode):
    """The closure with the weighted sum and with each term alone against the reference's LossBuilder with the same
    taps: losses rel <= 1e-5, gradients by the flip-aware comparison (TV: outright)."""
    fx = golden(f"taps_{case}_64x96_L1")
    eng = engines(mode)
    x = _fixture_setup(eng, fx)
    for name, (cw, sw, tvw) in TERMS:
        if name == "all":
            total, grad_ref, rows = fx["total"], fx["grad"], fx["rows"]
        else:
            tag = {"content": "c", "style": "s", "tv": "tv"}[name]
            total, grad_ref, rows = fx[f"total_{tag}"], fx[f"grad_{tag}"], None
        grad, losses = eng.closure(x, cw, sw, tvw)
        losses = losses.cpu().numpy()
        assert float(losses[-1]) == pytest.approx(float(total), rel=1e-5), (case, mode, name)
        if rows is not None:
            check_rows(losses[:-1].reshape(2, 4), np.array(rows), 2e-5, cw, sw, tvw)
        g = grad.cpu().numpy()
        if name == "tv":
            assert rel_l2(g, grad_ref) < 5e-6, (case, mode)
        else:
            assert_grad_close(g, grad_ref, f"taps {case} {mode} [{name}]")


def test_taps_run_to_run_bitwise(engines, golden):
    fx = golden("taps_same_64x96_L1")
    eng = engines("f16x2")
    x = _fixture_setup(eng, fx)
    g1, l1 = eng.closure(x, CW, SW, TVW)
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)


class _Truncated:
    """The engine as closure_vs_oracle_under_equal_decisions sees it, for a pass that stops at conv layer `top`: the
    activations above `top` were not written by this closure, so the decisions there are the oracle's own on the
    device's level image (those layers feed no loss term: any decision there leaves the loss and the gradient alone)."""

    def __init__(self, eng, top, weights):
        self._eng, self._top, self._w, self.x = eng, top, weights, None

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def closure(self, x, cw, sw, tvw):
        self.x = x
        return self._eng.closure(x, cw, sw, tvw)

    def level_activations(self, level):
        acts = self._eng.level_activations(level)
        img = (self.x if level == 0 else self._eng.level_image(level)).cpu().reshape(1, 3, *self._eng.level_shape(level))
        rec = []
        with torch.no_grad():
            cpu_ref.vgg19_features(img, self._w, record=rec)
        return [a if l <= self._top else torch.relu(rec[l]).to(a.device) for l, a in enumerate(acts)]


@pytest.mark.parametrize("content,style", [(1, (0, 1)), (2, (2, 3)), (5, (4,)), (0, (3,))])
def test_relu_taps_vs_oracle_under_equal_decisions(engines, vgg_weights, monkeypatch, content, style):
    """The strict parity (hip_helpers) with the oracle's tap constants set to the same maps."""
    from hip_helpers import levels as _levels, oracle_targets
    monkeypatch.setattr(cpu_ref, "CONTENT_INDEX", content)
    monkeypatch.setattr(cpu_ref, "STYLE_INDICES", tuple(style))
    eng = engines("f16x2")
    c, s = _levels(96, 80, 2, 1), _levels(70, 110, 2, 2)
    eng.configure(2, 96, 80)
    eng.set_taps(content, list(style))
    for i in range(2):
        eng.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
    tg = oracle_targets(c, s, vgg_weights)
    xt = cpu_ref.prepare_img((0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(96, 80, seed=9)).astype(np.float32))
    top = max(TAP_LAYER[content], *(TAP_LAYER[i] for i in style))
    closure_vs_oracle_under_equal_decisions(_Truncated(eng, top, vgg_weights), xt, tg, vgg_weights,
                                            f"taps c{content} s{list(style)}")


def test_explicit_default_taps_are_bitwise_the_default(vgg_weights, golden):
    """An engine that never called set_taps and one that set other taps and then the default ones back compute the
    same bits (the default schedule is untouched)."""
    from artstyletransfer_amd.engine import StyleEngine
    fx = golden("closure_64x96_L1")
    x = dev(cpu_ref.prepare_img(fx["x_img"]))
    out = []
    for explicit in (False, True):
        e = StyleEngine(vgg_weights, 0)
        try:
            if explicit:
                e.configure(2, 64, 96)
                e.set_taps(2, [2, 3])
                e.set_taps(4, [5, 3, 2, 1, 0, 0], use_relu=True)
            _setup(e, [fx["content0"], fx["content1"]], [fx["style0"], fx["style1"]])
            g, l = e.closure(x, CW, SW, TVW)
            out.append((g.clone(), l.clone()))
        finally:
            e.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_truncation_drops_conv_launches(engines, golden):
    """Deepest map relu4_1 (content 3, style 0..3): the forward stops at conv4_1 and the backward starts there - 8 + 8
    3x3 launches instead of 12 + 12."""
    fx = golden("closure_64x96_L1")
    eng = engines("f16x2")
    x = dev(cpu_ref.prepare_img(fx["x_img"]))
    counts = {}
    for taps in ((4, [0, 1, 2, 3, 5]), (3, [0, 1, 2, 3])):
        eng.configure(2, 64, 96)
        eng.set_taps(*taps)
        for i in range(2):
            eng.set_targets(i, dev(cpu_ref.prepare_img(fx[f"content{i}"])), dev(cpu_ref.prepare_img(fx[f"style{i}"])))
        eng.set_timing(2)
        try:
            eng.closure(x, CW, SW, TVW)
            torch.cuda.synchronize()
            counts[taps[0]] = eng.last_closure_class(0)[1]
        finally:
            eng.set_timing(0)
    assert counts == {4: 24, 3: 16}


def test_level_sharded_closure_adds_up(engines, golden):
    fx = golden("taps_c5s4_64x96_L1")
    eng = engines("f16x2")
    x = _fixture_setup(eng, fx)
    g, l = eng.closure(x, CW, SW, TVW)
    g0, l0 = eng.closure_levels(x, CW, SW, TVW, 0b01)
    g0, l0 = g0.clone(), l0.clone()
    g1, l1 = eng.closure_levels(x, CW, SW, TVW, 0b10)
    assert rel_l2((g0 + g1).cpu().numpy(), g.cpu().numpy()) < 1e-6
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    np.testing.assert_allclose(l0.cpu().numpy()[:4], rows[0], rtol=1e-6)
    np.testing.assert_allclose(l1.cpu().numpy()[4:8], rows[1], rtol=1e-6)
    assert not l0.cpu().numpy()[4:8].any() and not l1.cpu().numpy()[:4].any()


def test_stripe_closure_refuses_other_taps(vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        c = cpu_ref.synthetic_image(64, 96, 1)
        e.configure(1, 64, 96)
        e.set_taps(2, [2, 3])
        e.set_targets(0, dev(cpu_ref.prepare_img(c)), dev(cpu_ref.prepare_img(c)))
        x = dev(cpu_ref.prepare_img(c))
        with pytest.raises(NstError, match=r"\(-2\).*default feature maps"):
            e.window_begin(x, 0, 64, 64)
    finally:
        e.close()


def test_set_taps_drops_targets_and_validates(engines):
    from artstyletransfer_amd._lib import NstError
    eng = engines("f16x2")
    c = cpu_ref.synthetic_image(64, 96, 1)
    eng.configure(1, 64, 96)
    eng.set_targets(0, dev(cpu_ref.prepare_img(c)), dev(cpu_ref.prepare_img(c)))
    eng.set_taps(1, [0])
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure(dev(cpu_ref.prepare_img(c)), CW, SW, TVW)
    with pytest.raises(ValueError):
        eng.set_taps(1, [])
    lib = eng.lib
    assert lib.nst_job_set_taps(eng.ctx, 6, 1, 1) != 0 and lib.nst_job_set_taps(eng.ctx, 0, 0x40, 1) != 0
    assert lib.nst_job_set_taps(eng.ctx, 0, 0, 1) != 0 and lib.nst_job_set_taps(eng.ctx, 0, 1, 2) != 0
    eng.set_taps(4, [0, 1, 2, 3, 5])


def test_pooled_engine_comes_back_with_default_taps(vgg_weights):
    from artstyletransfer_amd import neural_nets
    from artstyletransfer_amd.engine import DEFAULT_TAPS
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 64, 96)
    e.set_taps(0, [3], use_relu=False)
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.taps == DEFAULT_TAPS
    finally:
        neural_nets.return_engine(again)


def test_vgg_prerelu_features_vs_reference(vgg_weights, golden):
    from artstyletransfer_amd import neural_nets
    from hip_helpers import check_summary
    neural_nets.set_weights(vgg_weights)
    fx = golden("taps_vgg_prerelu_48x80")
    net = neural_nets.Vgg19(use_relu=False).to("cuda:0")
    assert list(net.layer_names) == list(fx["layer_names"]) and net.offset == int(fx["offset"])
    outs = net(dev(cpu_ref.prepare_img(fx["img"])))
    assert list(type(outs)._fields) == list(fx["fields"])
    for i, o in enumerate(outs):
        scale = float(np.abs(fx[f"out{i}.val"]).max()) + 1.0
        check_summary(o, fx, f"out{i}", atol=2e-4 * scale)
    assert float(outs[5].min()) < 0.0 and all(float(o.min()) >= 0.0 for o in outs[:5])
    got = outs[5].cpu().numpy()
    assert rel_l2(got, fx["out5_full"]) < 1e-4
    # the shared (post-ReLU) engine is untouched
    relu5 = neural_nets.Vgg19().to("cuda:0")(dev(cpu_ref.prepare_img(fx["img"])))[5]
    assert float(relu5.min()) >= 0.0 and rel_l2(relu5.cpu().numpy(), np.maximum(got, 0.0)) < 1e-6


def test_adam_with_other_taps(engines, golden):
    """Ten Adam steps with content 2 / style [2, 3] stay finite; the first moves every pixel by lr against the sign of
    the reference's gradient."""
    from artstyletransfer_amd.engine import PixelOptimizer
    fx = golden("taps_same_64x96_L1")
    eng = engines("f16x2")
    x = _fixture_setup(eng, fx)
    x0 = x.clone()
    opt = PixelOptimizer(eng, "adam", 10.0)
    try:
        totals = []
        for k in range(10):
            _, rows = opt.step(x, CW, SW, TVW)
            assert np.isfinite(rows).all() and torch.isfinite(x).all()
            totals.append(float(np.asarray(rows).reshape(-1)[-1]))
            if k == 0:
                d = (x - x0).cpu().numpy()
                g = fx["grad"]
                big = np.abs(g) > 1e-3 * np.abs(g).max()
                assert np.mean(np.sign(d[big]) == -np.sign(g[big])) > 0.999
                assert np.abs(d[big]).min() > 9.9 and np.abs(d).max() < 10.01
    finally:
        opt.close()
    assert len(totals) == 10


def test_job_driver_with_other_taps(vgg_weights):
    from artstyletransfer_amd import config, neural_nets
    import neural_style_transfer as nst
    neural_nets.set_weights(vgg_weights)
    content = cpu_ref.synthetic_image(64, 96, seed=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=1, iters_num=3, optimizer="adam")

    async def run():
        out = []
        async for percent, img in nst.neural_style_transfer(
                nst.ContentStylePair(("c", content), ("s", style)), cfg.content_weight, cfg.style_weight, cfg.tv_weight,
                cfg.optimizer, cfg.model, "content+noise", cfg.iters_num, cfg.levels_num, cfg.noise_factor,
                cfg.noise_levels, cfg.noise_levels_central_amplitude, cfg.noise_levels_peripheral_amplitude,
                cfg.noise_levels_dispersion, content_layer="relu2_1", style_layers=["relu1_1", 1, 2]):
            out.append((percent, img))
        return out

    np.random.seed(0)
    out = asyncio.run(run())
    assert [round(p) for p, _ in out] == [33, 67, 100]
    for _, img in out:
        assert img.shape == (256, 384, 3) and np.isfinite(img).all()
