"""GPU: average pooling in the VGG19 feature network (nst_job_set_pooling, StyleEngine.set_pooling("avg")) against what the
reference's own Vgg19 / LossBuilder produced on its network with every MaxPool2d replaced by AvgPool2d(2, 2)
(tests/golden/make_fixtures_pool.py), against the CPU oracle with a test-local average-pool network under the device's ReLU
decisions, and the serving rules (dropped targets, closure reuse, stripe refusal, the default path bit for bit)."""
import asyncio

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from hip_helpers import (CW, SW, TERMS, TVW, assert_grad_close, check_rows, closure_vs_oracle_under_equal_decisions, dev,
                         levels as _levels, oracle_targets, rel_l2, report, rows_rel_err, setup as _setup)

pytestmark = pytest.mark.gpu

# the four modes of tests/test_hip_taps.py::MODES, and f16x2 with every convolution direct / with forced row bands
MODES = {"f16x2": {}, "per_level": {"batched": False}, "bf16x3": {"conv_mode": "bf16x3"}, "f32": {"conv_mode": "f32"},
         "direct": {"h2_winograd": False}, "bands": {"batched": False, "h2_band_rows": 16}}
FIXTURES = ("pool_avg_64x96_L1", "pool_avg_shallow_64x96_L1", "pool_avg_prerelu_64x96_L1", "pool_avg_50x76_L0")


def avg_vgg19_features(x, weights, decisions=None, record=None):
    """cpu_ref.vgg19_features with F.avg_pool2d for the four pools: ReLU masks from `decisions.relu` when given; the
    average itself has no decisions."""
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


def _avg_setup(eng, contents, styles):
    h, w = contents[0].shape[:2]
    eng.configure(len(contents), h, w)
    eng.set_pooling("avg")
    for i in range(len(contents)):
        eng.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))


def _fixture_setup(eng, fx):
    nlev = int(fx["levels"])
    h, w = fx["content0"].shape[:2]
    eng.configure(nlev, h, w)
    eng.set_taps(int(fx["content_index"]), [int(i) for i in fx["style_indices"]], use_relu=bool(fx["use_relu"]))
    eng.set_pooling("avg")
    assert eng.pooling == "avg" and eng.lib.nst_job_pooling(eng.ctx) == 1
    for i in range(nlev):
        eng.set_targets(i, dev(cpu_ref.prepare_img(fx[f"content{i}"])), dev(cpu_ref.prepare_img(fx[f"style{i}"])))
    return dev(cpu_ref.prepare_img(fx["x_img"])), nlev


def _reset(eng):
    eng.reset_taps()
    eng.reset_pooling()
    eng.reset_color()


# ---- 1. the six maps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "bf16x3", "f32"])
def test_avg_features_vs_reference_fixture(engines, golden, mode):
    """nst_vgg_features under NST_POOL_AVG against the reference's avg-pool network: rel-L2 <= 3e-6 on every map (the
    sampled entries of the fixture; the two smallest maps whole)."""
    fx = golden("pool_avg_vgg_48x80")
    eng = engines(mode)
    try:
        eng.set_pooling("avg")
        outs = eng.vgg_features(dev(cpu_ref.prepare_img(fx["img"])))
    finally:
        _reset(eng)
    for i, o in enumerate(outs):
        assert list(o.shape) == list(fx[f"out{i}.shape"])
        got = o.reshape(-1).cpu()[torch.from_numpy(fx[f"out{i}.idx"])].numpy()
        e = rel_l2(got, fx[f"out{i}.val"])
        report(f"avg features {mode} map {i}: rel-L2 {e:.2e}")
        assert e <= 3e-6, (mode, i, e)
    e5, e4 = rel_l2(outs[5].cpu().numpy(), fx["out5_full"]), rel_l2(outs[4].cpu().numpy(), fx["out4_full"])
    report(f"avg features {mode}: whole relu5_1 rel-L2 {e5:.2e}, whole conv4_2 {e4:.2e}")
    assert e5 <= 3e-6 and e4 <= 3e-6


def test_vgg19_mirror_with_avg_pooling(vgg_weights, golden):
    """neural_nets.Vgg19(pooling="avg") returns the same maps; the shared (max) engine is untouched."""
    from artstyletransfer_amd import neural_nets
    neural_nets.set_weights(vgg_weights)
    fx = golden("pool_avg_vgg_48x80")
    x = dev(cpu_ref.prepare_img(fx["img"]))
    outs = neural_nets.Vgg19(pooling="avg").to("cuda:0")(x)
    assert rel_l2(outs[5].cpu().numpy(), fx["out5_full"]) <= 3e-6
    mx = neural_nets.Vgg19().to("cuda:0")(x)
    assert rel_l2(mx[5].cpu().numpy(), golden("vgg_48x80")["out5_full"]) < 1e-4
    assert torch.equal(mx[0], outs[0]) and not torch.equal(mx[1], outs[1])       # relu1_1 sits above the first pool


# ---- 2. the closure against the reference's LossBuilder on the avg-pool network ------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", FIXTURES)
def test_avg_closure_vs_reference_fixture(engines, golden, name, mode):
    """Weighted sum and each term alone: losses rel <= 1e-5, rows by check_rows at 2e-5, gradients by the flip-aware
    comparison (TV: outright at 5e-6) - the bounds of test_taps_vs_reference_fixture."""
    fx = golden(name)
    eng = engines(mode)
    try:
        x, nlev = _fixture_setup(eng, fx)
        for term, (cw, sw, tvw) in TERMS:
            if term == "all":
                total, grad_ref, rows = fx["total"], fx["grad"], fx["rows"]
            else:
                tag = {"content": "c", "style": "s", "tv": "tv"}[term]
                total, grad_ref, rows = fx[f"total_{tag}"], fx[f"grad_{tag}"], None
            grad, losses = eng.closure(x, cw, sw, tvw)
            losses = losses.cpu().numpy()
            report(f"avg closure {name} {mode} [{term}]: total rel {abs(float(losses[-1]) - float(total)) / abs(float(total)):.2e}")
            assert float(losses[-1]) == pytest.approx(float(total), rel=1e-5), (name, mode, term)
            if rows is not None:
                check_rows(losses[:-1].reshape(nlev, 4), np.array(rows), 2e-5, cw, sw, tvw)
            g = grad.cpu().numpy()
            if term == "tv":
                assert rel_l2(g, grad_ref) < 5e-6, (name, mode)
            else:
                assert_grad_close(g, grad_ref, f"avg {name} {mode} [{term}]")
    finally:
        _reset(eng)


# ---- 3. strict parity under equal ReLU decisions -------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,hs,ws", [(96, 80, 70, 110), (89, 131, 64, 96)])
def test_avg_closure_vs_oracle_under_equal_decisions(engines, vgg_weights, monkeypatch, h, w, hs, ws):
    """hip_helpers' strict form with the oracle's network replaced by the test-local average-pool one: whole gradient 2e-5
    under the device's ReLU masks, per term, losses 1e-5.  89x131 halves to 44x65: odd sizes at every pool."""
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    eng = engines("f16x2")
    c, s = _levels(h, w, 2, 1), _levels(hs, ws, 2, 2)
    try:
        _avg_setup(eng, c, s)
        tg = oracle_targets(c, s, vgg_weights)
        xt = cpu_ref.prepare_img((0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32))
        closure_vs_oracle_under_equal_decisions(eng, xt, tg, vgg_weights, f"avg pooling {h}x{w} L1")
    finally:
        _reset(eng)


# ---- 4. the network's backward alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "bf16x3", "f32"])
@pytest.mark.parametrize("h,w", [(48, 80), (35, 51)])
def test_avg_vgg_backward_vs_autograd(engines, vgg_weights, mode, h, w):
    """nst_vgg_features_backward with random injected gradients (all six maps; relu2_1 alone; relu5_1 alone) against autograd
    through the test-local average-pool network under the device's ReLU masks: rel-L2 <= 2e-5."""
    eng = engines(mode)
    x0 = cpu_ref.prepare_img(cpu_ref.synthetic_image(h, w, seed=3))
    try:
        eng.set_pooling("avg")
        dec = cpu_ref.Decisions([a.cpu() for a in eng.vgg_activations(dev(x0))])
        g = torch.Generator().manual_seed(21)
        with torch.no_grad():
            gouts = [torch.randn(o.shape, generator=g) / o.numel() for o in avg_vgg19_features(x0, vgg_weights)]
        for keep in ((0, 1, 2, 3, 4, 5), (1,), (5,)):
            x = x0.clone().requires_grad_(True)
            outs = avg_vgg19_features(x, vgg_weights, dec)
            sum((outs[i] * gouts[i]).sum() for i in keep).backward()
            got = eng.vgg_features_backward(dev(x0), [dev(gouts[i]) if i in keep else None for i in range(6)])
            e = rel_l2(got.cpu().numpy(), x.grad.numpy())
            report(f"avg vgg backward {mode} {h}x{w} maps {keep}: rel-L2 {e:.2e}")
            assert e <= 2e-5, (mode, keep, e)
    finally:
        _reset(eng)


# ---- 5. composition: luminance, level sharding ---------------------------------------------------------------------------
def test_avg_luminance_closure_is_the_rgb_closure_at_E(engines, vgg_weights, monkeypatch):
    """The luminance closure under avg pooling = the avg-pool oracle's closure at E(u), gradient summed over the channels."""
    from test_hip_color import expand, lum_decisions, lum_setup, start_u
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    eng = engines("f16x2")
    c, s = _levels(128, 192, 2, 1), _levels(110, 150, 2, 2)
    try:
        eng.set_pooling("avg")
        tg = lum_setup(eng, c, s, vgg_weights)           # (configure keeps the context's pooling; set_color drops the targets)
        assert eng.pooling == "avg"
        u = start_u(c[0])
        ud = dev(u.reshape(1, 1, 128, 192))
        xt = expand(u)
        grad, losses = eng.closure(ud, CW, SW, TVW)
        dec = lum_decisions(eng, ud)
        losses = losses.cpu().numpy()
        loss, _, rows = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW)
        assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
        check_rows(losses[:-1].reshape(2, 4), np.array(rows), 1e-5, CW, SW, TVW)
        _, g_eq, _ = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        assert_grad_close(grad.cpu().numpy().reshape(128, 192), g_eq.sum(dim=1).numpy().reshape(128, 192), "avg luminance")
    finally:
        _reset(eng)


@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
def test_avg_level_sharded_closure_adds_up(engines, golden, mode):
    fx = golden("pool_avg_64x96_L1")
    eng = engines(mode)
    try:
        x, _ = _fixture_setup(eng, fx)
        g, l = eng.closure(x, CW, SW, TVW)
        g, l = g.clone(), l.clone()
        g0, l0 = eng.closure_levels(x, CW, SW, TVW, 0b01)
        g0, l0 = g0.clone(), l0.clone()
        g1, l1 = eng.closure_levels(x, CW, SW, TVW, 0b10)
        assert rel_l2((g0 + g1).cpu().numpy(), g.cpu().numpy()) < 1e-6
        rows = l.cpu().numpy()[:-1].reshape(2, 4)
        np.testing.assert_allclose(l0.cpu().numpy()[:4], rows[0], rtol=1e-6)
        np.testing.assert_allclose(l1.cpu().numpy()[4:8], rows[1], rtol=1e-6)
        assert not l0.cpu().numpy()[4:8].any() and not l1.cpu().numpy()[:4].any()
    finally:
        _reset(eng)


# ---- 6. bitwise and serving rules ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
def test_avg_run_to_run_bitwise(engines, golden, mode):
    fx = golden("pool_avg_64x96_L1")
    eng = engines(mode)
    try:
        x, _ = _fixture_setup(eng, fx)
        g1, l1 = eng.closure(x, CW, SW, TVW)
        g1, l1 = g1.clone(), l1.clone()
        g2, l2 = eng.closure(x, CW, SW, TVW)
        assert torch.equal(g1, g2) and torch.equal(l1, l2)
    finally:
        _reset(eng)


@pytest.mark.parametrize("mode", ["f16x2", "per_level", "bf16x3"])
def test_max_after_avg_is_bitwise_the_default(vgg_weights, golden, mode):
    """An engine that set avg, then max, then its targets again computes the bits of one that never called set_pooling."""
    from artstyletransfer_amd.engine import StyleEngine
    fx = golden("closure_64x96_L1")
    x = dev(cpu_ref.prepare_img(fx["x_img"]))
    out = []
    for detour in (False, True):
        e = StyleEngine(vgg_weights, 0, **MODES[mode])
        try:
            if detour:
                _avg_setup(e, [fx["content0"], fx["content1"]], [fx["style0"], fx["style1"]])
                e.closure(x, CW, SW, TVW)
                e.set_pooling("max")
                assert e.pooling == "max" and e.lib.nst_job_pooling(e.ctx) == 0
            _setup(e, [fx["content0"], fx["content1"]], [fx["style0"], fx["style1"]])
            g, l = e.closure(x, CW, SW, TVW)
            out.append((g.clone(), l.clone()))
        finally:
            e.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_set_pooling_drops_targets_and_validates(engines):
    from artstyletransfer_amd._lib import NstError
    eng = engines("f16x2")
    c = cpu_ref.synthetic_image(64, 96, 1)
    x = dev(cpu_ref.prepare_img(c))
    try:
        eng.configure(1, 64, 96)
        eng.set_targets(0, x, x)
        eng.closure(x, CW, SW, TVW)
        for mode in ("avg", "avg", "max"):                    # setting the mode, even the same one, drops the targets
            eng.set_pooling(mode)
            with pytest.raises(NstError, match=r"\(-2\)"):
                eng.closure(x, CW, SW, TVW)
            eng.set_targets(0, x, x)
            eng.closure(x, CW, SW, TVW)
        with pytest.raises(ValueError):
            eng.set_pooling("mean")
        assert eng.lib.nst_job_set_pooling(eng.ctx, 2) == -1 and eng.lib.nst_job_set_pooling(eng.ctx, -1) == -1
        assert eng.lib.nst_job_pooling(eng.ctx) == 0
        eng.closure(x, CW, SW, TVW)                           # a refused value leaves the context (and its targets) alone
    finally:
        _reset(eng)


def test_lbfgs_evaluates_its_first_closure_after_a_pooling_change(engines, golden):
    """Closure reuse forgets across nst_job_set_pooling: the step after the change evaluates (is not served) its first
    closure, also when the mode set is the one the context already had."""
    from artstyletransfer_amd.engine import PixelOptimizer
    fx = golden("closure_64x96_L1")
    eng = engines("f16x2")
    c, s = [fx["content0"], fx["content1"]], [fx["style0"], fx["style1"]]
    try:
        _setup(eng, c, s)
        x = dev(cpu_ref.prepare_img(fx["x_img"]))
        opt = PixelOptimizer(eng, "lbfgs")
        try:
            opt.step(x, CW, SW, TVW)
            before = opt.closure_stats()[1]
            opt.step(x, CW, SW, TVW)
            assert opt.closure_stats()[1] == before + 1          # nothing changed: served
            for mode in ("avg", "avg", "max"):
                eng.set_pooling(mode)
                for i in range(2):
                    eng.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
                before = opt.closure_stats()[1]
                _, rows = opt.step(x, CW, SW, TVW)
                assert opt.closure_stats()[1] == before, mode
                assert np.isfinite(rows).all()
        finally:
            opt.close()
    finally:
        _reset(eng)


def test_stripe_closure_refuses_avg_pooling(vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        c = cpu_ref.synthetic_image(64, 96, 1)
        x = dev(cpu_ref.prepare_img(c))
        e.configure(1, 64, 96)
        e.set_pooling("avg")
        e.set_targets(0, x, x)
        with pytest.raises(NstError, match=r"\(-2\).*max pooling"):
            e.window_begin(x, 0, 64, 64)
        e.set_pooling("max")
        e.set_targets(0, x, x)
        e.window_begin(x, 0, 64, 64)
    finally:
        e.close()


def test_pooled_engine_comes_back_with_max_pooling(vgg_weights):
    from artstyletransfer_amd import neural_nets
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 64, 96)
    e.set_pooling("avg")
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.pooling == "max" and again.lib.nst_job_pooling(again.ctx) == 0
    finally:
        neural_nets.return_engine(again)


# ---- 7. avg really is avg; free-running; the public path -----------------------------------------------------------------
def test_avg_and_max_losses_differ(engines, golden):
    fx = golden("closure_64x96_L1")
    eng = engines("f16x2")
    c, s = [fx["content0"], fx["content1"]], [fx["style0"], fx["style1"]]
    x = dev(cpu_ref.prepare_img(fx["x_img"]))
    try:
        _setup(eng, c, s)
        _, lm = eng.closure(x, CW, SW, TVW)
        lm = lm.cpu().numpy()
        _avg_setup(eng, c, s)
        _, la = eng.closure(x, CW, SW, TVW)
        la = la.cpu().numpy()
    finally:
        _reset(eng)
    assert float(lm[-1]) == pytest.approx(float(fx["total"]), rel=1e-5)
    assert float(la[-1]) == pytest.approx(float(golden("pool_avg_64x96_L1")["total"]), rel=1e-5)
    assert abs(float(la[-1]) - float(lm[-1])) > 1e-2 * abs(float(lm[-1]))
    assert la[3] == pytest.approx(lm[3], rel=1e-6)            # the TV term does not see the network


def test_avg_adam_trajectory_vs_oracle_process(engines, vgg_weights, monkeypatch):
    """12 free-running Adam iterations under avg pooling on the 64x96 L1 job of test_adam_trajectory_vs_reference against 12
    iterations of cpu_ref.run_process with the average-pool network: first closure's rows 2e-5, every closure's rows
    1e-2, mean |final image diff| < 2e-2 (that test's bounds)."""
    from artstyletransfer_amd.engine import PixelOptimizer
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    c, s = _levels(64, 96, 2, 1), _levels(64, 96, 2, 2)
    rec, final = [], None
    for img, _ in cpu_ref.run_process(c, s, c[0], vgg_weights, "adam", 12, CW, SW, TVW, record=rec):
        final = img
    ref_rows = np.array([r["rows"] for r in rec])
    eng = engines("f16x2")
    try:
        _avg_setup(eng, c, s)
        x = dev(cpu_ref.prepare_img(c[0]))
        opt = PixelOptimizer(eng, "adam")
        try:
            rows = []
            for k in range(12):
                info, r = opt.step(x, CW, SW, TVW)
                assert info.closures == 1 and info.total_closures == k + 1
                rows.append(r[0, :-1].reshape(2, 4))
        finally:
            opt.close()
        rows = np.array(rows)
        diff = float(np.mean(np.abs(eng.unprepare_img(x).cpu().numpy() - final)))
        report(f"avg adam 64x96 12 steps free-running: worst level-total rel err {rows_rel_err(rows, ref_rows):.2e}, mean |img diff| {diff:.2e}")
        check_rows(rows[:1], ref_rows[:1], 2e-5)
        check_rows(rows, ref_rows, 1e-2)
        assert diff < 2e-2
    finally:
        _reset(eng)


def test_job_driver_with_avg_pooling(vgg_weights):
    """neural_style_transfer(..., pooling="avg") yields; its percent sequence is the max run's; its first-step loss is the
    engine-level avg closure of the same start image (and not the max run's)."""
    from artstyletransfer_amd import config, neural_nets
    from artstyletransfer_amd import neural_style_transfer as impl
    import neural_style_transfer as nst
    neural_nets.set_weights(vgg_weights)
    content = cpu_ref.synthetic_image(64, 96, seed=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=1, iters_num=3, optimizer="adam")
    seen = {}
    real_step = impl._DeviceJob.step

    def run(pooling):
        first = {}

        def step(self, cw, sw, tvw):
            if "x0" not in first:
                first["x0"] = self.x.clone()
            out = real_step(self, cw, sw, tvw)
            first.setdefault("rows", np.asarray(out[1]).copy())
            return out

        impl._DeviceJob.step = step

        async def go():
            out = []
            async for percent, img in nst.neural_style_transfer(
                    nst.ContentStylePair(("c", content), ("s", style)), cfg.content_weight, cfg.style_weight, cfg.tv_weight,
                    cfg.optimizer, cfg.model, "content", cfg.iters_num, cfg.levels_num, cfg.noise_factor,
                    cfg.noise_levels, cfg.noise_levels_central_amplitude, cfg.noise_levels_peripheral_amplitude,
                    cfg.noise_levels_dispersion, pooling=pooling):
                out.append((percent, img))
            return out

        try:
            out = asyncio.run(go())
        finally:
            impl._DeviceJob.step = real_step
        seen[pooling] = first
        return out

    out_avg, out_max = run("avg"), run("max")
    assert [round(p) for p, _ in out_avg] == [round(p) for p, _ in out_max] == [33, 67, 100]
    for _, img in out_avg:
        assert img.shape == (256, 384, 3) and np.isfinite(img).all()
    # the engine-level closure of the same start image under avg pooling (targets: the job's own level images)
    x0 = seen["avg"]["x0"]
    assert torch.equal(x0, seen["max"]["x0"])
    from artstyletransfer_amd import device_image
    setup_eng = neural_nets.shared_engine(torch.device("cuda", 0))
    c_lv = device_image.pyramid(setup_eng, device_image.upload(setup_eng, content), 1)
    s_lv = device_image.pyramid(setup_eng, device_image.upload(setup_eng, style), 1)
    from artstyletransfer_amd.engine import StyleEngine
    eng = StyleEngine(vgg_weights, 0)
    try:
        eng.configure(1, x0.shape[-2], x0.shape[-1])
        eng.set_pooling("avg")
        eng.set_targets(0, eng.prepare_img(c_lv[0].contiguous()), eng.prepare_img(s_lv[0].contiguous()))
        _, l = eng.closure(x0, cfg.content_weight, cfg.style_weight, cfg.tv_weight)
        l = l.cpu().numpy()
    finally:
        eng.close()
    first_avg = float(np.asarray(seen["avg"]["rows"]).reshape(-1)[-1])
    first_max = float(np.asarray(seen["max"]["rows"]).reshape(-1)[-1])
    assert first_avg == pytest.approx(float(l[-1]), rel=1e-6)
    assert abs(first_avg - first_max) > 1e-2 * abs(first_max)
