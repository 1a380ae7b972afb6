"""CPU: the host side of the TV-L1 flow estimator (nst_flow_tvl1_estimate in include/nst_hip.h;
artstyletransfer_amd/flow_modes.py, video.py, engine.flow_tvl1_workspace) and the fp64 restatement of its definitions
(tests/flow_tvl1_ref.py) beside Horn-Schunck's (tests/flow_ref.py) on the scenes tests/test_hip_flow_tvl1.py holds the device to.

What TV-L1 is here for: at a motion boundary its mean endpoint error is at most HALF of Horn-Schunck's, over the visible pixels
and over the band of 4 px either side of the moving rectangle's edge - asserted in fp64 on every scene, and on the two pure
translations of flow_ref.PAIRS.  Measured with the committed generator, defaults of both estimators, fp64 (px; HS -> TV-L1):
    48x64, bg (0,0), fg (3,1):          visible 0.273 -> 0.077, band 0.828 -> 0.200
    64x96, bg (-1.5,0.5), fg (4,-2):    visible 0.387 -> 0.106, band 1.450 -> 0.425
    48x64, bg (1,0), fg (-3,1.5):       visible 0.389 -> 0.126, band 0.971 -> 0.211
    flow_ref.PAIRS:                     0.0418 -> 0.0086 and 0.1013 -> 0.0151
The fp32 restatement sits 1.1e-6, 3.9e-6 and 8.7e-6 (rel-L2) from the fp64 one on the scenes, 1.9e-7 and 2.9e-7 on the pairs
(reported, not bounded: it is the yardstick of the device's bound, not a result)."""
import inspect
import os
import re

import numpy as np
import pytest

import flow_ref as hs
import flow_tvl1_ref as ref


@pytest.fixture(scope="module")
def scenes():
    """scene index -> (truth, visible, band, fp64 TV-L1 flow, fp32 TV-L1 flow, fp64 Horn-Schunck flow); computed once."""
    out = []
    for sc in ref.SCENES:
        A, B, truth, visible, band = ref.scene(*sc)
        out.append((truth, visible, band, ref.estimate(A, B, np.float64)[0], ref.estimate(A, B, np.float32)[0],
                    hs.estimate(A, B, np.float64)[0]))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_the_scenes_and_defaults_are_the_documented_ones():
    assert ref.DEFAULTS == dict(lambda_=0.15, theta=0.3, tau=0.25, scales=0, warps=5, iterations=50)
    assert [(s[0], s[1], s[3], s[4]) for s in ref.SCENES] == [(48, 64, (0.0, 0.0), (3.0, 1.0)), (64, 96, (-1.5, 0.5), (4.0, -2.0)),
                                                              (48, 64, (1.0, 0.0), (-3.0, 1.5))]
    for sc in ref.SCENES:
        h, w, _, t_bg, t_fg, rect = sc
        A, B, truth, visible, band = ref.scene(*sc)
        A2 = ref.scene(*sc)[0]
        assert A.shape == B.shape == (h, w) and A.dtype == B.dtype == np.float32 and np.array_equal(A, A2)
        assert 0.0 <= A.min() and A.max() <= 255.0 and A.std() > 20.0
        assert visible.mean() > 0.85 and 0.1 < band.mean() < 0.3 and not (band & ~visible).any()
        # both motions are there, and the truth says which pixel has which
        fg = (truth[0] == -t_fg[0]) & (truth[1] == -t_fg[1])
        area = (rect[1] - rect[0]) * (rect[3] - rect[2])
        assert 0.8 * area < fg.sum() <= area and ((truth[0] == -t_bg[0]) & (truth[1] == -t_bg[1]))[~fg].all()
        # the frames obey the truth where it is visible: `to` sampled at p + w(p) is `from`, up to the bilinear sampling
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        sx, sy = xx + truth[0], yy + truth[1]
        whole = visible & (sx == np.floor(sx)) & (sy == np.floor(sy))
        if whole.any():
            assert np.abs(B[sy[whole].astype(int), sx[whole].astype(int)] - A[whole]).max() < 1e-3


@pytest.mark.parametrize("k", range(len(ref.SCENES)))
def test_tvl1_halves_the_error_of_horn_schunck_at_a_motion_boundary(scenes, k):
    truth, visible, band, tv64, tv32, hs64 = scenes[k]
    for name, where in (("visible", visible), ("band", band)):
        e_tv, e_hs = ref.endpoint_error(tv64, truth, where), ref.endpoint_error(hs64, truth, where)
        print(f"scene {k} {ref.SCENES[k][:2]}: {name} EPE Horn-Schunck {e_hs:.3f} px, TV-L1 {e_tv:.3f} px (ratio {e_tv / e_hs:.2f})")
        assert e_tv <= 0.5 * e_hs, (k, name, e_tv, e_hs)
    d = float(np.linalg.norm(tv32.astype(np.float64) - tv64) / np.linalg.norm(tv64))
    print(f"scene {k}: fp32 restatement {d:.2e} (rel-L2) from the fp64 one")
    assert np.isfinite(tv32).all()


@pytest.mark.parametrize("k", range(len(hs.PAIRS)))
def test_tvl1_halves_the_error_of_horn_schunck_on_a_pure_translation(k):
    shape, t, seed = hs.PAIRS[k]
    A, B = hs.synthetic_pair(shape, t, seed)
    tv64, scales = ref.estimate(A, B, np.float64)
    tv32 = ref.estimate(A, B, np.float32)[0]
    e_tv, e_hs = hs.endpoint_error(tv64, t), hs.endpoint_error(hs.estimate(A, B, np.float64)[0], t)
    d = float(np.linalg.norm(tv32.astype(np.float64) - tv64) / np.linalg.norm(tv64))
    print(f"pair {shape} t={t}: {scales} scales, EPE Horn-Schunck {e_hs:.4f} px, TV-L1 {e_tv:.4f} px; fp32 restatement {d:.2e} from fp64")
    assert tv64.shape == (2,) + shape and scales == 3 and e_tv <= 0.5 * e_hs


def test_restatement_basics():
    """Identical frames: the flow is exactly zero.  Without a data term and with zero duals a flow stays as it is; the last
    column of p11, p21 and the last row of p12, p22 are read as 0 and come out 0; on a 1x1 plane every difference is 0."""
    A, _ = hs.synthetic_pair((33, 47), (0.0, 0.0), 5)
    rng = np.random.RandomState(1)
    for dt in (np.float64, np.float32):
        flow, scales = ref.estimate(A, A, dt, warps=2, iterations=3)
        assert not flow.any() and scales == 3
        z = np.zeros((4, 6))
        f = rng.uniform(-2, 2, (2, 4, 6)).astype(dt)
        out, dual = ref.iterate(z, z, z, f, np.zeros((4, 4, 6)), 0.15, 0.3, 0.25, 1, dt)
        assert np.array_equal(out, f) and dual.any()
        assert not dual[0][:, -1].any() and not dual[2][:, -1].any() and not dual[1][-1].any() and not dual[3][-1].any()
        d = rng.uniform(-0.9, 0.9, (4, 4, 6))
        masked = ref.read_duals(d, dt)
        a = ref.iterate(z + 3, z - 2, z + 1, f, d, 0.15, 0.3, 0.25, 2, dt)
        b = ref.iterate(z + 3, z - 2, z + 1, f, masked, 0.15, 0.3, 0.25, 2, dt)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and not np.array_equal(masked, d.astype(dt))
        one = ref.iterate([[2.0]], [[-1.0]], [[0.5]], [[[0.25]], [[-0.5]]], np.full((4, 1, 1), 0.7), 0.15, 0.3, 0.25, 3, dt)
        assert not one[1].any() and np.isfinite(one[0]).all()


def test_the_thresholding_step_is_continuous_in_rho():
    """k takes lt / -lt outside |r| <= lt g2 and -r / g2 inside, the same value at either edge."""
    ix, iy = np.full((1, 1), 3.0), np.full((1, 1), -4.0)          # g2 = 25, lt = 0.045, b = 1.125
    f, d = np.zeros((2, 1, 1)), np.zeros((4, 1, 1))
    u = [float(ref.iterate(ix, iy, np.full((1, 1), r), f, d, 0.15, 0.3, 0.25, 1, np.float64)[0][0, 0, 0])
         for r in (-5.0, -1.125 - 1e-9, -1.125 + 1e-9, 0.0, 1.125 - 1e-9, 1.125 + 1e-9, 5.0)]
    assert u[0] == pytest.approx(0.135) and u[-1] == pytest.approx(-0.135) and u[3] == 0.0
    assert u[1] == pytest.approx(u[2], abs=1e-9) and u[4] == pytest.approx(u[5], abs=1e-9)


# ---- TVL1Params ------------------------------------------------------------------------------------------------------------
def test_tvl1_params_defaults_and_normal_forms():
    from artstyletransfer_amd import flow_modes as fm
    assert fm.TVL1Params() == (0.15, 0.3, 0.25, 0, 5, 50) == fm.normalize_tvl1(None)
    assert fm.TVL1Params._fields == ("lambda_", "theta", "tau", "scales", "warps", "iterations")
    assert fm.normalize_tvl1({"iterations": 7, "lambda_": 0.2}) == fm.TVL1Params(lambda_=0.2, iterations=7)
    assert fm.normalize_tvl1(fm.TVL1Params(theta=np.float32(0.5), scales=np.int64(3))) == fm.TVL1Params(0.15, 0.5, 0.25, 3, 5, 50)
    p = fm.normalize_tvl1(fm.TVL1Params(lambda_=1, theta=1, tau=1, scales=12, warps=1, iterations=1))
    assert [type(v) for v in p] == [float, float, float, int, int, int]
    assert fm.normalize_tvl1(dict(lambda_=2e-19, theta=1e-19)).lambda_ == 2e-19          # lt = 2e-38: still normal
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", inspect.getsource(fm), flags=re.M)
    # FlowParams and its normaliser are as they were
    assert fm.FlowParams() == (15.0, 0, 5, 50) == fm.normalize_flow(None) and fm.FlowParams._fields == ("alpha", "scales", "warps", "iterations")


@pytest.mark.parametrize("bad", [
    dict(lambda_=0.0), dict(lambda_=-0.15), dict(lambda_=float("nan")), dict(lambda_=float("inf")), dict(lambda_=1e39), dict(lambda_=1e-60),
    dict(lambda_="0.15"), dict(lambda_=True), dict(lambda_=None), dict(theta=0.0), dict(theta=-0.3), dict(theta=float("nan")),
    dict(theta=float("inf")), dict(theta=None), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau="x"),
    dict(lambda_=1e-20, theta=1e-20),          # lt underflows to a subnormal
    dict(lambda_=1e20, theta=1e20),            # lt overflows
    dict(tau=1e-20, theta=1e20),               # taut underflows
    dict(tau=1e20, theta=1e-20),               # taut overflows
    dict(scales=-1), dict(scales=13), dict(scales=1.5), dict(scales=True), dict(warps=0), dict(warps=2.0), dict(iterations=0),
    dict(iterations=-3), dict(iterations="50"), dict(iterations=2 ** 31)])
def test_normalize_tvl1_refuses(bad):
    from artstyletransfer_amd import flow_modes as fm
    with pytest.raises(ValueError):
        fm.normalize_tvl1(fm.TVL1Params(**bad))
    with pytest.raises(ValueError):
        fm.normalize_tvl1(bad)


def test_normalize_tvl1_refuses_other_types_and_normalize_flow_still_refuses_a_tvl1params():
    from artstyletransfer_amd import flow_modes as fm
    for bad in ("tvl1", 0.15, [0.15, 0.3, 0.25], (0.15, 0.3, 0.25), (0.15, 0.3, 0.25, 0, 5, 50), {"lambda": 0.15}, {"alpha": 15.0},
                fm.FlowParams(), object()):
        with pytest.raises(ValueError):
            fm.normalize_tvl1(bad)
    with pytest.raises(ValueError):
        fm.normalize_flow(fm.TVL1Params())
    with pytest.raises(ValueError):
        fm.normalize_flow(fm.TVL1Params(scales=1))


# ---- the video driver ------------------------------------------------------------------------------------------------------------
FRAMES = [np.zeros((64, 96, 3), np.float32)] * 3
STYLE = np.zeros((64, 96, 3), np.float32)
H, W = 512, 768                    # what a two-level job yields for a 64 x 96 frame


def _cfg():
    from artstyletransfer_amd import config
    return config.Config(levels_num=2, iters_num=2, optimizer="adam", init_method="content")


def _first(gen):
    import asyncio

    async def go():
        try:
            return await gen.__anext__()
        finally:
            await gen.aclose()
    return asyncio.run(go())


@pytest.mark.parametrize("kw,match", [
    (dict(backward_flows=dict(lambda_=-1.0)), "TV-L1 flow lambda_"),
    (dict(backward_flows=dict(theta=0.0)), "TV-L1 flow lambda_"),
    (dict(backward_flows=dict(scales=13)), "flow scales"),
    (dict(backward_flows=dict(iterations=0)), "flow iterations"),
    (dict(backward_flows={}, forward_flows=[np.zeros((H, W, 2), np.float32)] * 2), "forward_flows cannot be combined"),
])
def test_video_driver_refuses_tvl1_parameters_before_any_gpu_work(monkeypatch, kw, match):
    from artstyletransfer_amd import flow_modes as fm, video
    from artstyletransfer_amd import neural_style_transfer as impl

    def reached(*a, **k):
        raise AssertionError("GPU work was reached")

    monkeypatch.setattr(impl, "shared_engine", reached)
    monkeypatch.setattr(impl, "_make_job", reached)
    kw = dict(kw)
    params = fm.TVL1Params(**kw.pop("backward_flows"))
    gen = video.neural_style_transfer_video(FRAMES, STYLE, params, kw.pop("forward_flows", None), cfg=_cfg(), temporal_weight=1.0)
    with pytest.raises(ValueError, match=match):
        _first(gen)


def test_video_driver_hands_a_tvl1params_to_both_estimates(monkeypatch):
    """The start callable of frame 1 with backward_flows = a TVL1Params: the backward estimate (frame 1 -> frame 0) and the
    forward one get the normalised TVL1Params - the engine dispatches on its type."""
    import asyncio

    import torch

    from artstyletransfer_amd import flow_modes as fm, video
    from artstyletransfer_amd import neural_style_transfer as impl
    starts, log = [], []

    async def fake_plain(pair, *a, **kw):
        yield 100.0, np.full((H, W, 3), 0.5, np.float32)

    def fake_from(pair, *a, device=None, start=None, **kw):
        starts.append(start)

        async def gen():
            yield 100.0, np.full((H, W, 3), 0.75, np.float32)
        return gen()

    monkeypatch.setattr(impl, "neural_style_transfer", fake_plain)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    frames = [np.full((64, 96, 3), v, np.float32) for v in (0.1, 0.2)]
    given = fm.TVL1Params(lambda_=np.float32(0.25), iterations=np.int64(7))

    async def go():
        return [i async for i, _, _ in video.neural_style_transfer_video(frames, STYLE, given, temporal_weight=2.0, cfg=_cfg())]

    assert asyncio.run(go()) == [0, 1] and len(starts) == 1

    class Setup:
        device = torch.device("cpu")

        def resize(self, img, nh, nw):
            return img[:1, :1].expand(nh, nw, 3).contiguous()

        def luminance(self, hwc):
            return (255.0 * hwc[..., 0])[None, None].contiguous()

        def flow_estimate(self, a, b, p):
            log.append((round(float(a[0, 0]) / 255.0, 3), round(float(b[0, 0]) / 255.0, 3), p))
            return torch.zeros((2, H, W))

        def flow_weights(self, fwd, bwd):
            return torch.ones((H, W))

        def warp_bilinear(self, src, flow):
            return src.clone(), torch.ones((H, W))

        def prepare_img(self, hwc):
            return hwc.permute(2, 0, 1)[None].contiguous()

        def bicubic_half(self, x):
            return x[:, :, ::2, ::2].contiguous()

    starts[0](Setup(), (H, W))
    want = fm.TVL1Params(0.25, 0.3, 0.25, 0, 5, 7)
    assert log == [(0.2, 0.1, want), (0.1, 0.2, want)]
    assert all(type(p) is fm.TVL1Params and [type(v) for v in p] == [float, float, float, int, int, int] for _, _, p in log)


def test_the_flows_are_still_no_job_setting_and_the_signatures_stay():
    from artstyletransfer_amd import config, job_settings, video
    from artstyletransfer_amd import neural_style_transfer as impl
    assert not any("flow" in k or "tvl1" in k for k in job_settings.KEYWORDS)
    assert not any("flow" in a or "tvl1" in a for a in vars(config.Config()))
    p = inspect.signature(video.neural_style_transfer_video).parameters
    assert list(p) == ["frames", "style", "backward_flows", "forward_flows", "weights", "temporal_weight", "cfg", "device"]
    assert p["backward_flows"].default is None
    assert not any("flow" in k for k in inspect.signature(impl.neural_style_transfer).parameters)


# ---- the workspace and the bindings ------------------------------------------------------------------------------------------
def test_tvl1_workspace_is_the_horn_schunck_one_plus_two_copies_of_the_duals():
    from artstyletransfer_amd import _lib, engine
    for h, w in ((1, 1), (7, 9), (16, 16), (33, 47), (48, 64), (512, 768), (1024, 1536)):
        for scales in (0, 1, 2, 12):
            floats, used = engine.flow_tvl1_workspace(h, w, scales)
            base, base_used = engine.flow_workspace(h, w, scales)
            assert used == base_used == hs.scales_used(h, w, scales)
            assert base + 8 * h * w <= floats <= base + 8 * h * w + 8, (h, w, scales)
    for bad in ((0, 5, 0), (5, 0, 0), (-1, 5, 0), (5, 5, -1), (5, 5, 13)):
        with pytest.raises(ValueError):
            engine.flow_tvl1_workspace(*bad)
    assert _lib.load().nst_flow_tvl1_workspace(48, 64, 0, None, None) == _lib.NST_OK          # either pointer may be null


def test_tvl1_bindings_match_the_header():
    from artstyletransfer_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    for name, nargs in (("nst_flow_tvl1_workspace", 5), ("nst_flow_tvl1_estimate", 15), ("nst_flow_tvl1_iterations", 16)):
        m = re.search(r"\nint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(decl.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    assert re.search(r"Zach, Pock & Bischof", hdr) and re.search(r"Sanchez, Meinhardt-Llopis & Facciolo", hdr)
