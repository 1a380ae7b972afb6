"""CPU: the host side of the flow estimator (nst_flow_estimate in include/nst_hip.h; artstyletransfer_amd/flow_modes.py,
video.py) and the fp64 restatement of its definitions (tests/flow_ref.py) on the synthetic pairs tests/test_hip_flow.py
holds the device to.

The restatement recovers the known translations: mean endpoint error below 0.5 px at the default parameters (measured with
the committed generator: 0.042 px on the 48x64 pair, t = (-3.25, 2.0), and 0.101 px on the 33x47 pair, t = (1.5, 0.5); three
scales each).

Sample positions and inside-flag flips: no sample position of any linearise step may lie within 1e-3 px of a flip (the
positions 0 and n - 1 of an axis), at the defaults and with scales=1 - the two parameter sets of the GPU pipeline test, whose
comparison of fp32 with fp64 is well-posed only then.  Measured: 2.0e-3 and 2.2e-3 px on the 48x64 pair (whose integer ty
puts row h - 3 next to a flip: flow_ref.PAIRS says how its seed was picked), 1.2e-2 and 3.3e-3 px on the 33x47 pair."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flow_ref as ref

PARAM_SETS = ({}, {"scales": 1})        # what tests/test_hip_flow.py runs the pipeline with


@pytest.fixture(scope="module")
def estimates():
    """(pair index, parameter set index) -> (fp64 flow, scales used, smallest flip distance); computed once."""
    out = {}
    for k, (shape, t, seed) in enumerate(ref.PAIRS):
        A, B = ref.synthetic_pair(shape, t, seed)
        for j, kw in enumerate(PARAM_SETS):
            out[k, j] = ref.estimate(A, B, np.float64, **kw)
    return out


# ---- the restatement on the synthetic pairs -------------------------------------------------------------------------------
def test_the_pairs_and_defaults_are_the_documented_ones():
    assert [(s, t) for s, t, _ in ref.PAIRS] == [((48, 64), (-3.25, 2.0)), ((33, 47), (1.5, 0.5))]
    assert ref.DEFAULTS == dict(alpha=15.0, scales=0, warps=5, iterations=50)
    for shape, t, seed in ref.PAIRS:
        A, B = ref.synthetic_pair(shape, t, seed)
        A2, _ = ref.synthetic_pair(shape, t, seed)
        assert A.shape == B.shape == shape and A.dtype == B.dtype == np.float32 and np.array_equal(A, A2)
        assert A.min() >= 0.0 and A.max() <= 255.0 and A.std() > 20.0 and not np.array_equal(A, B)


@pytest.mark.parametrize("k", range(len(ref.PAIRS)))
def test_fp64_restatement_recovers_the_translation(estimates, k):
    shape, t, _ = ref.PAIRS[k]
    flow, scales, _ = estimates[k, 0]
    epe = ref.endpoint_error(flow, t)
    print(f"pair {shape} t={t}: {scales} scales, mean endpoint error {epe:.4f} px")
    assert flow.shape == (2,) + shape and scales == 3
    assert epe < 0.5


@pytest.mark.parametrize("j", range(len(PARAM_SETS)))
@pytest.mark.parametrize("k", range(len(ref.PAIRS)))
def test_no_sample_position_within_1e_3_px_of_a_flag_flip(estimates, k, j):
    near = estimates[k, j][2]
    print(f"pair {ref.PAIRS[k][0]} {PARAM_SETS[j]}: smallest distance of a sample position from a flag flip {near:.3e} px")
    assert near >= 1e-3


def test_restatement_basics():
    """Identical frames: the flow is exactly zero.  reduce keeps a constant; prolong doubles a constant; a sweep without a
    data term keeps a constant flow."""
    A, _ = ref.synthetic_pair((33, 47), (0.0, 0.0), 5)
    for dt in (np.float64, np.float32):
        flow, scales, near = ref.estimate(A, A, dt, warps=2, iterations=3)
        assert not flow.any() and scales == 3 and near == float("inf")
        assert np.array_equal(ref.reduce(np.full((5, 7), 3.0), dt), np.full((3, 4), 3.0, dt))
        assert np.array_equal(ref.prolong(np.full((2, 3, 4), 1.5), 5, 7, dt), np.full((2, 5, 7), 3.0, dt))
        z = np.zeros((4, 6))
        f = np.stack([np.full((4, 6), 0.75), np.full((4, 6), -1.25)])
        assert np.allclose(ref.sweeps(z, z, z, f, 15.0, 3, dt), f, rtol=1e-6)
    assert ref.flip_distance(np.full((2, 4, 6), 0.25)) == pytest.approx(0.25)
    assert [ref.scales_used(h, w, s) for h, w, s in ((48, 64, 0), (33, 47, 0), (48, 64, 2), (14, 200, 0), (16, 16, 0), (1, 1, 0),
                                                    (1024, 1536, 0), (10 ** 5, 10 ** 5, 0))] == [3, 3, 2, 1, 2, 1, 8, 12]


# ---- FlowParams ------------------------------------------------------------------------------------------------------------------
def test_flow_params_defaults_and_normal_forms():
    from artstyletransfer_amd import flow_modes as fm
    from artstyletransfer_amd import _lib
    assert fm.FlowParams() == (15.0, 0, 5, 50) == fm.normalize_flow(None) and fm.MAX_SCALES == _lib.NST_MAX_FLOW_SCALES == 12
    assert fm.normalize_flow((1e-18,)).alpha == 1e-18 and fm.normalize_flow((1e19,)).alpha == 1e19
    assert fm.normalize_flow(fm.FlowParams(alpha=np.float32(8), scales=np.int64(3))) == fm.FlowParams(8.0, 3, 5, 50)
    assert fm.normalize_flow({"iterations": 7}) == fm.FlowParams(iterations=7)
    assert fm.normalize_flow((20, 1)) == fm.FlowParams(20.0, 1, 5, 50)
    p = fm.normalize_flow(fm.FlowParams(alpha=1, scales=12, warps=1, iterations=1))
    assert [type(v) for v in p] == [float, int, int, int]
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy)", inspect.getsource(fm), flags=re.M)


@pytest.mark.parametrize("bad", [
    dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=1e39), dict(alpha=1e-60), dict(alpha=1e-30), dict(alpha=1e-22), dict(alpha=1e20), dict(alpha="15"),
    dict(alpha=True), dict(alpha=None), dict(scales=-1), dict(scales=13), dict(scales=1.5), dict(scales=True), dict(warps=0),
    dict(warps=2.0), dict(iterations=0), dict(iterations=-3), dict(iterations="50"), dict(iterations=2 ** 31)])
def test_normalize_flow_refuses(bad):
    from artstyletransfer_amd import flow_modes as fm
    with pytest.raises(ValueError):
        fm.normalize_flow(fm.FlowParams(**bad))
    with pytest.raises(ValueError):
        fm.normalize_flow(bad)


@pytest.mark.parametrize("bad", ["default", 15.0, [15.0, 0, 5, 50], (15.0, 0, 5, 50, 1), {"alpha": 15.0, "levels": 3}, object()])
def test_normalize_flow_refuses_other_types(bad):
    from artstyletransfer_amd import flow_modes as fm
    with pytest.raises(ValueError):
        fm.normalize_flow(bad)


# ---- the video driver ------------------------------------------------------------------------------------------------------------
FRAMES = [np.zeros((64, 96, 3), np.float32)] * 3
STYLE = np.zeros((64, 96, 3), np.float32)
H, W = 512, 768                    # what a two-level job yields for a 64 x 96 frame


def _cfg(**kw):
    from artstyletransfer_amd import config
    return config.Config(levels_num=2, iters_num=2, optimizer="adam", init_method="content", **kw)


def _no_gpu_work(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl

    def reached(*a, **k):
        raise AssertionError("GPU work was reached")

    monkeypatch.setattr(impl, "shared_engine", reached)
    monkeypatch.setattr(impl, "_make_job", reached)


def _first(gen):
    async def go():
        try:
            return await gen.__anext__()
        finally:
            await gen.aclose()
    return asyncio.run(go())


def test_backward_flows_default_to_none_and_the_parameter_list_stays():
    from artstyletransfer_amd import video
    p = inspect.signature(video.neural_style_transfer_video).parameters
    assert list(p) == ["frames", "style", "backward_flows", "forward_flows", "weights", "temporal_weight", "cfg", "device"]
    assert p["backward_flows"].default is None and p["forward_flows"].default is None and p["weights"].default is None
    assert p["temporal_weight"].default is inspect.Parameter.empty
    assert "caller supplies the flows" not in (video.__doc__ + video.neural_style_transfer_video.__doc__)


@pytest.mark.parametrize("what,kw,match", [
    ("forward flows beside estimated ones", dict(forward_flows=[np.zeros((H, W, 2), np.float32)] * 2), "forward_flows cannot be combined"),
    ("the same with parameters", dict(backward_flows="params", forward_flows=[np.zeros((H, W, 2), np.float32)] * 2),
     "forward_flows cannot be combined"),
    ("bad alpha", dict(backward_flows=dict(alpha=-1.0)), "flow alpha"),
    ("bad scales", dict(backward_flows=dict(scales=13)), "flow scales"),
    ("bad warps", dict(backward_flows=dict(warps=0)), "flow warps"),
    ("bad iterations", dict(backward_flows=dict(iterations=0)), "flow iterations"),
    ("weights still checked", dict(weights=[np.ones((H, W), np.float32)]), "weights: expected 2"),
    ("temporal weight still checked", dict(temporal_weight=-1.0), "temporal_weight must be finite"),
])
def test_video_driver_refuses_before_any_gpu_work(monkeypatch, what, kw, match):
    from artstyletransfer_amd import flow_modes as fm, video
    _no_gpu_work(monkeypatch)
    args = dict(backward_flows=None, forward_flows=None, weights=None, temporal_weight=1.0)
    args.update(kw)
    b = args.pop("backward_flows")
    b = fm.FlowParams() if b == "params" else fm.FlowParams(**b) if isinstance(b, dict) else b
    gen = video.neural_style_transfer_video(FRAMES, STYLE, b, args.pop("forward_flows"), args.pop("weights"), cfg=_cfg(), **args)
    with pytest.raises(ValueError, match=match):
        _first(gen)


@pytest.mark.parametrize("given_weights", [False, True])
@pytest.mark.parametrize("params", [None, (8.0, 2, 3, 4)])
def test_video_driver_estimates_between_the_luminance_planes_at_the_yielded_size(monkeypatch, params, given_weights):
    """The start callable of frame 1: both frames resized to the yielded size, their luminance planes, the backward flow as
    estimate(frame 1, frame 0); the forward flow and flow_weights only when no weights are given."""
    from artstyletransfer_amd import flow_modes as fm, video
    from artstyletransfer_amd import neural_style_transfer as impl
    starts = []

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
    wts = [np.full((H, W), 0.5, np.float32)] if given_weights else None
    fp = None if params is None else fm.FlowParams(*params)

    async def go():
        return [i async for i, _, _ in video.neural_style_transfer_video(frames, STYLE, fp, weights=wts, temporal_weight=2.0, cfg=_cfg())]

    assert asyncio.run(go()) == [0, 1] and len(starts) == 1
    log = []

    class Setup:
        device = torch.device("cpu")

        def resize(self, img, nh, nw):
            log.append(("resize", tuple(img.shape), nh, nw))
            return img[:1, :1].expand(nh, nw, 3).contiguous()

        def luminance(self, hwc):
            log.append(("luminance", tuple(hwc.shape)))
            return (255.0 * hwc[..., 0])[None, None].contiguous()

        def flow_estimate(self, a, b, p):
            log.append(("estimate", round(float(a[0, 0]) / 255.0, 3), round(float(b[0, 0]) / 255.0, 3), p))
            assert tuple(a.shape) == tuple(b.shape) == (H, W)
            return torch.full((2, H, W), float(a[0, 0]))

        def flow_weights(self, fwd, bwd):
            log.append(("weights", round(float(fwd[0, 0, 0]) / 255.0, 3), round(float(bwd[0, 0, 0]) / 255.0, 3)))
            return torch.ones((H, W))

        def warp_bilinear(self, src, flow):
            log.append(("warp", round(float(flow[0, 0, 0]) / 255.0, 3)))
            return src.clone(), torch.ones((H, W))

        def prepare_img(self, hwc):
            return hwc.permute(2, 0, 1)[None].contiguous()

        def bicubic_half(self, x):
            return x[:, :, ::2, ::2].contiguous()

    omega, anchors, weights, gamma = starts[0](Setup(), (H, W))
    want = fm.normalize_flow(fp)
    est = [e for e in log if e[0] == "estimate"]
    assert est[0] == ("estimate", 0.2, 0.1, want)                       # backward: frame 1 -> frame 0
    assert ("warp", 0.2) in log and gamma == 2.0 and tuple(omega.shape) == (H, W, 3)
    assert [e for e in log if e[0] == "resize"][:2] == [("resize", (64, 96, 3), H, W)] * 2
    if given_weights:
        assert len(est) == 1 and not [e for e in log if e[0] == "weights"]
        assert float(weights[0][0, 0]) == 0.5
    else:
        assert est[1] == ("estimate", 0.1, 0.2, want) and ("weights", 0.1, 0.2) in log      # forward: frame 0 -> frame 1
        assert float(weights[0][0, 0]) == 1.0


def test_video_driver_forms_each_luminance_plane_once(monkeypatch):
    """Three frames: frame 1's plane, formed for its own backward flow, is read again as frame 2's previous plane."""
    from artstyletransfer_amd import video
    from artstyletransfer_amd import neural_style_transfer as impl
    starts, resized = [], []

    async def fake_plain(pair, *a, **kw):
        yield 100.0, np.full((H, W, 3), 0.5, np.float32)

    def fake_from(pair, *a, device=None, start=None, **kw):
        starts.append(start)

        async def gen():
            yield 100.0, np.full((H, W, 3), 0.75, np.float32)
        return gen()

    monkeypatch.setattr(impl, "neural_style_transfer", fake_plain)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    frames = [np.full((64, 96, 3), v, np.float32) for v in (0.1, 0.2, 0.3)]

    async def go():
        return [i async for i, _, _ in video.neural_style_transfer_video(frames, STYLE, temporal_weight=2.0, cfg=_cfg())]

    assert asyncio.run(go()) == [0, 1, 2] and len(starts) == 2
    pairs = []

    class Setup:
        device = torch.device("cpu")

        def resize(self, img, nh, nw):
            resized.append(round(float(img[0, 0, 0]), 3))
            return img[:1, :1].expand(nh, nw, 3).contiguous()

        def luminance(self, hwc):
            return hwc[..., 0][None, None].contiguous()

        def flow_estimate(self, a, b, p):
            pairs.append((round(float(a[0, 0]), 3), round(float(b[0, 0]), 3)))
            return torch.zeros((2, H, W))

        def flow_weights(self, fwd, bwd):
            return torch.ones((H, W))

        def warp_bilinear(self, src, flow):
            return src.clone(), torch.ones((H, W))

        def prepare_img(self, hwc):
            return hwc.permute(2, 0, 1)[None].contiguous()

        def bicubic_half(self, x):
            return x[:, :, ::2, ::2].contiguous()

    for start in starts:
        start(Setup(), (H, W))
    assert sorted(resized) == [0.1, 0.2, 0.3]
    assert pairs == [(0.2, 0.1), (0.1, 0.2), (0.3, 0.2), (0.2, 0.3)]


def test_the_flows_are_no_job_setting():
    from artstyletransfer_amd import config, job_settings
    assert not any("flow" in k for k in job_settings.KEYWORDS) and not any("flow" in k for k in job_settings.KEYS)
    assert not any("flow" in a for a in vars(config.Config()))


# ---- the workspace: a pure function of the library ------------------------------------------------------------------------------
def test_flow_workspace_is_monotone_and_reports_the_scales():
    from artstyletransfer_amd import _lib, engine
    for h, w in ((1, 1), (7, 9), (15, 16), (16, 16), (33, 47), (48, 64), (100, 37), (512, 768), (1024, 1536)):
        for scales in (0, 1, 2, 5, 12):
            floats, used = engine.flow_workspace(h, w, scales)
            assert used == ref.scales_used(h, w, scales), (h, w, scales)
            # the planes the definitions need: both pyramids above scale 0, Ix, Iy, rho and a second flow buffer
            need, hs, ws = 5 * h * w, h, w
            for _ in range(1, used):
                hs, ws = (hs + 1) // 2, (ws + 1) // 2
                need += 2 * hs * ws
            assert need <= floats <= need + 4 * (2 * used + 2), (h, w, scales)
            assert engine.flow_workspace(h + 1, w, scales)[0] >= floats and engine.flow_workspace(h, w + 1, scales)[0] >= floats
        assert engine.flow_workspace(h, w, 0) == engine.flow_workspace(h, w, 12)
        assert [engine.flow_workspace(h, w, s)[0] for s in range(1, 12)] == sorted(engine.flow_workspace(h, w, s)[0] for s in range(1, 12))
    for bad in ((0, 5, 0), (5, 0, 0), (-1, 5, 0), (5, 5, -1), (5, 5, 13)):
        with pytest.raises(ValueError):
            engine.flow_workspace(*bad)
    assert _lib.load().nst_flow_workspace(48, 64, 0, None, None) == _lib.NST_OK          # either pointer may be null
    assert _lib.NST_MAX_FLOW_SCALES == 12


def test_flow_bindings_match_the_header():
    from artstyletransfer_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert "#define NST_MAX_FLOW_SCALES 12 " in hdr
    for name, nargs in (("nst_flow_workspace", 5), ("nst_flow_estimate", 13), ("nst_flow_reduce", 6), ("nst_flow_prolong", 6),
                        ("nst_flow_linearize", 10), ("nst_flow_sweeps", 12)):
        m = re.search(r"\nint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(decl.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    assert re.search(r"Horn & Schunck", hdr) and re.search(r"Meinhardt-Llopis, Sanchez & Kondermann", hdr)
