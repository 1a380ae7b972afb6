"""CPU: the host side of the long-term anchor (video.neural_style_transfer_video_long_term, video.long_term_anchor,
StyleEngine.anchor_fold / nst_anchor_fold): the properties of the fp64 restatement the GPU tests compare against
(tests/long_term_ref.py), what the driver refuses before any GPU work, which flows it estimates and what it keeps, and that
without long_term it reaches the code it reached."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest
import torch

import long_term_ref as ref


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


FRAMES = [np.zeros((64, 96, 3), np.float32)] * 4
STYLE = np.zeros((64, 96, 3), np.float32)
H, W = 512, 768                    # what a two-level job yields for a 64 x 96 frame


def _flows(n, shape=(H, W, 2)):
    return [np.zeros(shape, np.float32)] * n


def _planes(n, value=1.0, shape=(H, W)):
    return [np.full(shape, value, np.float32)] * n


# ---- the restatement's own properties ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 2, 3, 8])
def test_restatement_weight_is_at_most_one_and_the_gradient_identity_holds(J):
    h, w, C = 40, 50, 3
    weights = ref.random_weights(J, h, w, seed=10 + J)
    assert all((c == 0).mean() > 0.15 and (c == 1).mean() > 0.15 for c in weights)
    sources = ref.random_sources(J, C, h, w, seed=20 + J)
    for dtype in (np.float32, np.float64):
        parts, wsum = ref.parts_of(weights, dtype)
        assert parts.dtype == dtype and (parts >= 0).all() and wsum.max() <= 1.0, (dtype, float(wsum.max()))
    anchor, weight, parts, wsum = ref.fold(sources, weights)
    y = np.random.RandomState(J).uniform(-120.0, 135.0, (C, h, w))
    lhs = sum(parts[j][None] * (y - np.where(parts[j][None] > 0, sources[j].astype(np.float64), 0.0)) for j in range(J))
    rhs = weight[None] * (y - anchor)
    assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(lhs).max()
    # the incremental form of the header is the weighted mean
    abar, wbar = ref.mean_anchor(sources, parts)
    assert np.abs(abar - anchor).max() <= 1e-12 * np.abs(anchor).max() and np.abs(wbar - weight).max() <= 1e-15
    # the loss values differ by the constant: sum_j l_j (y - a_j)^2 = W (y - a~)^2 + sum_j l_j (a_j - a~)^2
    full = sum(float((parts[j][None] * np.where(parts[j][None] > 0, y - sources[j], 0.0) ** 2).sum()) for j in range(J)) / y.size
    folded = float((weight[None] * (y - anchor) ** 2).sum()) / y.size
    assert full - folded == pytest.approx(ref.constant(sources, parts), rel=1e-9, abs=1e-9 * full)
    assert (ref.constant(sources, parts) > 0) == (J > 1)


@pytest.mark.parametrize("J", [1, 2, 3, 8])
def test_restatement_binary_weights_give_disjoint_parts_and_no_constant(J):
    h, w, C = 24, 36, 3
    rng = np.random.RandomState(30 + J)
    weights = [(rng.uniform(size=(h, w)) < 0.4).astype(np.float32) for _ in range(J)]
    sources = ref.random_sources(J, C, h, w, seed=40 + J)
    anchor, weight, parts, _ = ref.fold(sources, weights)
    assert set(np.unique(parts)) <= {0.0, 1.0} and set(np.unique(weight)) <= {0.0, 1.0}
    assert (parts.sum(0) <= 1).all() and np.array_equal(parts.sum(0), weight)
    assert np.array_equal(weight, np.max(weights, axis=0))                  # covered by any source: covered
    first = np.argmax(np.stack(weights), axis=0)                            # the nearest reliable source (0 where none)
    want = np.choose(first[None], [s.astype(np.float64) for s in sources])
    assert np.array_equal(anchor, want)
    assert ref.constant(sources, parts) == 0.0
    # and in fp32 the same select, bit for bit
    a32 = ref.fold(sources, weights, np.float32)[0]
    assert np.array_equal(a32, want.astype(np.float32)) and np.array_equal(ref.fold_torch(sources, weights), a32)


def test_restatement_sanitises_the_weights_and_does_not_leak_dead_sources():
    w0 = np.array([[np.nan, -0.5, 1.5, 0.25, 0.0]], np.float32)
    w1 = np.ones((1, 5), np.float32)
    s0 = np.full((1, 1, 5), 7.0, np.float32)
    s1 = np.full((1, 1, 5), 9.0, np.float32)
    s1[0, 0, 2] = np.nan                                                    # dead there: source 0 has weight 1.5 -> 1
    anchor, weight, parts, _ = ref.fold([s0, s1], [w0, w1])
    assert np.array_equal(parts[0], [[0, 0, 1, 0.25, 0]]) and np.array_equal(parts[1], [[1, 1, 0, 0.75, 1]])
    assert np.array_equal(weight, np.ones((1, 5)))
    assert np.array_equal(anchor[0], [[9, 9, 7, 7 + 0.75 * 2, 9]])


# ---- the driver's refusals -----------------------------------------------------------------------------------------------------
def _lt(j, n=4, **kw):
    entry = [_flows(n - j), kw.get("forward"), kw.get("weights")]
    if "backward" in kw:
        entry[0] = kw["backward"]
    return {j: tuple(entry)}


@pytest.mark.parametrize("what,kw,match", [
    ("offset below two", dict(long_term=(1,)), "offsets are >= 2"),
    ("offset zero", dict(long_term=(2, 0)), "offsets are >= 2"),
    ("duplicate offsets", dict(long_term=(2, 4, 2)), "must be distinct"),
    ("float offset", dict(long_term=(2.0,)), "offsets are integers"),
    ("bool offset", dict(long_term=(True,)), "offsets are integers"),
    ("too many offsets", dict(long_term=tuple(range(2, 10))), "at most 7 offsets"),
    ("flows without offsets", dict(backward_flows=_flows(3), long_term_flows=_lt(2)), "long_term_flows without long_term"),
    ("other keys", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows=_lt(3)), "its keys must be the offsets"),
    ("a key missing", dict(backward_flows=_flows(3), long_term=(2, 3), long_term_flows=_lt(2)), "its keys must be the offsets"),
    ("backward count", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows=_lt(2, backward=_flows(3))),
     r"long_term_flows\[2\] backward: expected 2 entries"),
    ("backward shape", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows=_lt(2, backward=_flows(2, (64, 96, 2)))),
     r"long_term_flows\[2\] backward\[0\]: expected shape"),
    ("forward count", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows=_lt(2, forward=_flows(1))),
     r"long_term_flows\[2\] forward: expected 2 entries"),
    ("weights shape", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows=_lt(2, weights=_planes(2, shape=(H, W, 1)))),
     r"long_term_flows\[2\] weights\[0\]: expected shape"),
    ("weights above one", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows=_lt(2, weights=_planes(2, 1.5))),
     r"long_term_flows\[2\] weights\[0\]: values must lie"),
    ("weights nan", dict(backward_flows=_flows(3), long_term=(3,), long_term_flows=_lt(3, weights=_planes(1, np.nan))),
     r"long_term_flows\[3\] weights\[0\]: values must lie"),
    ("no triple", dict(backward_flows=_flows(3), long_term=(2,), long_term_flows={2: (_flows(2),)}), "expected .backward, forward, weights"),
    ("flows beside estimated ones", dict(long_term=(2,), long_term_flows=_lt(2)), "cannot be combined with estimated backward flows"),
    ("offsets beside caller flows alone", dict(backward_flows=_flows(3), long_term=(2,)), "needs long_term_flows"),
    ("offset-1 checks stay", dict(backward_flows=_flows(2), long_term=(2,), long_term_flows=_lt(2)), "backward_flows: expected 3"),
])
def test_long_term_driver_refuses_before_any_gpu_work(monkeypatch, what, kw, match):
    from artstyletransfer_amd import video
    _no_gpu_work(monkeypatch)
    args = dict(backward_flows=None, temporal_weight=1.0)
    args.update(kw)
    gen = video.neural_style_transfer_video_long_term(FRAMES, STYLE, args.pop("backward_flows"), cfg=_cfg(), **args)
    with pytest.raises(ValueError, match=match):
        _first(gen)


def test_offsets_are_normalised_to_ascending_order():
    from artstyletransfer_amd import video
    assert video.normalize_long_term(None) is None and video.normalize_long_term(()) == ()
    assert video.normalize_long_term([4, np.int64(2), 8]) == (2, 4, 8)
    assert video.normalize_long_term(range(2, 9)) == (2, 3, 4, 5, 6, 7, 8) and video.MAX_LONG_TERM == 7
    p = inspect.signature(video.neural_style_transfer_video_long_term).parameters
    assert list(p) == list(inspect.signature(video.neural_style_transfer_video).parameters) + ["long_term", "long_term_flows"]
    assert p["long_term"].default is None and p["long_term_flows"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("temporal_weight", "cfg", "device", "long_term", "long_term_flows"))


# ---- what the driver does ---------------------------------------------------------------------------------------------------------
class _Setup:
    """An engine that records its calls; values carry the frame they came from."""
    device = torch.device("cpu")

    def __init__(self):
        self.log = []

    def resize(self, img, nh, nw):
        self.log.append(("resize", round(float(img[0, 0, 0]), 3)))
        return img[:1, :1].expand(nh, nw, 3).contiguous()

    def luminance(self, hwc):
        return hwc[..., 0][None, None].contiguous()

    def flow_estimate(self, a, b, p):
        self.log.append(("estimate", round(float(a[0, 0]), 3), round(float(b[0, 0]), 3)))
        return torch.full((2, H, W), float(a[0, 0]) - float(b[0, 0]))

    def flow_weights(self, fwd, bwd):
        self.log.append(("weights", round(float(fwd[0, 0, 0]), 3), round(float(bwd[0, 0, 0]), 3)))
        return torch.full((H, W), 0.5)

    def warp_bilinear(self, src, flow):
        self.log.append(("warp", round(float(src[0, 0, 0]), 3), round(float(flow[0, 0, 0]), 3)))
        return src.clone(), torch.ones((H, W))

    def anchor_fold(self, sources, weights, want_parts=False):
        self.log.append(("fold", [round(float(s[0, 0, 0]), 3) for s in sources], [round(float(c[0, 0]), 3) for c in weights]))
        assert want_parts and all(tuple(s.shape) == (3, H, W) for s in sources) and all(tuple(c.shape) == (H, W) for c in weights)
        return sources[0].clone(), torch.ones((H, W)), torch.ones((len(sources), H, W))

    def prepare_img(self, hwc):
        return hwc.permute(2, 0, 1)[None].contiguous()

    def bicubic_half(self, x):
        return x[:, :, ::2, ::2].contiguous()


def _fake_jobs(monkeypatch, starts, run_each=None):
    """Frame k's job yields one image of the value 10 + k; `starts` collects the start callables; run_each(start) is called
    when a job with a start begins, as the real job would call it."""
    from artstyletransfer_amd import neural_style_transfer as impl
    count = [0]

    async def fake_plain(pair, *a, **kw):
        count[0] += 1
        yield 100.0, np.full((H, W, 3), 10.0, np.float32)

    def fake_from(pair, *a, device=None, start=None, **kw):
        starts.append(start)
        k = count[0]
        count[0] += 1

        async def gen():
            if run_each is not None:
                run_each(start)
            yield 100.0, np.full((H, W, 3), 10.0 + k, np.float32)
        return gen()

    monkeypatch.setattr(impl, "neural_style_transfer", fake_plain)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)


def test_without_long_term_both_entry_points_reach_the_code_they_reached(monkeypatch):
    """long_term=None, long_term_flows=None: the start callable warps once, forms c as before and never folds."""
    from artstyletransfer_amd import video
    frames = [np.full((64, 96, 3), v, np.float32) for v in (0.1, 0.2, 0.3)]
    logs = []
    for fn, kw in ((video.neural_style_transfer_video, {}), (video.neural_style_transfer_video_long_term, dict(long_term=None, long_term_flows=None))):
        starts = []
        _fake_jobs(monkeypatch, starts)

        async def go():
            return [i async for i, _, _ in fn(frames, STYLE, temporal_weight=2.0, cfg=_cfg(), **kw)]

        assert asyncio.run(go()) == [0, 1, 2] and len(starts) == 2
        s = _Setup()
        for start in starts:
            omega, anchors, weights, gamma = start(s, (H, W))
            assert tuple(omega.shape) == (H, W, 3) and gamma == 2.0 and float(weights[0][0, 0]) == 0.5
        assert not [e for e in s.log if e[0] == "fold"]
        logs.append(s.log)
    assert logs[0] == logs[1]
    assert [e for e in logs[0] if e[0] == "estimate"] == [("estimate", 0.2, 0.1), ("estimate", 0.1, 0.2), ("estimate", 0.3, 0.2), ("estimate", 0.2, 0.3)]
    assert sorted(e[1] for e in logs[0] if e[0] == "resize") == [0.1, 0.2, 0.3]


def test_long_term_driver_estimates_every_offset_in_use_and_forms_each_plane_once(monkeypatch):
    """Six frames, long_term=(4, 2): frame i folds the offsets 1, 2, 4 that are <= i, nearest first; backward =
    estimate(plane(i), plane(i-j)), forward the other way; each plane is formed once although the driver drops the planes
    older than max(offsets) frames as it goes."""
    from artstyletransfer_amd import video
    values = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
    frames = [np.full((64, 96, 3), v, np.float32) for v in values]
    starts, s = [], _Setup()
    per_frame = []

    def run(start):
        before = len(s.log)
        omega, anchors, weights, gamma = start(s, (H, W))
        per_frame.append(s.log[before:])
        assert tuple(omega.shape) == (H, W, 3) and [tuple(c.shape) for c in weights] == [(H, W), (H // 2, W // 2)]

    _fake_jobs(monkeypatch, starts, run)

    async def go():
        return [i async for i, _, _ in video.neural_style_transfer_video_long_term(frames, STYLE, temporal_weight=2.0, cfg=_cfg(),
                                                                                  long_term=(4, 2))]

    assert asyncio.run(go()) == [0, 1, 2, 3, 4, 5] and len(starts) == 5
    used = {1: [1], 2: [1, 2], 3: [1, 2], 4: [1, 2, 4], 5: [1, 2, 4]}
    for i, log in zip(range(1, 6), per_frame):
        here = values[i]
        est = [e for e in log if e[0] == "estimate"]
        want = []
        for j in used[i]:
            want += [("estimate", here, values[i - j]), ("estimate", values[i - j], here)]
        assert est == want, (i, est)
        fold = [e for e in log if e[0] == "fold"]
        assert len(fold) == 1 and fold[0][1] == [10.0 + (i - j) for j in used[i]] and fold[0][2] == [0.5] * len(used[i])
        assert [e[1] for e in log if e[0] == "warp"] == fold[0][1]
    assert sorted(e[1] for e in s.log if e[0] == "resize") == list(values)          # every plane once: none was dropped too early


def test_long_term_driver_reads_the_callers_flows_by_offset(monkeypatch):
    """Caller flows: entry k of offset j's lists relates frame k + j to frame k; weights win over forward flows, forward
    flows over the valid plane - per offset, as for offset 1."""
    from artstyletransfer_amd import video
    frames = [np.full((64, 96, 3), 0.1 * (k + 1), np.float32) for k in range(4)]
    bwd1 = [np.full((H, W, 2), 100.0 + k, np.float32) for k in range(3)]
    bwd2 = [np.full((H, W, 2), 200.0 + k, np.float32) for k in range(2)]
    fwd2 = [np.full((H, W, 2), 300.0 + k, np.float32) for k in range(2)]
    bwd3 = [np.full((H, W, 2), 400.0, np.float32)]
    wts3 = [np.full((H, W), 0.25, np.float32)]
    starts, s = [], _Setup()
    _fake_jobs(monkeypatch, starts)

    async def go():
        return [i async for i, _, _ in video.neural_style_transfer_video_long_term(
            frames, STYLE, bwd1, temporal_weight=2.0, cfg=_cfg(), long_term=(2, 3),
            long_term_flows={3: (bwd3, _flows(1), wts3), 2: (bwd2, fwd2, None)})]

    assert asyncio.run(go()) == [0, 1, 2, 3] and len(starts) == 3
    starts[2](s, (H, W))                                                    # frame 3: offsets 1, 2, 3 -> frames 2, 1, 0
    assert [e for e in s.log if e[0] == "warp"] == [("warp", 12.0, 102.0), ("warp", 11.0, 201.0), ("warp", 10.0, 400.0)]
    assert [e for e in s.log if e[0] == "weights"] == [("weights", 301.0, 201.0)]
    assert [e for e in s.log if e[0] == "fold"] == [("fold", [12.0, 11.0, 10.0], [1.0, 0.5, 0.25])]
    assert not [e for e in s.log if e[0] == "estimate"]


def test_long_term_anchor_checks_its_lists():
    from artstyletransfer_amd import video
    with pytest.raises(ValueError, match="2 results need 2 backward flows"):
        video.long_term_anchor(_Setup(), [torch.zeros(3, H, W)] * 2, [torch.zeros(2, H, W)])
    with pytest.raises(ValueError, match="2 results need 2 backward flows"):
        video.long_term_anchor(_Setup(), [torch.zeros(3, H, W)] * 2, [torch.zeros(2, H, W)] * 2, weights=[None])


# ---- the engine call and the bindings -----------------------------------------------------------------------------------------
def test_anchor_fold_refuses_a_bad_source_count_before_the_library():
    from artstyletransfer_amd import engine
    e = object.__new__(engine.StyleEngine)
    for n in (0, 9):
        with pytest.raises(ValueError, match="1 .. 8 sources"):
            e.anchor_fold([torch.zeros(3, 4, 4)] * n, [torch.zeros(4, 4)] * n)
    with pytest.raises(ValueError, match="as many weight planes"):
        e.anchor_fold([torch.zeros(3, 4, 4)] * 2, [torch.zeros(4, 4)])


def test_long_term_bindings_match_the_header():
    from artstyletransfer_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert "#define NST_MAX_ANCHOR_SOURCES 8\n" in hdr and _lib.NST_MAX_ANCHOR_SOURCES == 8 == ref.MAX_SOURCES
    m = re.search(r"\nint nst_anchor_fold\(([^;]*)\);", hdr)
    decl = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert len(decl.split(",")) == 11 == len(_lib.SYMBOLS["nst_anchor_fold"][1])
    assert "section 4.3, eq. 9-10" in hdr
    src = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "temporal.hip" in src
