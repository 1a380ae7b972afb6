"""CPU: the Gram pass's local statistic, split rule, window plan and model (tests/gram_local.py).

Three things are shown here, without a device:
  1. coverage - the window plan on the shapes the GPU tests use (SHAPES, SLAB_SHAPES, imported there) reaches, for each tile
     shape, every mechanism of gram_h2_body and of the finish pass's slab reads: the chunk each prologue load stages and one
     staged by the in-loop load into either LDS buffer, each k-step alone, a ragged last chunk, a ragged last 8-pixel group, the
     pixel N - 1, a window across a split boundary, splits of one chunk and of odd and even chunk counts, and a window in slab 0,
     in each of the 8 lane groups, in the 64-at-a-time loop, in the 32-at-a-time tail, in the last slab of a count that is no
     multiple of 8 and in the last slab of the largest count.
     The split rule gives a lone map one chunk per split until it has more chunks than the largest split count, so the in-loop
     load is first reached at 3 x 256 chunks + 1: 98 305 pixels of 64 channels (25 MB), 24 577 of 128 channels (12.6 MB) - the
     two large shapes; every other shape is the smallest that reaches its branch.
  2. the model's healthy arithmetic stays under max(4 x torch-fp32, 5e-7) on every window of every shape (measured: 3e-8 ...
     2.4e-7 in the worst family), in the plain, the shifted and the guided form;
  3. every planted defect stands at least 4x above that bound in the family that owns it - and the k-step defect on a WHOLE map
     passes both assertions the suite had (test_gram_mfma's): the gap this closes."""
import numpy as np
import pytest
import torch

import gram_local as gl
from local_accuracy import FACTOR, FLOOR

# C, h, w - lone maps (the plan's windows) and the shapes whose slabs are visited (large split counts)
SHAPES = [(64, 3, 5), (64, 297, 334), (128, 17, 9), (128, 155, 159), (256, 50, 61), (384, 9, 11), (512, 49, 53)]
SLAB_SHAPES = [(64, 150, 230), (64, 128, 256), (128, 155, 159), (128, 64, 128), (256, 40, 68), (384, 32, 42), (512, 25, 32)]
# the shifted and the guided form: ragged in the chunk and in the 8-pixel group, more than one split
FORM_SHAPES = [(64, 23, 37), (128, 17, 9), (256, 50, 61)]

CHUNKS = {"chunk:load0", "chunk:load1", "chunk:loop_buf0", "chunk:loop_buf1"}
BODY = CHUNKS | {"kstep:0", "kstep:1", "ragged_chunk", "ragged_group", "last_pixel", "straddle", "split:one", "split:odd", "split:even"}
SLABS = {"slab:0", "slab:read64", "slab:read32", "slab:last_not_mult8", "slab:last_of_max"} | {f"slab:group{g}" for g in range(8)}


def _geo(C, h, w):
    return (C, h * w) + gl.geometry(C, h * w)


def _features(shapes, plan):
    out = {64: set(), 128: set()}
    for C, h, w in shapes:
        g = _geo(C, h, w)
        for _, p0, p1 in plan(*g):
            out[gl.gram_ts(C)] |= gl.window_features(*g, p0, p1)
    return out


# ---- 1. the split rule and the coverage of the plan ----------------------------------------------------------------------------
def test_split_rule_restated():
    # one chunk per split up to the largest count; 256 splits of whole chunks at C = 64 need 256 x 128 pixels exactly
    assert gl.geometry(64, 32768) == (256, 128) and gl.geometry(128, 8192) == (256, 32)
    assert gl.geometry(64, 15) == (1, 128) and gl.geometry(512, 15) == (1, 32)
    assert [gl.gram_max_splits(c) for c in (64, 128, 256, 384, 512, 1024)] == [256, 256, 85, 42, 25, 7]      # 256 / pairs (the 32 MiB cap - 8 slabs at C = 1024 - is never the smaller one here)
    assert gl.geometry(64, 99198) == (194, 512) and gl.geometry(128, 24645) == (193, 128) and gl.geometry(512, 2597) == (21, 128)
    for C in (64, 128, 256, 384, 512):
        for N in (1, 7, 31, 32, 33, 127, 128, 129, 1000, 4097, 33123, 99198):
            ns, pps = gl.geometry(C, N)
            assert pps % gl.gram_kp(C) == 0 and (ns - 1) * pps < N <= ns * pps and ns <= gl.gram_max_splits(C), (C, N, ns, pps)
    # in a batch the largest map of a channel count keeps its split count, a smaller one gets the same pixels per workgroup
    items = [(128, 24645), (128, 6132), (128, 1520), (64, 99198), (64, 24600)]
    got = [gl.geometry(*it, items, i) for i, it in enumerate(items)]
    assert got[0] == gl.geometry(128, 24645) and got[3] == gl.geometry(64, 99198)
    assert got[1] == (48, 128) and got[2] == (12, 128) and got[4] == (49, 512)
    for i, (C, N) in enumerate(items):
        assert got[i][0] <= gl.gram_nsplit(C, N) and (got[i][0] - 1) * got[i][1] < N <= got[i][0] * got[i][1]
    assert gl.geometry(128, 6132)[0] == 192          # (alone it would take 192 splits of one chunk)


def test_the_plan_reaches_every_mechanism_for_each_tile_shape():
    body, slabs = _features(SHAPES, gl.window_plan), _features(SLAB_SHAPES, gl.slab_plan)
    for ts in (64, 128):
        assert BODY <= body[ts], (ts, sorted(BODY - body[ts]))
        assert SLABS <= slabs[ts], (ts, sorted(SLABS - slabs[ts]))
    # one, two, three and four tiles per side, and the 64-wide shape
    assert {C for C, _, _ in SHAPES} == {64, 128, 256, 384, 512} == {C for C, _, _ in SLAB_SHAPES}
    # the 64-at-a-time loop needs 58 slabs at least; the largest count of every channel count is there
    assert all(max(gl.geometry(C, h * w)[0] for C, h, w in SLAB_SHAPES if gl.gram_ts(C) == ts) >= 58 for ts in (64, 128))
    for C in (64, 128, 256, 384, 512):
        assert any(gl.geometry(c, h * w)[0] == gl.gram_max_splits(C) for c, h, w in SLAB_SHAPES if c == C), C
    # every chunk window is a whole chunk and every k-step window 16 pixels (or what the map has)
    for C, h, w in SHAPES:
        g = _geo(C, h, w)
        for name, p0, p1 in gl.window_plan(*g):
            if ".chunk" in name:
                assert p1 - p0 == min(gl.gram_kp(C), h * w - p0) and gl.window_features(*g, p0, p1) & CHUNKS, (C, name)
            if ".kstep" in name:
                assert p1 - p0 <= 16 and gl.window_features(*g, p0, p1) & {"kstep:0", "kstep:1"}, (C, name)


def test_read64_is_the_loop_condition_of_the_finish_pass():
    for nslabs in (1, 7, 8, 56, 57, 58, 64, 65, 85, 135, 193, 256):
        seen = {}
        for grp in range(8):                                   # gram_finish_body's two loops, as written
            k = grp
            while k + 56 < nslabs:
                seen.update({k + 8 * q: True for q in range(8)})
                k += 64
            while k < nslabs:
                seen.update({k + 8 * q: False for q in range(4) if k + 8 * q < nslabs})
                k += 32
        assert sorted(seen) == list(range(nslabs))
        assert all(gl.read64(k, nslabs) == v for k, v in seen.items()), nslabs


# ---- the statistic itself ------------------------------------------------------------------------------------------------------
def test_exact_values_on_a_hand_made_error_pattern():
    C = 256
    ref = np.full((C, C), 2.0)
    got = ref.copy()
    got[40, 200] += 4.0                                        # block (1, 6), tile (0, 1), row 40
    got[130, :] += 0.5                                         # row 130
    s = gl.gram_stats(got, ref)
    assert s["rows"] == (pytest.approx(0.25), 130)
    assert s["blocks"] == (pytest.approx(np.sqrt(16.0 / 1024) / 2.0), (1, 6))
    assert s["tiles"] == (pytest.approx(np.sqrt(0.25 * 128 / 16384) / 2.0), (1, 0))      # (half of row 130 outweighs the one entry)
    assert gl.gram_errors(got, ref)["tiles"][0, 1] == pytest.approx(np.sqrt(16.0 / 16384) / 2.0)
    assert s["matrix"][0] == pytest.approx(np.sqrt((16.0 + 0.25 * C) / (C * C)) / 2.0)
    assert gl.gram_stats(got, ref, scale=4.0)["rows"][0] == pytest.approx(0.125)
    e = gl.gram_errors(got, ref)
    assert e["blocks"].shape == (8, 8) and e["tiles"].shape == (2, 2) and e["rows"].shape == (C,)
    assert gl.gram_errors(got[:64, :64], ref[:64, :64])["tiles"].shape == (1, 1)
    ref32 = ref + 1e-7
    with pytest.raises(AssertionError) as exc:
        gl.assert_gram_locally_as_accurate(got, ref, ref32, "hand-made")
    assert "blocks" in str(exc.value) and "rows" in str(exc.value)
    gl.assert_gram_locally_as_accurate(ref + 3e-7, ref, ref32, "hand-made, 3x", floor=0.0)
    with pytest.raises(AssertionError):
        gl.assert_gram_locally_as_accurate(ref + 5e-7, ref, ref32, "hand-made, 5x", floor=0.0)
    gl.assert_gram_locally_as_accurate(ref + 9e-7, ref, ref, "hand-made, under the floor")
    with pytest.raises(AssertionError):
        gl.assert_gram_locally_as_accurate(ref + 1.1e-6, ref, ref, "hand-made, over the floor")
    with pytest.raises(AssertionError):
        gl.assert_gram_locally_as_accurate(ref, ref, ref32, "a factor above the cap", factor=17.0)


# ---- 2. the healthy model --------------------------------------------------------------------------------------------------------
def _setup(C, h, w):
    F = gl.pixel_major(gl.feature_map(C, h, w))
    return F, F.numpy(), float(C * h * w)


def _hold(failures, *args, **kw):
    try:
        return gl.assert_gram_locally_as_accurate(*args, **kw)
    except AssertionError as err:
        failures.append(str(err))


def _soft_plane(h, w):
    t = np.full((h, w), 0.7, np.float32)
    t[:, : w // 2] = 0.9
    return t.reshape(-1)


@pytest.mark.parametrize("C,h,w", SHAPES + [s for s in SLAB_SHAPES if s not in SHAPES], ids=lambda v: str(v))
def test_healthy_model_stays_under_the_bound_on_every_window(C, h, w):
    """Measured, worst family: 3e-8 (one pixel) ... 2.4e-7 (whole maps) - under the floor on every window; torch-fp32 itself
    1e-8 ... 1.9e-7."""
    F, Fn, div = _setup(C, h, w)
    g = _geo(C, h, w)
    wins = [("whole map", 0, h * w)] if (C, h, w) in SHAPES else []
    wins += gl.window_plan(*g) if (C, h, w) in SHAPES else []
    wins += gl.slab_plan(*g) if (C, h, w) in SLAB_SHAPES else []
    failures = []
    for name, p0, p1 in wins:
        ref64, ref32 = gl.window_truths(F, p0, p1, div)
        got = gl.model_gram(Fn, g[2], g[3], div, window=(p0, p1))
        assert np.array_equal(got, got.T)
        _hold(failures, got, ref64, ref32, f"model C={C} {h}x{w} plain [{p0},{p1}) {name}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("C,h,w", FORM_SHAPES, ids=lambda v: str(v))
def test_healthy_model_of_the_shifted_and_guided_forms(C, h, w):
    F, Fn, div = _setup(C, h, w)
    N = h * w
    g = _geo(C, h, w)
    assert N % gl.gram_kp(C) and N % 8 and g[2] > 1
    wins = [("whole map", 0, N)] + [x for x in gl.window_plan(*g) if x[0].startswith(("ragged", "last"))]
    failures = []
    for name, p0, p1 in wins:
        Fw = Fn[p0:p1]
        for what, o in (("shift -1", np.full(C, -1.0, np.float32)), ("centred", (-Fw.astype(np.float64).sum(axis=0) / N).astype(np.float32))):
            ref64, ref32 = gl.window_truths(F, p0, p1, div, o=torch.from_numpy(o))
            amax = float(np.abs(Fw).max() + np.abs(o).max())
            got = gl.model_gram(Fn, g[2], g[3], div, window=(p0, p1), o=o, absmax=amax)
            _hold(failures, got, ref64, ref32, f"model C={C} {h}x{w} {what} [{p0},{p1}) {name}")
    soft = _soft_plane(h, w)
    ref64, ref32 = gl.window_truths(F, 0, N, div, t=torch.from_numpy(soft))
    _hold(failures, gl.model_gram(Fn, g[2], g[3], div, t=soft), ref64, ref32, f"model C={C} {h}x{w} guided 0.9/0.7")
    for name, p0, p1 in gl.window_plan(*g):
        t = np.zeros(N, np.float32)
        t[p0:p1] = 1.0
        ref64, ref32 = gl.window_truths(F, p0, p1, div)           # (t = 1 on the window, 0 elsewhere: the window's Gram)
        got = gl.model_gram(Fn, g[2], g[3], div, t=t)              # ... with the absmax of the WHOLE map
        _hold(failures, got, ref64, ref32, f"model C={C} {h}x{w} guided window plane [{p0},{p1}) {name}")
    assert not failures, "\n".join(failures)


# ---- 3. planted defects ----------------------------------------------------------------------------------------------------------
DEFECT_SHAPES = [(64, 150, 230), (128, 155, 159), (256, 50, 61), (512, 49, 53)]


def _over(got, ref64, ref32, family):
    """the statistic of `family` as a multiple of its bound"""
    d, t = gl.gram_stats(got, ref64)[family][0], gl.gram_stats(ref32, ref64)[family][0]
    return d / max(FACTOR * t, FLOOR)


@pytest.mark.parametrize("C,h,w", DEFECT_SHAPES, ids=lambda v: str(v))
def test_defects_of_one_chunk_stand_4x_above_the_bound_in_their_block(C, h, w):
    """Measured: both cross products of one k-step lost 30x ... 900x the bound on windows of 16 ... 128 pixels; lo x hi of one
    chunk lost 20x ... 600x; a wrong fragment pair 1e5x and more."""
    F, Fn, div = _setup(C, h, w)
    g = _geo(C, h, w)
    nb, kp = C // 32, gl.gram_kp(C)
    worst = {}
    for name, p0, p1 in gl.window_plan(*g):
        feats = gl.window_features(*g, p0, p1)
        if not feats & CHUNKS:
            continue
        ref64, ref32 = gl.window_truths(F, p0, p1, div)
        sp, off = p0 // g[3], p0 % g[3]
        for rb, cb in {(0, 1), (0, nb - 1), (nb - 1, nb - 1)}:
            cases = {"kstep_cross": ("kstep_cross", sp, off - off % 16, rb, cb), "wrong_fragment": ("wrong_fragment", sp, rb, cb, cb - 1)}
            if p1 - p0 == kp:
                cases["one_cross"] = ("one_cross", sp, off // kp, rb, cb)
            for kind, defect in cases.items():
                got = gl.model_gram(Fn, g[2], g[3], div, window=(p0, p1), defect=defect)
                over = _over(got, ref64, ref32, "blocks")
                assert gl.gram_stats(got, ref64)["blocks"][1] in ((rb, cb), (cb, rb)), (kind, name, rb, cb)      # (mirrored)
                worst[kind] = min(worst.get(kind, np.inf), over)
                assert over >= 4.0, (kind, name, (rb, cb), over)
    gl.report(f"model C={C} {h}x{w}: planted defects, least multiple of the bound (blocks): "
              + ", ".join(f"{k} {v:.0f}x" for k, v in sorted(worst.items())))
    assert set(worst) == {"kstep_cross", "one_cross", "wrong_fragment"}


@pytest.mark.parametrize("C,h,w", FORM_SHAPES, ids=lambda v: str(v))
def test_defects_of_the_finish_the_shift_and_the_guide_stand_4x_above_the_bound(C, h, w):
    F, Fn, div = _setup(C, h, w)
    N = h * w
    g = _geo(C, h, w)
    out = {}
    # a slab left out: the whole map, and a window across a split boundary
    edge = g[3]
    for name, p0, p1, slab in (("whole map", 0, N, g[2] - 1), ("across a boundary", edge - 8, edge + 8, 1)):
        ref64, ref32 = gl.window_truths(F, p0, p1, div)
        out[f"no_slab, {name}"] = _over(gl.model_gram(Fn, g[2], g[3], div, window=(p0, p1), defect=("no_slab", slab)), ref64, ref32, "matrix")
    # the shifted form: the staged pixels behind p1 contribute o o^T
    o = np.full(C, -1.0, np.float32)
    for name, p0, p1 in (("whole map", 0, N), ("ragged last group", N - N % 8, N)):
        ref64, ref32 = gl.window_truths(F, p0, p1, div, o=torch.from_numpy(o))
        got = gl.model_gram(Fn, g[2], g[3], div, window=(p0, p1), o=o, absmax=float(np.abs(Fn[p0:p1]).max() + 1.0), defect=("tail_offsets",))
        out[f"tail_offsets, {name}"] = _over(got, ref64, ref32, "matrix")
    # the guided form: t read one pixel late
    soft = _soft_plane(h, w)
    ref64, ref32 = gl.window_truths(F, 0, N, div, t=torch.from_numpy(soft))
    out["guide_off_by_one, 0.9/0.7"] = _over(gl.model_gram(Fn, g[2], g[3], div, t=soft, defect=("guide_off_by_one",)), ref64, ref32, "matrix")
    t = np.zeros(N, np.float32)
    t[N - N % 8:] = 1.0
    ref64, ref32 = gl.window_truths(F, N - N % 8, N, div)
    out["guide_off_by_one, window plane"] = _over(gl.model_gram(Fn, g[2], g[3], div, t=t, defect=("guide_off_by_one",)), ref64, ref32, "matrix")
    gl.report(f"model C={C} {h}x{w}: planted defects, multiple of the bound (matrix): " + ", ".join(f"{k} {v:.0f}x" for k, v in out.items()))
    assert all(v >= 4.0 for v in out.values()), out


def test_the_kstep_defect_on_a_whole_map_passes_the_assertions_the_suite_had():
    """The gap: both cross products of one k-step lost in one block, on the whole 64 x 128 x 192 map of test_gram_mfma - under
    rel-L2 < 2e-6 and rtol 1e-4 / atol 1e-6 max|G|, and within 4x of torch-fp32 even per block.  On the k-step's own window the
    same defect is far outside (the test above)."""
    C, h, w = 64, 128, 192
    F, Fn, div = _setup(C, h, w)
    g = _geo(C, h, w)
    ref64, ref32 = gl.window_truths(F, 0, h * w, div)
    got = gl.model_gram(Fn, g[2], g[3], div, defect=("kstep_cross", 1, 16, 0, 1))
    assert np.linalg.norm(got - ref64) / np.linalg.norm(ref64) < 2e-6
    np.testing.assert_allclose(got, ref64, rtol=1e-4, atol=1e-6 * np.abs(ref64).max())
    assert _over(got, ref64, ref32, "blocks") < 1.0
