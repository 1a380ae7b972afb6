"""GPU: what a long-lived context computes for a job must be THE BITS a fresh context computes for it, whatever ran before.

The library is a serving library: one nst_ctx runs job after job.  A context carries ten job-level settings with three different
life cycles across nst_job_configure, absmax records that five different places zero, stored ReLU / pooling decisions, the record
of maps nobody stored, the forward-half token, a captured hipGraph, the optimiser's served-closure cache - and device memory that
hipMalloc hands back with the previous job's bytes in it.  The closure is bitwise reproducible from run to run and from engine to
engine, so no oracle and no tolerance is needed: a record, mask, offset, target or workspace left over from an earlier job shows
as a different bit.

  part 0 (CPU)  the station list and the visiting orders hold what they exist for (test_plan_*).
  part 1        per engine variant: every station on a fresh engine (FRESH), then ONE engine visits the stations in four orders,
                with the things a serving process does in between (DISTURBANCES), and every kept quantity is compared bitwise.
  part 2        one call between nst_closure_forward and nst_closure_backward, and between two L-BFGS steps: either the bits of
                the undisturbed run, or NST_E_STATE with nothing written - which of the two is taken from include/nst_hip.h.
  part 3        two contexts on one device, interleaved.

A mismatch is reported as (order, position, station, predecessor, first differing quantity)."""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

from hip_helpers import CW, SW, TVW, dev, levels, report

SENTINEL = -12345.0
TAP_LAYER = (0, 2, 4, 8, 9, 12)              # conv layer of the six maps of Vgg19.layer_names
W_ONE = (1.0, 0.5, 2.0, 0.25, 1.0, 0.0)      # style layer weights: every tap set of the stations keeps a positive map under either
W_TWO = (0.0, 1.5, 0.75, 3.0, 1.0, 0.5)
# moment loss (set_moments): (weights of the mean terms, of the deviation terms) by map index; a map with both, with one, with neither
M_ONE = ((1e3, 0.0, 5e2, 1e3, 0.0, 2e3), (1e3, 7e2, 0.0, 1e3, 0.0, 2e3))
M_TWO = ((0.0, 8e2, 1e3, 0.0, 0.0, 5e2), (2e3, 0.0, 1e3, 6e2, 0.0, 0.0))
M_TAPS = ((0.0, 5e2, 0.0, 1e3, 0.0, 2e3), (0.0, 7e2, 0.0, 0.0, 0.0, 2e3))      # on the style maps of taps (1, 3, 5) only

Station = collections.namedtuple(
    "Station", "name h w nlev hs ws seed amp taps color pooling style_weights laplacian matting gram_shift guidance blend eval moments",
    defaults=(0, None, "rgb", "max", None, None, None, None, None, None, ("closure",), None))

# guidance: (split direction, region weights); blend: the `blend` argument of set_targets_blend for K = 2
STATIONS = (
    Station("plain3", 68, 260, 3, 80, 120, 1),
    Station("plain3_hi", 68, 260, 3, 80, 120, 1, amp=4),
    Station("plain3_lo", 68, 260, 3, 80, 120, 1, amp=-10),
    Station("lum_lap_mat", 64, 96, 2, 56, 88, 5, color="luminance", laplacian=((1, 2), (3.0, 40.0)), matting=(2.8e8, 1e-7),
            eval=("halves",)),
    Station("lum_avg_mat", 64, 96, 2, 56, 88, 5, color="luminance", pooling="avg", matting=(1.4e8, 1e-5), eval=("halves",)),
    Station("avg_guided", 124, 252, 2, 100, 180, 3, pooling="avg", style_weights=W_ONE, guidance=("columns", None)),
    Station("shift_blend", 124, 252, 2, 100, 180, 3, gram_shift=(0.0, "mean", -1.0, "mean", 0.0, 0.5), blend=(0.25, 0.75)),
    Station("shift_taps", 64, 96, 2, 56, 88, 7, taps=(2, (2, 3), True), style_weights=W_TWO,
            gram_shift=(0.0, 0.0, 0.75, "mean", 0.0, 0.0)),
    Station("six_norelu", 68, 260, 3, 80, 120, 1, taps=(4, (0, 1, 2, 3, 4, 5), False), eval=("levels", 0b101)),
    Station("stripes", 124, 252, 1, 100, 180, 3, eval=("window",)),
    Station("small_lap_blend", 50, 76, 1, 40, 60, 11, pooling="avg", laplacian=((2, 1), (25.0, 2.0)),
            blend=((1.0, 0.0, 0.5, 2.0, 1.0, 0.25), (0.5, 1.0, 0.5, 0.0, 1.0, 0.75))),
    Station("lbfgs", 64, 96, 2, 56, 88, 1, eval=("lbfgs",)),
    Station("guided_rgb", 64, 96, 2, 56, 88, 1, guidance=("rows", (1.0, 0.5))),
    Station("rgb_lap_mat", 64, 96, 2, 56, 88, 1, laplacian=((1, 2), (5.0, 60.0)), matting=(2.8e8, 1e-7)),
    Station("weights_level0", 64, 96, 2, 56, 88, 1, style_weights=W_ONE, eval=("levels", 0b01)),
    Station("adam_lum", 50, 76, 1, 40, 60, 11, color="luminance", eval=("adam",)),
    # the moment loss: alone; under a centred Gram shift, a blend, unequal style weights and average pooling; under luminance with
    # the two pixel-space terms; on non-default taps whose deepest map is taken before its ReLU
    Station("moments3", 68, 260, 3, 80, 120, 1, moments=M_ONE),
    Station("mom_shift_blend_avg", 124, 252, 2, 100, 180, 3, pooling="avg", style_weights=W_TWO,
            gram_shift=(0.5, "mean", 0.0, "mean", 0.0, -0.25), blend=(0.25, 0.75), moments=M_TWO),
    Station("mom_lum_lap_mat", 64, 96, 2, 56, 88, 5, color="luminance", laplacian=((1, 2), (3.0, 40.0)), matting=(2.8e8, 1e-7),
            moments=M_ONE),
    Station("mom_taps_norelu", 64, 96, 2, 56, 88, 7, taps=(4, (1, 3, 5), False), moments=M_TAPS),
)
BY_NAME = {s.name: s for s in STATIONS}
AMPLITUDE = ("plain3", "plain3_hi", "plain3_lo")
SETTERS = ("taps", "color", "pooling", "style_weights", "laplacian", "matting", "gram_shift", "guidance", "blend", "moments")
EVAL_KINDS = ("closure", "levels", "halves", "window", "adam", "lbfgs")

VARIANTS = collections.OrderedDict((
    ("default", dict()),
    ("per_level", dict(batched=False)),
    ("graph", dict(use_graph=True)),
    ("direct", dict(h2_winograd=False)),
    ("f32_per_level", dict(conv_mode="f32", batched=False)),
))


def is_set(st, setter):
    v = getattr(st, setter)
    return v is not None and v not in ("rgb", "max")


def kept(variant):
    """The stations of an engine variant.  Left out: the halves where nst_closure_forward is unavailable (the per-level schedule -
    test_forward_half_is_unavailable_off_the_batched_schedule - and use_graph, include/nst_hip.h), and outside the f16x2 arithmetic
    the shifted Gram, the moment loss, spatial control and the stripe closure, which all return NST_E_STATE there."""
    opts = VARIANTS[variant]
    no_halves = opts.get("batched") is False or opts.get("use_graph")
    f16x2 = opts.get("conv_mode") is None
    return tuple(s.name for s in STATIONS
                 if not (no_halves and s.eval[0] == "halves")
                 and (f16x2 or not (s.gram_shift or s.moments or s.guidance or s.eval[0] == "window")))


# (the moment stations: after and before the plain job of their geometry, a guided job, a shifted one, and each other)
_ORDER_A = ("rgb_lap_mat", "plain3_hi", "plain3_lo", "plain3", "moments3", "adam_lum", "avg_guided", "mom_taps_norelu", "small_lap_blend",
            "shift_blend", "mom_shift_blend_avg", "lum_lap_mat", "shift_taps", "stripes", "lum_avg_mat", "mom_lum_lap_mat", "six_norelu",
            "lbfgs", "guided_rgb", "weights_level0")
_ORDER_B = ("lbfgs", "mom_lum_lap_mat", "plain3_lo", "plain3_hi", "adam_lum", "six_norelu", "moments3", "small_lap_blend", "plain3",
            "weights_level0", "shift_blend", "guided_rgb", "mom_shift_blend_avg", "mom_taps_norelu", "avg_guided", "lum_lap_mat",
            "stripes", "shift_taps", "lum_avg_mat", "rgb_lap_mat")
ORDERS = collections.OrderedDict((
    ("a", _ORDER_A),
    ("b", _ORDER_B),
    ("twice", tuple(n for s in STATIONS for n in (s.name, s.name))),
    # one job kept while its image changes: the walker enters a station whose job is its predecessor's WITHOUT nst_job_configure
    # (which allocates zeroed absmax records) and sets the targets again at the odd positions only - see same_job()
    ("sweep", ("plain3_hi", "plain3_lo", "plain3", "plain3_lo", "plain3_hi")),
))


def same_job(a, b):
    """Two stations that differ in the start image alone: a caller with a new image for the job it has configured applies nothing."""
    return a._replace(name="", amp=0) == b._replace(name="", amp=0)


def order_of(variant, order):
    keep = set(kept(variant))
    return tuple(n for n in ORDERS[order] if n in keep)


# ---- the disturbances: name -> contract between the halves, 'a' = the backward half is still valid, 'b' = it is refused ------------
# From include/nst_hip.h: the standalone pieces are functions of caller buffers (their scratch is their own) and a refused
# nst_closure_backward "launches nothing ... the context stays usable": (a).  nst_closure*, nst_level_activation and nst_job_* calls,
# "not even a failed one", end the validity, and the backward half belongs to the LAST forward: (b).  The read-backs the header
# was silent about write no level buffer: (a), and the header and INTEGRATION.md now say so.
DISTURBANCES = collections.OrderedDict((
    ("vgg_features", "a"), ("vgg_activations", "a"), ("vgg_features_backward", "a"), ("gram64", "a"), ("gram256", "a"),
    ("gram_shifted64", "a"), ("gram_shifted256", "a"), ("guided_gram_backward", "a"), ("total_variation", "a"),
    ("laplacian_loss", "a"), ("matting_loss", "a"), ("bicubic_half", "a"), ("bicubic_half_backward", "a"), ("resize", "a"),
    ("color_stats", "a"), ("color_affine", "a"), ("luminance", "a"), ("adam_step", "a"), ("lbfgs_direction", "a"),
    ("refused_backward", "a"), ("moments", "a"),
    ("abandoned_forward", "b"), ("refused_configure", "b"), ("refused_gram_shift", "b"), ("timed_closure", "b"),
    ("level_activations0", "b"), ("refused_moments", "b"),
))
# between the halves only: read-backs of the job
READ_BACKS = collections.OrderedDict((
    ("level_image", "a"), ("laplacian_losses", "a"), ("matting_losses", "a"), ("level_gram_offsets", "a"), ("guidance_planes", "a"),
    ("moment_losses", "a"), ("closure_schedule", "a"),
    ("level_activation", "b"),
))
PICKS = 3


def picks(order_index, position):
    """The disturbances before the station at `position` >= 1 of order number `order_index`: a fixed rule."""
    names = tuple(DISTURBANCES)
    return tuple(names[(7 * order_index + 3 * position + 11 * j) % len(names)] for j in range(PICKS))


# ---- part 0: the plan (CPU) ---------------------------------------------------------------------------------------------------------
def test_plan_stations_hold_every_setter_combination_and_evaluation():
    """CPU: the conditions the station list exists for - edits cannot thin it silently.  Geometry: every top level at or below
    ~35k pixels, coarsest level and coarsest style at least 16x16, a style of another size than the content, and the suite's
    edge-tile geometries 68x260 L3 and 124x252 L2 (test_hip_tile_shapes.GEOMETRIES) with other style sizes, 64x96 L2 and 50x76 L1;
    one-level jobs below 256x256 (the per-level walker on every engine) beside multi-level ones (the batched walker).  Every
    setter on at least two stations and off on others; with two different arguments where it has more than one (colour and
    pooling have one value besides the default: they are reached twice).  set_taps with use_relu=False and with six style maps;
    two Laplacian entries with pools 1 and 2; a shifted and a centred map in every Gram shift; R = 2; K = 2.  The combinations the
    code branches on; the three amplitudes of one job, 14 binades apart; every evaluation kind."""
    from test_hip_tile_shapes import GEOMETRIES
    assert len(STATIONS) >= 12 and len(BY_NAME) == len(STATIONS)
    geos = {(s.h, s.w, s.nlev) for s in STATIONS}
    assert {(68, 260, 3), (124, 252, 2), (64, 96, 2), (50, 76, 1)} <= geos
    known = {g[:3]: g[3:] for g in GEOMETRIES}
    for s in STATIONS:
        assert s.h * s.w <= 35_000, s.name
        assert min(s.h >> (s.nlev - 1), s.w >> (s.nlev - 1), s.hs >> (s.nlev - 1), s.ws >> (s.nlev - 1)) >= 16, s.name
        assert (s.hs, s.ws) != (s.h, s.w) and (s.hs, s.ws) != known.get((s.h, s.w, s.nlev)), s.name
        assert s.eval[0] in EVAL_KINDS
    assert any(s.nlev == 1 and s.h * s.w < 256 * 256 for s in STATIONS) and any(s.nlev > 1 for s in STATIONS)
    for setter in SETTERS:
        on = [getattr(s, setter) for s in STATIONS if is_set(s, setter)]
        assert len(on) >= 2 and len(on) < len(STATIONS), setter
        if setter not in ("color", "pooling"):
            assert len(set(on)) >= 2, setter
    taps = [s.taps for s in STATIONS if s.taps]
    assert any(t[2] is False for t in taps) and any(len(t[1]) == 6 for t in taps)
    assert all(sorted(s.laplacian[0]) == [1, 2] for s in STATIONS if s.laplacian)
    for s in STATIONS:
        if s.gram_shift:
            live = [s.gram_shift[i] for i in (s.taps[1] if s.taps else (0, 1, 2, 3, 5))]
            assert "mean" in live and any(isinstance(v, float) and v != 0.0 for v in live), s.name
            assert not s.guidance                                          # (the kernels exclude offset with guide)
        if s.blend:
            assert len(s.blend) == 2
        if s.style_weights:                                                # a caller may set them under any station's taps
            assert all(any(s.style_weights[i] > 0 for i in (t.taps[1] if t.taps else (0, 1, 2, 3, 5))) for t in STATIONS)
    assert any(s.color == "luminance" and s.laplacian and s.matting for s in STATIONS)
    assert any(s.pooling == "avg" and s.guidance for s in STATIONS)
    assert any(s.gram_shift and s.blend for s in STATIONS)
    assert any(s.gram_shift and not s.blend and not s.guidance for s in STATIONS)
    for s in STATIONS:
        if s.moments:                                                      # only on style maps of the station's taps, never guided
            live = s.taps[1] if s.taps else (0, 1, 2, 3, 5)
            assert all(i in live for wts in s.moments[:2] for i, v in enumerate(wts) if v > 0) and not s.guidance, s.name
            assert any(v > 0 for v in s.moments[0]) and any(v > 0 for v in s.moments[1]), s.name
    mom = [s for s in STATIONS if s.moments]
    assert any(not any(is_set(s, k) for k in SETTERS if k != "moments") and (s.h, s.w, s.nlev) == (68, 260, 3) for s in mom)
    assert any(s.gram_shift and "mean" in s.gram_shift and s.blend and s.style_weights and s.pooling == "avg"
               and (s.h, s.w, s.nlev) == (124, 252, 2) for s in mom)
    assert any(s.color == "luminance" and s.laplacian and s.matting and (s.h, s.w, s.nlev) == (64, 96, 2) for s in mom)
    assert any(s.taps and s.taps[2] is False and 5 in s.taps[1] and s.moments[0][5] > 0 for s in mom)
    base = BY_NAME["plain3"]
    assert [BY_NAME[n].amp for n in AMPLITUDE] == [0, 4, -10]
    assert all(BY_NAME[n]._replace(name="", amp=0) == base._replace(name="") for n in AMPLITUDE)
    assert {s.eval[0] for s in STATIONS} == set(EVAL_KINDS)
    for s in STATIONS:
        if s.eval[0] == "levels":                                          # partial, and with level 0 (level_activations(0) follows)
            assert 0 < s.eval[1] < (1 << s.nlev) - 1 and s.eval[1] & 1, s.name
        if s.eval[0] == "window":                                          # what nst_window_* implements
            assert s.nlev == 1 and not any(is_set(s, k) for k in SETTERS)


def test_plan_orders_give_every_station_two_predecessors_and_every_setter_both_pasts():
    """CPU: per engine variant at least eight stations (what is left out and why: kept()), two fixed permutations plus every
    station twice in a row; over the orders every station has at least two different predecessors, every setter is met both after
    a station that had it set and after one that had not, the amplitude stations follow each other in both directions, a
    permutation grows, shrinks and grows again in consecutive steps, and the fixed rule reaches every disturbance.  The settings
    read back from the context (nst_job_* getters) are a kept quantity and are compared BEFORE a station is evaluated: a stale
    setting whose buffers went with the previous job is then a failed comparison on the host, not a launch.
    The order "sweep" was added when dropping the absmax zeroing of the per-level front of batched_forward passed every other
    order: nst_job_configure hands every station freshly zeroed records, so the records of one image can reach the next only
    where a job is kept - the three amplitude stations there follow each other on ONE configured job, 14 binades apart in
    both directions, with the targets set again in between (a target forward runs that front on every engine variant)."""
    sweep = [BY_NAME[n] for n in ORDERS["sweep"]]
    steps = [b.amp - a.amp for a, b in zip(sweep, sweep[1:])]
    assert all(same_job(a, b) for a, b in zip(sweep, sweep[1:])) and min(steps) <= -14 and max(steps) >= 14
    assert steps[0] <= -14                     # (position 1 sets the targets again: their forward pass right after the brightest image)
    assert len(ORDERS) >= 3 and set(ORDERS["a"]) == set(ORDERS["b"]) == set(BY_NAME) and ORDERS["a"] != ORDERS["b"]
    assert len(ORDERS["a"]) == len(STATIONS) and len(ORDERS["twice"]) == 2 * len(STATIONS)
    assert kept("default") == kept("direct") == tuple(BY_NAME)
    for variant in VARIANTS:
        names = kept(variant)
        assert len(names) >= 8, variant
        assert set(AMPLITUDE) <= set(names) and {BY_NAME[n].eval[0] for n in names} >= {"closure", "levels", "adam", "lbfgs"}
        pred = collections.defaultdict(set)
        pairs = set()
        used = set()
        for oi, order in enumerate(ORDERS):
            seq = order_of(variant, order)
            for p, (a, b) in enumerate(zip(seq, seq[1:]), start=1):
                pred[b].add(a)
                pairs.add((a, b))
                used.update(picks(oi, p))
        assert all(len(pred[n]) >= 2 for n in names), (variant, {n: pred[n] for n in names if len(pred[n]) < 2})
        for setter in SETTERS:
            if not any(is_set(BY_NAME[n], setter) for n in names):
                assert variant == "f32_per_level" and setter in ("gram_shift", "guidance", "moments")
                continue
            pasts = {(is_set(BY_NAME[a], setter), is_set(BY_NAME[b], setter)) for a, b in pairs}
            assert {(True, True), (False, True), (True, False)} <= pasts, (variant, setter)
        assert ("plain3_hi", "plain3_lo") in pairs and ("plain3_lo", "plain3_hi") in pairs
        grows = False
        for order in ("a", "b"):
            px = [BY_NAME[n].h * BY_NAME[n].w * ((4 ** BY_NAME[n].nlev - 1) / 3) for n in order_of(variant, order)]
            grows = grows or any(px[i + 1] > px[i] and px[i + 2] < px[i + 1] and px[i + 3] > px[i + 2] for i in range(len(px) - 3))
        assert grows, variant
        assert used == set(DISTURBANCES), (variant, set(DISTURBANCES) - used)
    assert set(DISTURBANCES.values()) == set(READ_BACKS.values()) == {"a", "b"}


# ---- jobs ---------------------------------------------------------------------------------------------------------------------------
_JOBS = {}        # station name -> device tensors of the job, made once and never written
_FOREIGN = {}     # inputs of the standalone calls
_FRESH = {}       # variant -> {station name: kept result}
_FIRST = {}       # (variant, disturbance, job settings it depends on) -> bits of its first results
_COUNTS = collections.Counter()


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().contiguous().cpu().numpy()
    a = np.ascontiguousarray(t)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).copy()


def _planes(kind, h, w):
    """R = 2, soft (0.9 on the own half, 0.7 on the other): each region keeps one pixel's worth of mass on the smallest map."""
    own = np.full((h, w), 0.7, dtype=np.float32)
    if kind == "columns":
        own[:, : w // 2] = 0.9
    else:
        own[: h // 2, :] = 0.9
    return dev(torch.from_numpy(np.stack([own, 1.6 - own]).astype(np.float32)))


def _job(st):
    if st.name in _JOBS:
        return _JOBS[st.name]
    from oracle import cpu_ref
    from artstyletransfer_amd import host_image
    c, s = levels(st.h, st.w, st.nlev, st.seed), levels(st.hs, st.ws, st.nlev, st.seed + 1)
    s2 = levels(st.hs - 8, st.ws + 12, st.nlev, st.seed + 2) if st.blend else None
    start = (0.6 * c[0] + 0.4 * cpu_ref.synthetic_image(st.h, st.w, seed=9)).astype(np.float32)
    if st.color == "luminance":
        alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
        prep_c = lambda a: dev(torch.from_numpy(host_image.luminance(a)))                      # noqa: E731
        prep_s = lambda a: dev(torch.from_numpy(host_image.luminance(a, alpha, beta)))         # noqa: E731
        x = torch.from_numpy(host_image.luminance(start)).reshape(1, 1, st.h, st.w)
    else:
        prep_c = prep_s = lambda a: dev(cpu_ref.prepare_img(a))                                 # noqa: E731
        x = cpu_ref.prepare_img(start)
    job = {"content": [prep_c(a) for a in c], "style": [prep_s(a) for a in s],
           "style2": [prep_s(a) for a in s2] if s2 else None,
           "x": dev((x * float(2.0 ** st.amp)).contiguous())}                                   # (a power of two: exact, finite)
    if st.guidance:
        job["planes"] = [_planes(st.guidance[0], st.h >> l, st.w >> l) for l in range(st.nlev)]
        job["style_planes"] = [_planes(st.guidance[0], st.hs >> l, st.ws >> l) for l in range(st.nlev)]
    _JOBS[st.name] = job
    return job


def _apply_settings(eng, st):
    """What a caller applies for a new job: configure, the setters the station names, the documented reset_* for the rest."""
    eng.configure(st.nlev, st.h, st.w)
    if st.style_weights is None:
        eng.reset_style_weights()
    eng.set_taps(*st.taps) if st.taps else eng.reset_taps()
    eng.set_color("luminance") if st.color == "luminance" else eng.reset_color()
    eng.set_pooling("avg") if st.pooling == "avg" else eng.reset_pooling()
    if st.style_weights is not None:
        eng.set_style_weights(st.style_weights)
    eng.set_laplacian(*st.laplacian) if st.laplacian else eng.reset_laplacian()
    eng.set_matting(*st.matting) if st.matting else eng.reset_matting()
    eng.set_gram_shift(list(st.gram_shift)) if st.gram_shift else eng.reset_gram_shift()
    eng.set_moments(*st.moments) if st.moments else eng.reset_moments()
    return repr((eng.levels, eng.shape, eng.lib.nst_job_color(eng.ctx), eng.lib.nst_job_pooling(eng.ctx), eng.style_weights(),
                 eng.laplacian_setting(), eng.matting_setting(), eng.gram_shift_setting(), eng.moments_setting(),
                 [eng.guidance(l)[0] for l in range(st.nlev)], [eng.map_stats(l) for l in range(st.nlev)]))


def _apply_targets(eng, st):
    job = _job(st)
    for l in range(st.nlev):
        if st.guidance:
            eng.set_guidance(l, job["planes"][l], st.guidance[1])
            eng.set_targets_guided(l, job["content"][l], job["style"][l], job["style_planes"][l])
        elif st.blend:
            eng.set_targets_blend(l, job["content"][l], [job["style"][l], job["style2"][l]], [list(r) if isinstance(r, tuple) else r
                                                                                              for r in st.blend])
        else:
            eng.set_targets(l, job["content"][l], job["style"][l])


FIELDS = ("closures", "total_closures", "accepted", "loss", "lr", "t", "history")


def _info(info):
    return np.array([int(np.asarray(getattr(info, f), dtype=np.float32).view(np.uint32)) if f in ("loss", "lr", "t")
                     else int(getattr(info, f)) for f in FIELDS], dtype=np.int64)


def run_optimiser(eng, st, between=None, steps=4):
    """Four steps of the station's optimiser from a copy of its start image; `between(i)` runs before step i >= 1."""
    from artstyletransfer_amd.engine import PixelOptimizer
    opt = PixelOptimizer(eng, "lbfgs", 1.0, 26) if st.eval[0] == "lbfgs" else PixelOptimizer(eng, "adam", 10.0, 1)
    out = collections.OrderedDict()
    try:
        x = _job(st)["x"].clone()
        for i in range(steps):
            if between is not None and i:
                between(i)
            info, rows = opt.step(x, CW, SW, TVW)
            out[f"step {i} info {FIELDS}"] = _info(info)
            out[f"step {i} loss rows"] = _bits(rows)
            out[f"step {i} x"] = _bits(x)
        out["history()"] = np.array(opt.history())
        out["closure_stats()"] = np.array(opt.closure_stats())
        out["backward_stats()"] = np.array(opt.backward_stats())
    finally:
        opt.close()
    return out


def _evaluate(eng, st, graph):
    """The kept result of a station on a configured engine: an ordered dict of bit patterns, the cheap diagnostics first."""
    job = _job(st)
    x = job["x"]
    kind = st.eval[0]
    mask = st.eval[1] if kind == "levels" else (1 << st.nlev) - 1
    out = collections.OrderedDict()
    grad = torch.full((1, eng.channels, st.h, st.w), SENTINEL, device=x.device)
    losses = torch.full((4 * st.nlev + 1,), SENTINEL, device=x.device)
    if kind in ("closure", "levels"):
        for _ in range(3 if graph else 1):           # use_graph: the same three calls into the same buffers (capture, replay)
            if kind == "closure":
                eng.closure(x, CW, SW, TVW, grad=grad, losses=losses)
            else:
                eng.closure_levels(x, CW, SW, TVW, mask, grad=grad, losses=losses)
    elif kind == "halves":
        eng.closure_forward(x, CW, SW, TVW, losses=losses)
        eng.closure_backward(x, CW, SW, TVW, grad=grad)
    elif kind == "window":
        from artstyletransfer_amd.sharding import StripePlan
        plans = [StripePlan(st.h, 2, r) for r in range(2)]
        assert all(p.ext_rows == st.h for p in plans) and plans[0].own[1] == plans[1].own[0]     # (the halo spans this image)
        sums = None
        for p in plans:
            # (the last of the nst_window_sums_count words is padding no call writes: a filled buffer, not torch.empty's bytes)
            part = eng.window_begin(p.cut(x), p.row0, p.rows, st.h, sums=torch.full((eng.window_sums_count(),), SENTINEL, device=x.device))
            out[f"stripe {p.own} sums"] = _bits(part)
            sums = part.clone() if sums is None else sums + part
        grad.zero_()
        for p in plans:
            xs = p.cut(x)
            eng.window_begin(xs, p.row0, p.rows, st.h)
            gxs, row = eng.window_end(xs, p.row0, p.rows, st.h, CW, SW, TVW, sums.clone())
            out[f"stripe {p.own} loss row"] = _bits(row)
            p.add_into(grad, gxs)
            losses = row
    else:
        out.update(run_optimiser(eng, st))
    if kind not in ("adam", "lbfgs"):
        out["loss row"] = _bits(losses)
    if st.laplacian:
        out["laplacian_losses()"] = _bits(eng.laplacian_losses())
    if st.matting:
        out["matting_losses()"] = _bits(eng.matting_losses())
    if st.moments:
        out["moment_losses()"] = _bits(eng.moment_losses())
    lv = [l for l in range(st.nlev) if (mask >> l) & 1]
    if st.gram_shift:
        for l in lv:
            for q in range(len(eng.taps[1])):
                out[f"level {l} gram offsets of slot {q}"] = _bits(eng.level_gram_offsets(l, q))
    top = max(TAP_LAYER[i] for i in (eng.taps[0],) + tuple(eng.taps[1]))
    for l in lv:
        for layer in (0, top):
            out[f"level {l} activation of conv layer {layer}"] = _bits(eng.level_activation(l, layer))
    if kind not in ("adam", "lbfgs"):
        out["gradient"] = _bits(grad)
    torch.cuda.synchronize()
    return out


def first_difference(ref, got):
    if list(ref) != list(got):
        return "the kept quantities themselves: " + str(sorted(set(ref) ^ set(got)))
    for k in ref:
        if isinstance(ref[k], str):
            if ref[k] != got[k]:
                return f"{k}: {got[k]} instead of {ref[k]}"
        elif ref[k].shape != got[k].shape or not np.array_equal(ref[k], got[k]):
            n = int((ref[k] != got[k]).sum()) if ref[k].shape == got[k].shape else -1
            return f"{k} ({n} of {ref[k].size} words)"
    return None


def _floats(bits):
    return bits.view(np.float32)


def _guard(st, res):
    """Vacuity guards on a fresh result: a finite non-zero gradient, every enabled term's loss entry > 0."""
    if st.eval[0] in ("adam", "lbfgs"):
        rows = _floats(res["step 0 loss rows"])[0]
        assert any(res[f"step {i} info {FIELDS}"][2] for i in range(4)), st.name
        assert not np.array_equal(res["step 3 x"], res["step 0 x"]) and np.isfinite(_floats(res["step 3 x"])).all(), st.name
        if st.eval[0] == "lbfgs":
            assert res["history()"][0] > 0 and res[f"step 3 info {FIELDS}"][0] > 1, st.name       # accepted steps, a line search
    else:
        rows = _floats(res["loss row"])
        g = _floats(res["gradient"])
        assert np.isfinite(g).all() and np.abs(g).max() > 0 and not (g == SENTINEL).any(), st.name
    mask = st.eval[1] if st.eval[0] == "levels" else (1 << st.nlev) - 1
    lv = [l for l in range(st.nlev) if (mask >> l) & 1]
    assert np.isfinite(rows).all() and rows[-1] > 0, st.name
    assert (rows[:-1].reshape(-1, 4)[lv if st.eval[0] != "window" else [0]] > 0).all(), (st.name, rows)
    if st.laplacian:
        assert (_floats(res["laplacian_losses()"]).reshape(st.nlev, 4)[lv][:, :2] > 0).all(), st.name
    if st.matting:
        assert (_floats(res["matting_losses()"])[lv] > 0).all(), st.name
    if st.moments:                                                          # every weighted (level, map, term) entry
        ml = _floats(res["moment_losses()"]).reshape(st.nlev, 6, 2)[lv]
        on = np.stack([np.array(st.moments[0]) > 0, np.array(st.moments[1]) > 0], axis=1)
        assert np.isfinite(ml).all() and (ml[:, on] > 0).all(), (st.name, ml)
    if st.gram_shift:
        assert any(res[k].any() for k in res if "gram offsets" in k), st.name
    assert all(res[k].any() for k in res if "activation" in k), st.name


def fresh(variant, weights):
    """The fresh results of a variant: one new StyleEngine per station, made once per variant and shared by every test."""
    if variant in _FRESH:
        return _FRESH[variant]
    from artstyletransfer_amd.engine import StyleEngine
    out = collections.OrderedDict()
    for name in kept(variant):
        st = BY_NAME[name]
        eng = StyleEngine(weights, 0, **VARIANTS[variant])
        try:
            settings = _apply_settings(eng, st)
            _apply_targets(eng, st)
            res = collections.OrderedDict(settings=settings)
            res.update(_evaluate(eng, st, bool(VARIANTS[variant].get("use_graph"))))
        finally:
            eng.close()
        _guard(st, res)
        out[name] = res
    _FRESH[variant] = out
    return out


# ---- the disturbances ---------------------------------------------------------------------------------------------------------------
def _foreign():
    if not _FOREIGN:
        g = torch.Generator().manual_seed(2024)
        r = lambda *shape: torch.rand(*shape, generator=g)                                       # noqa: E731
        n = lambda *shape: torch.randn(*shape, generator=g)                                      # noqa: E731
        f = {"x35": 255.0 * r(1, 3, 35, 51) - 120.0, "g0": n(1, 64, 35, 51), "g2": n(1, 256, 8, 12), "g5": n(1, 512, 2, 3),
             "f64": n(1, 64, 23, 37).abs(), "f256": n(1, 256, 9, 13).abs(), "gf": n(45, 64), "gp": r(2, 45), "gs": n(2, 64, 64),
             "y": 255.0 * r(1, 3, 35, 51) - 120.0, "guide": r(1, 3, 35, 51), "x36": n(1, 3, 36, 52), "gy": n(1, 3, 18, 26),
             "hwc": r(35, 51, 3), "ax": n(5355), "ag": n(5355), "am": 0.1 * n(5355), "av": 0.01 * n(5355).abs()}
        ss = [0.1 * n(5355) for _ in range(7)]
        f["ys"] = [2.0 * s + 0.03 * n(5355) for s in ss]
        f["ss"] = ss
        f["ro"] = [float(1.0 / y.dot(s)) for y, s in zip(f["ys"], ss)]
        f["hd"] = float(f["ys"][-1].dot(ss[-1]) / f["ys"][-1].dot(f["ys"][-1]))
        for k, v in f.items():
            _FOREIGN[k] = [dev(t) for t in v] if isinstance(v, list) and isinstance(v[0], torch.Tensor) else (dev(v) if isinstance(v, torch.Tensor) else v)
    return _FOREIGN


def _raw_backward(eng, x, grad, cw=CW):
    return eng.lib.nst_closure_backward(eng.ctx, C.c_void_p(x.data_ptr()), cw, SW, TVW, 0xFFFFFFFF, C.c_void_p(grad.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _refused(eng, fn, *codes):
    from artstyletransfer_amd import _lib
    with pytest.raises(_lib.NstError) as e:
        fn()
    assert any(f"({c})" in str(e.value) for c in codes), str(e.value)


def disturb(eng, name, x, variant):
    """One call of a serving process on engine `eng`, whose current job's start image is `x` (never written).  The standalone
    pieces are pure functions of their caller buffers: their results are held to the bits of the first time they ran on this
    variant (the network ones under the same pooling / use_relu, which they document they read)."""
    from artstyletransfer_amd import _lib
    f = _foreign()
    f16x2 = VARIANTS[variant].get("conv_mode") is None
    halves = f16x2 and VARIANTS[variant].get("batched") is not False and not VARIANTS[variant].get("use_graph")
    key = (variant, name)
    res = None
    if name == "vgg_features":
        res, key = eng.vgg_features(f["x35"]), key + (eng.pooling, eng.taps[2])
    elif name == "vgg_activations":
        res, key = eng.vgg_activations(f["x35"]), key + (eng.pooling, eng.taps[2])
    elif name == "vgg_features_backward":
        res, key = [eng.vgg_features_backward(f["x35"], [f["g0"], None, f["g2"], None, None, f["g5"]])], key + (eng.pooling, eng.taps[2])
    elif name == "gram64":
        res = [eng.gram(f["f64"])]
    elif name == "gram256":
        res = [eng.gram(f["f256"])]
    elif name in ("gram_shifted64", "gram_shifted256"):
        call = (lambda: eng.gram_shifted(f["f64"], shift=0.5)) if name.endswith("64") else (lambda: eng.gram_shifted(f["f256"], center=True))
        if f16x2:
            res = list(call())
        else:
            _refused(eng, call, _lib.NST_E_STATE)
    elif name == "guided_gram_backward":
        res = [eng.guided_gram_backward(f["gf"], f["gp"], f["gs"])]
    elif name == "total_variation":
        res = list(eng.total_variation(f["y"], want_grad=True))
    elif name == "laplacian_loss":
        res = list(eng.laplacian_loss(f["y"], f["x35"], 2, want_grad=True))
    elif name == "matting_loss":
        res = list(eng.matting_loss(f["y"], f["guide"], want_grad=True))
    elif name == "bicubic_half":
        res = [eng.bicubic_half(f["x36"])]
    elif name == "bicubic_half_backward":
        res = [eng.bicubic_half_backward(f["gy"], 36, 52)]
    elif name == "resize":
        res = [eng.resize(f["hwc"], 20, 30)]
    elif name == "color_stats":
        res = list(eng.color_stats(f["hwc"]))
    elif name == "color_affine":
        res = [eng.color_affine(f["hwc"], np.array([[0.9, 0.1, 0.0], [0.0, 1.1, -0.1], [0.05, 0.0, 0.95]]), np.array([0.01, -0.02, 0.03]))]
    elif name == "luminance":
        res = [eng.luminance(f["hwc"], 0.9, 0.05)]
    elif name == "adam_step":
        xx, m, v = f["ax"].clone(), f["am"].clone(), f["av"].clone()
        eng.adam_step(xx, f["ag"], m, v, 3, 9.98)
        res = [xx, m, v]
    elif name == "lbfgs_direction":
        res = [eng.lbfgs_direction(f["ag"], f["ys"], f["ss"], f["ro"], f["hd"], 0)]
    elif name == "refused_backward":                       # no forward half of these weights is pending, whatever came before
        grad = torch.full_like(x, SENTINEL)
        assert _raw_backward(eng, x, grad, cw=2.0 * CW) == _lib.NST_E_STATE
        torch.cuda.synchronize()
        assert bool((grad == SENTINEL).all())
    elif name == "abandoned_forward":                      # at another image, never followed by its backward
        other = (0.5 * x).contiguous()
        if halves and eng.levels > 1:
            eng.closure_forward(other, CW, SW, TVW)
        else:                                              # (also one level below 256 x 256: the per-level walker)
            _refused(eng, lambda: eng.closure_forward(other, CW, SW, TVW), _lib.NST_E_UNAVAILABLE)
    elif name == "refused_configure":
        assert eng.lib.nst_job_configure(eng.ctx, 9, 4096, 4096) == _lib.NST_E_ARG
    elif name == "refused_gram_shift":
        assert eng.lib.nst_job_set_gram_shift(eng.ctx, (C.c_float * 6)(0.0, float("nan"), 0.0, 0.0, 0.0, 0.0), 0) == _lib.NST_E_ARG
    elif name == "moments":
        res = list(eng.moments(f["f64"])) + list(eng.moments(f["f256"], 1e-3))
    elif name == "refused_moments":
        # a positive weight while a level is guided: NST_E_STATE; elsewhere a NaN weight: NST_E_ARG - "with nothing changed"
        one = (C.c_float * 6)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        before = eng.moments_setting()
        if eng.levels and eng.guidance(0)[0]:
            assert eng.lib.nst_job_set_moments(eng.ctx, one, one, 1e-5) == _lib.NST_E_STATE
        else:
            assert eng.lib.nst_job_set_moments(eng.ctx, (C.c_float * 6)(0.0, float("nan"), 0.0, 0.0, 0.0, 0.0), one, 1e-5) == _lib.NST_E_ARG
        assert eng.moments_setting() == before
    elif name == "moment_losses":
        eng.moment_losses()
    elif name == "closure_schedule":
        assert set(eng.last_closure_schedule()) == {"side_forks", "level_streams", "graph_replay"}
    elif name == "timed_closure":
        eng.set_timing(2)
        try:
            eng.closure((0.5 * x).contiguous(), CW, SW, TVW)
        finally:
            eng.set_timing(0)
    elif name == "level_activations0":
        eng.level_activations(0)
    elif name == "level_activation":
        eng.level_activation(1, 0)
    elif name == "level_image":
        eng.level_image(1)
    elif name == "laplacian_losses":
        eng.laplacian_losses()
    elif name == "matting_losses":
        eng.matting_losses()
    elif name == "level_gram_offsets":
        if eng.gram_shift is not None:
            eng.level_gram_offsets(1, 0)
        else:
            _refused(eng, lambda: eng.level_gram_offsets(1, 0), _lib.NST_E_STATE)
    elif name == "guidance_planes":
        if eng.guidance(1)[0]:
            eng.guidance_planes(1, 2)
        else:
            _refused(eng, lambda: eng.guidance_planes(1, 2), _lib.NST_E_STATE)
    else:
        raise KeyError(name)
    _COUNTS[variant] += 1
    if res is not None:
        got = [_bits(t) for t in res]
        first = _FIRST.setdefault(key, got)
        for i, (a, b) in enumerate(zip(first, got)):
            assert a.shape == b.shape and np.array_equal(a, b), f"{name}: result {i} differs from the first time it ran ({key})"


# ---- part 1: the walk -----------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
_T0 = []


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    _T0.append(time.time())
    yield
    if _FRESH:
        report(f"context history: module wall time {time.time() - _T0[0]:.1f} s")


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fresh_results_are_not_vacuous(vgg_weights, variant):
    """Per station on the fresh result: _guard; the three amplitude stations differ from each other; any two stations of one
    geometry differ in at least one kept quantity."""
    res = fresh(variant, vgg_weights)
    for a in AMPLITUDE:
        for b in AMPLITUDE:
            if a < b:
                assert not np.array_equal(res[a]["gradient"], res[b]["gradient"]) and not np.array_equal(res[a]["loss row"], res[b]["loss row"])
    names = list(res)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            sa, sb = BY_NAME[a], BY_NAME[b]
            if (sa.h, sa.w, sa.nlev) == (sb.h, sb.w, sb.nlev):
                ra = {k: v for k, v in res[a].items() if k != "settings"}
                rb = {k: v for k, v in res[b].items() if k != "settings"}
                assert first_difference(ra, rb) is not None, (a, b)


@gpu
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_engine_walks_the_stations_and_gives_the_fresh_bits(vgg_weights, variant, order):
    from artstyletransfer_amd.engine import StyleEngine
    ref = fresh(variant, vgg_weights)
    seq = order_of(variant, order)
    oi = list(ORDERS).index(order)
    graph = bool(VARIANTS[variant].get("use_graph"))
    before = _COUNTS[variant]
    bad = []
    eng = StyleEngine(vgg_weights, 0, **VARIANTS[variant])
    try:
        for p, name in enumerate(seq):
            st = BY_NAME[name]
            if p:
                for d in picks(oi, p):
                    disturb(eng, d, _job(BY_NAME[seq[p - 1]])["x"], variant)
            where = f"order {order} position {p}: station {name} after {seq[p - 1] if p else None} (then {picks(oi, p) if p else ()})"
            if order == "sweep" and p and same_job(BY_NAME[seq[p - 1]], st):
                settings = ref[name]["settings"]                 # the job stays: a new image, at odd positions new targets
                if p % 2:
                    _apply_targets(eng, st)
            else:
                settings = _apply_settings(eng, st)
                # on the host, before anything of the station is launched: a setting that outlived its buffers must not reach a kernel
                assert settings == ref[name]["settings"], f"{where}: settings read back {settings} instead of {ref[name]['settings']}"
                _apply_targets(eng, st)
            got = collections.OrderedDict(settings=settings)
            got.update(_evaluate(eng, st, graph))
            diff = first_difference(ref[name], got)
            if diff:
                bad.append(f"{where}: {diff}")
    finally:
        eng.close()
    report(f"context history, {variant} order {order}: {len(seq)} stations ({len(set(seq))} different), {_COUNTS[variant] - before} disturbances, "
           f"{len(bad)} stations off the fresh bits")
    assert not bad, "\n".join(bad)


# ---- part 2: between the halves, and between optimiser steps ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


def _set_up(eng, name):
    st = BY_NAME[name]
    _apply_settings(eng, st)
    _apply_targets(eng, st)
    return st, _job(st)["x"]


@gpu
@pytest.mark.parametrize("job", ("rgb_lap_mat", "shift_taps", "guided_rgb", "mom_lum_lap_mat"))
def test_one_call_between_the_halves(eng, vgg_weights, job):
    """closure_forward(x), ONE other call, closure_backward(x) into a sentinel-filled buffer.  Contract (a): the gradient is bitwise
    nst_closure's (the fresh engine's).  Contract (b): NST_E_STATE, the buffer untouched, and the next closure gives the fresh
    bits.  rgb_lap_mat (64x96 L2, Laplacian and matting on) takes every call; the shifted, the guided and the moment job take
    the read-backs and refusals that need them (the moment job: its row biases and folded S wait between the halves)."""
    from artstyletransfer_amd import _lib
    ref = fresh("default", vgg_weights)[job]
    st, x = _set_up(eng, job)
    calls = list(DISTURBANCES.items()) + list(READ_BACKS.items())
    if job == "shift_taps":
        calls = [("level_gram_offsets", "a"), ("level_activation", "b")]
    elif job == "guided_rgb":
        calls = [("guidance_planes", "a"), ("level_image", "a"), ("refused_moments", "b")]     # (refused BECAUSE the level is guided)
    elif job == "mom_lum_lap_mat":
        calls = [("moment_losses", "a"), ("closure_schedule", "a"), ("moments", "a"), ("laplacian_losses", "a"), ("refused_moments", "b")]
    bad = []
    for name, contract in calls:
        eng.closure_forward(x, CW, SW, TVW)
        disturb(eng, name, x, "default")
        grad = torch.full_like(x, SENTINEL)
        rc = _raw_backward(eng, x, grad)
        torch.cuda.synchronize()
        if contract == "a":
            if rc != 0:
                bad.append(f"{name}: the backward half was refused ({rc}) where the header keeps it valid")
            elif not np.array_equal(_bits(grad), ref["gradient"]):
                bad.append(f"{name}: the gradient of the backward half is not the closure's")
        else:
            if rc != _lib.NST_E_STATE:
                bad.append(f"{name}: nst_closure_backward returned {rc}, not NST_E_STATE")
            elif not bool((grad == SENTINEL).all()):
                bad.append(f"{name}: a refused backward wrote the gradient buffer")
            g, l = eng.closure(x, CW, SW, TVW)
            if not (np.array_equal(_bits(g), ref["gradient"]) and np.array_equal(_bits(l), ref["loss row"])):
                bad.append(f"{name}: the closure after the refusal is off the fresh bits")
    report(f"context history, between the halves of {job}: {len(calls)} calls, {len(bad)} off their contract")
    assert not bad, "\n".join(bad)


@gpu
def test_one_call_between_lbfgs_steps(eng, vgg_weights):
    """Four L-BFGS steps (max_eval 26, closure reuse and lazy backward at their defaults) with one call of the list between
    consecutive steps - three per run, every call of the list over the runs - and once with a closure at ANOTHER image between
    the steps, which the reuse cache must not serve: every step's x, loss rows and info fields are the undisturbed run's."""
    ref = fresh("default", vgg_weights)["lbfgs"]
    st, x = _set_up(eng, "lbfgs")
    calls = list(DISTURBANCES) + list(READ_BACKS)
    runs = [calls[i:i + 3] for i in range(0, len(calls), 3)]
    other = (0.5 * x).contiguous()
    bad = []
    for chunk in runs + [["closure at another image"] * 3]:
        def between(i, chunk=chunk):
            name = chunk[(i - 1) % len(chunk)]
            if name == "closure at another image":
                eng.closure(other, CW, SW, TVW)
            else:
                disturb(eng, name, x, "default")
        got = run_optimiser(eng, st, between)
        keys = [k for k in ref if k.startswith("step ")]
        diff = first_difference({k: ref[k] for k in keys}, {k: got[k] for k in keys})
        if diff:
            bad.append(f"{chunk}: {diff}")
    report(f"context history, between L-BFGS steps: {len(runs) + 1} runs of 4 steps, {len(bad)} off the undisturbed run")
    assert not bad, "\n".join(bad)


# ---- part 3: two contexts on one device, interleaved ---------------------------------------------------------------------------------
@gpu
def test_two_contexts_interleaved_share_nothing(vgg_weights):
    """A (68x260 L3, default settings) and B (64x96 L2, luminance + avg pooling + matting) alive together on the current stream:
    A.forward, B.closure, A.backward, B.forward, A.closure, B.backward - every result bitwise the solo one."""
    from artstyletransfer_amd.engine import StyleEngine
    ref = fresh("default", vgg_weights)
    a, b = StyleEngine(vgg_weights, 0), StyleEngine(vgg_weights, 0)
    try:
        (_, xa), (_, xb) = _set_up(a, "plain3"), _set_up(b, "lum_avg_mat")
        ra, rb = ref["plain3"], ref["lum_avg_mat"]
        la = a.closure_forward(xa, CW, SW, TVW)
        gb, lb = b.closure(xb, CW, SW, TVW)
        ga = a.closure_backward(xa, CW, SW, TVW, grad=torch.full_like(xa, SENTINEL))
        lb2 = b.closure_forward(xb, CW, SW, TVW)
        ga2, la2 = a.closure(xa, CW, SW, TVW)
        gb2 = b.closure_backward(xb, CW, SW, TVW, grad=torch.full_like(xb, SENTINEL))
        torch.cuda.synchronize()
        for what, t, want in (("A.closure_forward", la, ra["loss row"]), ("B.closure loss row", lb, rb["loss row"]),
                              ("B.closure gradient", gb, rb["gradient"]), ("A.closure_backward", ga, ra["gradient"]),
                              ("B.closure_forward", lb2, rb["loss row"]), ("A.closure loss row", la2, ra["loss row"]),
                              ("A.closure gradient", ga2, ra["gradient"]), ("B.closure_backward", gb2, rb["gradient"])):
            assert np.array_equal(_bits(t).reshape(-1), want.reshape(-1)), what
        assert np.array_equal(_bits(b.matting_losses()), rb["matting_losses()"])
    finally:
        a.close()
        b.close()
