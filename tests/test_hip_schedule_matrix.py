"""GPU: every job setting under every schedule, held to the bits of the schedule's twin.

include/nst_hip.h promises that each job setting (taps, luminance, average pooling, style layer weights, blends, guidance, the
Laplacian and matting terms, the Gram shift, the moment loss) composes with every schedule.  The schedule switches were tested
on one plain RGB job, the settings on the default engine and on batched=False.  Where the two meet is host code: the overlap
predicate and the 0x07 / 0x18 split of the style maps (with the offset, row-bias and moment riders of each batch), the two
chains of level_split on the side stream, the persistent tile chain with its row bias / second K source / pooling epilogue /
guided addend, and what use_graph switches off.  A schedule launches the same kernels on the same tiles as its twin and the
closure is bitwise reproducible: a missing join, a dropped mask bit or a rider left off a side-stream batch is a different bit.

  part 0 (CPU)  every setter, set and unset, under every schedule; a multi-level station under each; the table of expected
                side forks against a restatement of the overlap predicate (test_plan_*).
  part 1        per schedule ONE engine walks the stations of tests/test_hip_context_history.py (its machinery is imported,
                not copied) and every kept quantity is compared with the twin's - bitwise, the four-step L-BFGS and Adam
                trajectories included.  level_split alone has another twin: the two masked closures of the default engine.
  part 2        h2_persist on images with more tiles than the chip holds workgroups.
  part 3        a captured graph does not outlive a setting that arrives on a kept job.

That the schedule RAN is read from the library (nst_last_closure_schedule, nst_last_closure_launches), on a probe closure made
after the compared one; a station on which it did not run fails.  A mismatch is reported as (schedule, station, first
differing quantity)."""
import collections
import time

import numpy as np
import pytest
import torch

from hip_helpers import CW, SW, TVW, rel_l2, report
from test_hip_context_history import (BY_NAME, SENTINEL, SETTERS, STATIONS, W_ONE, M_ONE, M_TWO, Station, _apply_settings, _apply_targets,
                                      _bits, _evaluate, _floats, _guard, _job, first_difference, fresh, is_set)

Schedule = collections.namedtuple("Schedule", "opts twin_opts twin_fresh")       # twin_fresh: the variant of fresh() with the twin's bits
SCHEDULES = collections.OrderedDict((
    ("graph", Schedule(dict(use_graph=True), dict(), "default")),
    ("overlap", Schedule(dict(gram_overlap=True), dict(), "default")),
    ("one_stream", Schedule(dict(batched=False, single_stream=True), dict(batched=False), "per_level")),
    ("bands", Schedule(dict(batched=False, h2_band_rows=16), dict(batched=False), "per_level")),
    ("keep_maps", Schedule(dict(keep_all_maps=True), dict(), "default")),
    ("no_fwd_pack", Schedule(dict(forward_pack=False), dict(), "default")),
    ("no_gram_pack", Schedule(dict(gram_pack=False), dict(), "default")),
    ("split", Schedule(dict(level_split=True), dict(), "default")),
    ("split_overlap", Schedule(dict(level_split=True, gram_overlap=True), dict(level_split=True), None)),
    ("persist", Schedule(dict(h2_persist=True), dict(), None)),
))
WALKED = tuple(s for s in SCHEDULES if s != "persist")

# persist: the two smallest geometries of test_persistent_launches_are_bitwise_the_one_tile_launches (style = content - (64, 32)),
# four settings each; between them they hold every setter (the plan test), taps and a blend on the three-level geometry
_G_SHIFT = (0.5, "mean", 0.0, "mean", 0.0, -0.25)
_LAP, _MAT = ((1, 2), (3.0, 40.0)), (2.8e8, 1e-7)
PERSIST_STATIONS = (
    Station("p528_plain", 528, 336, 2, 464, 304, 21),
    Station("p528_avg_shift_mom", 528, 336, 2, 464, 304, 21, pooling="avg", style_weights=W_ONE, gram_shift=_G_SHIFT, moments=M_ONE),
    Station("p528_lum_lap_mat", 528, 336, 2, 464, 304, 21, color="luminance", laplacian=_LAP, matting=_MAT),
    Station("p528_guided", 528, 336, 2, 464, 304, 21, guidance=("columns", None)),
    Station("p400_plain", 400, 600, 3, 336, 568, 21),
    Station("p400_avg_shift_mom", 400, 600, 3, 336, 568, 21, pooling="avg", style_weights=W_ONE, gram_shift=_G_SHIFT, moments=M_TWO,
            blend=(0.25, 0.75)),
    Station("p400_lum_lap_mat", 400, 600, 3, 336, 568, 21, color="luminance", laplacian=_LAP, matting=_MAT),
    Station("p400_guided", 400, 600, 3, 336, 568, 21, taps=(2, (2, 3), True), guidance=("rows", (1.0, 0.5))),
)
PERSIST_GEOMETRIES = ((528, 336, 2), (400, 600, 3))


def mask_of(st):
    return st.eval[1] if st.eval[0] == "levels" else (1 << st.nlev) - 1


def batch_eligible(st):
    """nst_closure.cpp batch_eligible on a batched f16x2 engine: several levels, or one of at least 256 x 256 pixels."""
    return st.nlev > 1 or st.h * st.w >= 256 * 256


def stations_of(schedule):
    """The stations a schedule is held on.  The closure kinds of the context-history file; the two optimiser stations where the
    comparison is bitwise against an engine (all but split, whose twin is two masked closures); the halves left out where
    nst_closure_forward is unavailable (kept()'s rule: the per-level schedule and use_graph); the split schedules only where the
    split happens - a level mask with level 0 AND a lower level."""
    if schedule == "persist":
        return PERSIST_STATIONS
    opts = SCHEDULES[schedule].opts
    no_halves = opts.get("batched") is False or opts.get("use_graph")
    kinds = ("closure", "levels", "halves") + (() if schedule == "split" else ("lbfgs", "adam"))
    out = []
    for s in STATIONS:
        if s.eval[0] not in kinds or (no_halves and s.eval[0] == "halves"):
            continue
        if opts.get("level_split") and not (mask_of(s) & 1 and mask_of(s) & ~1):
            continue
        out.append(s)
    return tuple(out)


# side forks of one whole closure (nst_last_closure_schedule) under gram_overlap, written down per station: 1 = the overlap runs,
# 0 = the library falls back to one stream (non-default taps, guided levels, or the per-level walker of a small one-level job)
OVERLAP_FORKS = {
    "plain3": 1, "plain3_hi": 1, "plain3_lo": 1, "lum_lap_mat": 1, "lum_avg_mat": 1, "avg_guided": 0, "shift_blend": 1, "shift_taps": 0,
    "six_norelu": 0, "small_lap_blend": 0, "lbfgs": 1, "guided_rgb": 0, "rgb_lap_mat": 1, "weights_level0": 1, "adam_lum": 0,
    "moments3": 1, "mom_shift_blend_avg": 1, "mom_lum_lap_mat": 1, "mom_taps_norelu": 0,
}


def expected_counters(schedule, st):
    """(side_forks, level_streams, graph_replay) of the probe: one whole nst_closure_levels of the station's mask (use_graph:
    the third of three calls into the same buffers).  level_split switches gram_overlap off (one side stream,
    include/nst_hip.h): split_overlap forks as split does - the split's one fork plus one per chain that overlaps, of which
    there is none."""
    if schedule == "graph":
        return (0, 0, 1 if batch_eligible(st) else 0)
    if schedule == "overlap":
        return (OVERLAP_FORKS[st.name], 0, 0)
    if schedule in ("split", "split_overlap"):
        return (1, 0, 0)
    if schedule == "bands":     # (the per-level schedule on its per-level streams, as its twin: the bands are read from the launch record)
        return (0, st.nlev if st.nlev > 1 else 0, 0)
    return (0, 0, 0)            # one_stream: no per-level stream; keep_maps / no_*_pack / persist: the counters say nothing


# ---- part 0: the plan (CPU) ---------------------------------------------------------------------------------------------------------
def test_plan_every_setter_is_set_and_unset_under_every_schedule():
    for schedule in SCHEDULES:
        sts = stations_of(schedule)
        assert len(sts) >= 8 and len({s.name for s in sts}) == len(sts), schedule
        for setter in SETTERS:
            assert any(is_set(s, setter) for s in sts) and any(not is_set(s, setter) for s in sts), (schedule, setter)
        assert any(s.moments for s in sts) and "moments" in SETTERS
    assert set(SETTERS) <= set(Station._fields)
    for schedule in WALKED:                                # the four moment stations of the context-history file, under each
        assert sum(1 for s in stations_of(schedule) if s.moments) == 4, schedule
    assert {(s.h, s.w, s.nlev) for s in PERSIST_STATIONS} == set(PERSIST_GEOMETRIES)
    for geo in PERSIST_GEOMETRIES:
        mine = [s for s in PERSIST_STATIONS if (s.h, s.w, s.nlev) == geo]
        assert len(mine) == 4 and not any(is_set(mine[0], k) for k in SETTERS)
        assert any(s.pooling == "avg" and s.gram_shift and s.moments and s.style_weights for s in mine)
        assert any(s.color == "luminance" and s.laplacian and s.matting for s in mine)
        assert any(s.guidance for s in mine)


def test_plan_every_schedule_has_a_multi_level_station_and_the_kinds_it_is_held_on():
    for schedule in SCHEDULES:
        sts = stations_of(schedule)
        assert any(s.nlev > 1 for s in sts) and any(s.nlev >= 3 for s in sts), schedule
        kinds = {s.eval[0] for s in sts}
        assert "window" not in kinds
        if schedule in ("split", "split_overlap"):
            assert all(s.nlev > 1 and mask_of(s) & 1 and mask_of(s) & ~1 for s in sts)
            assert any(s.eval[0] == "levels" and mask_of(s) != (1 << s.nlev) - 1 for s in sts)        # a partial mask that still splits
        if schedule not in ("split", "persist"):
            assert "lbfgs" in kinds and (schedule == "split_overlap" or "adam" in kinds), schedule
        opts = SCHEDULES[schedule].opts
        assert ("halves" in kinds) == (not (opts.get("batched") is False or opts.get("use_graph")) and schedule != "persist"), schedule
    # the twins launch the same kernels on the same tiles: they differ from the schedule in the schedule's own switches only
    for name, sch in SCHEDULES.items():
        assert all(sch.opts[k] == v for k, v in sch.twin_opts.items()) and len(sch.opts) > len(sch.twin_opts), name


def test_plan_expected_side_forks_agree_with_the_overlap_predicate():
    """closure_batched_forward: overlap = gram_overlap && f16x2 && !use_graph && side stream && default taps && no guided level -
    on the batched walker (batch_eligible).  Both outcomes are on the list, each with moments, a Gram shift and a blend."""
    sts = stations_of("overlap")
    assert {s.name for s in sts} == set(OVERLAP_FORKS)
    for s in sts:
        runs = batch_eligible(s) and s.taps is None and s.guidance is None
        assert OVERLAP_FORKS[s.name] == int(runs), s.name
    ran = [s for s in sts if OVERLAP_FORKS[s.name]]
    fell = [s for s in sts if not OVERLAP_FORKS[s.name]]
    assert any(s.moments for s in ran) and any(s.gram_shift for s in ran) and any(s.blend for s in ran) and any(s.pooling == "avg" for s in ran)
    assert any(s.moments for s in fell) and any(s.gram_shift for s in fell) and any(s.guidance for s in fell) and any(s.taps for s in fell)
    assert all(expected_counters("split", s) == expected_counters("split_overlap", s) == (1, 0, 0) for s in stations_of("split_overlap"))
    assert any(not batch_eligible(s) for s in stations_of("graph")) and any(batch_eligible(s) for s in stations_of("graph"))


# ---- part 1: the walk ---------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
_T0 = []
_RAN = []
_TWIN = {}        # twin options -> {station name: kept result}: twins that fresh() does not hold


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    _T0.append(time.time())
    yield
    if _RAN:
        report(f"schedule matrix: module wall time {time.time() - _T0[0]:.1f} s")


def _words(res):
    return sum(v.size for v in res.values() if not isinstance(v, str))


def _counters(eng):
    c = eng.last_closure_schedule()
    return (c["side_forks"], c["level_streams"], c["graph_replay"])


def probe(eng, st, calls=1, timed=False, cw=CW):
    """One whole closure of the station's level mask AFTER the compared evaluation, at its start image: the schedule counters of
    each of `calls` calls into the same buffers, and (timed) the launch record of the last.  `cw`: use_graph keys its capture
    on the buffer addresses and the weights, and the allocator may hand the probe the addresses of the evaluation before it -
    another content weight makes the first call one the context has not seen."""
    x = _job(st)["x"]
    grad = torch.full((1, eng.channels, st.h, st.w), SENTINEL, device=x.device)
    losses = torch.full((4 * st.nlev + 1,), SENTINEL, device=x.device)
    seen, launches = [], []
    if timed:
        eng.set_timing(2)
    try:
        for _ in range(calls):
            eng.closure_levels(x, cw, SW, TVW, mask_of(st), grad=grad, losses=losses)
            seen.append(_counters(eng))
        if timed:
            launches = eng.last_closure_launches()
    finally:
        if timed:
            eng.set_timing(0)
    torch.cuda.synchronize()
    return seen, launches


def visit(eng, st, graph=False):
    settings = _apply_settings(eng, st)
    _apply_targets(eng, st)
    res = collections.OrderedDict(settings=settings)
    res.update(_evaluate(eng, st, graph))
    return res


def twin_results(schedule, weights):
    sch = SCHEDULES[schedule]
    if sch.twin_fresh:
        return fresh(sch.twin_fresh, weights)
    key = (schedule == "persist", tuple(sorted(sch.twin_opts.items())))
    if key not in _TWIN:
        from artstyletransfer_amd.engine import StyleEngine
        out = collections.OrderedDict()
        eng = StyleEngine(weights, 0, **sch.twin_opts)
        try:
            for st in stations_of(schedule):
                out[st.name] = visit(eng, st)
                _guard(st, out[st.name])
        finally:
            eng.close()
        _TWIN[key] = out
    return _TWIN[key]


def ran_check(schedule, eng, st):
    """None, or why the schedule did not run on the station as the plan says; and the counters read, for the report."""
    want = expected_counters(schedule, st)
    if schedule == "graph":
        seen, _ = probe(eng, st, calls=3, cw=2.0 * CW)
        if seen[0][2] != 0 or seen[2] != want:
            return f"graph: first call {seen[0]}, third call {seen[2]} instead of (0, 0, 0) and {want}", seen[2]
        return None, seen[2]
    seen, launches = probe(eng, st, timed=schedule in ("bands", "persist"))
    got = seen[0]
    if got != want:
        return f"(side_forks, level_streams, graph_replay) = {got} instead of {want}", got
    if schedule == "bands" and not any(l["h2_bands"] > 1 for l in launches):
        return "no launch of the timed closure ran in row bands", got
    if schedule == "persist" and not any(l["h2_persist"] == 1 for l in launches):
        return "no launch of the timed closure ran persistent workgroups", got
    return None, got


def split_reference(eng, st):
    """The twin of level_split: nst_closure_levels on the default engine with the masks of the two chains - level 0 alone, the
    lower levels among themselves - put together as the split closure reports them: every per-level quantity from the call
    that owns the level, the gradient g(mask 1) + g(mask rest) added in fp32 (one addend of every sum in the bicubic chain is
    zero).  The total of the loss row is a sum over all levels and has no twin here: it is held by the 1e-5 comparison."""
    m = mask_of(st)
    _apply_settings(eng, st)
    _apply_targets(eng, st)
    a = _evaluate(eng, st._replace(eval=("levels", m & 1)), False)
    b = _evaluate(eng, st._replace(eval=("levels", m & ~1)), False)
    out = collections.OrderedDict()
    for k in list(a) + [k for k in b if k not in a]:
        if k.startswith("level "):
            out[k] = a[k] if k.startswith("level 0 ") else b[k]
        elif k == "gradient":
            out[k] = (_floats(a[k]) + _floats(b[k])).view(np.uint32)
        else:
            rows = {"loss row": 4, "laplacian_losses()": 4, "matting_losses()": 1, "moment_losses()": 12}[k]
            va, vb = a[k].reshape(-1), b[k].reshape(-1)
            n = st.nlev * rows
            out[k] = np.concatenate([va[:rows], vb[rows:n]])
    return out


def split_shape(st, res):
    """A split closure's result in the layout of split_reference (key order included)."""
    out = collections.OrderedDict()
    for k in res:
        if k == "settings":
            continue
        if k.startswith("level ") or k == "gradient":
            out[k] = res[k]
        else:
            rows = {"loss row": 4, "laplacian_losses()": 4, "matting_losses()": 1, "moment_losses()": 12}[k]
            out[k] = res[k].reshape(-1)[: st.nlev * rows]
    return out


def trajectory(schedule, st, res):
    """use_graph has no forward half: its optimiser serves every trial point by a whole closure where the default engine's
    runs the forward half alone, so the two counters of HOW the closures were served are no twins.  Everything else is: x, loss
    rows and info fields of every step, and the history."""
    if schedule == "graph" and st.eval[0] in ("lbfgs", "adam"):
        return collections.OrderedDict((k, v) for k, v in res.items() if k not in ("closure_stats()", "backward_stats()"))
    return res


@gpu
@pytest.mark.parametrize("schedule", WALKED)
def test_schedule_gives_the_bits_of_its_twin_on_every_station(vgg_weights, schedule):
    from artstyletransfer_amd.engine import StyleEngine
    sch = SCHEDULES[schedule]
    twin = twin_results(schedule, vgg_weights)
    whole = fresh("default", vgg_weights) if schedule == "split" else None
    bad = []
    eng = StyleEngine(vgg_weights, 0, **sch.opts)
    ref_eng = StyleEngine(vgg_weights, 0) if schedule == "split" else None
    try:
        for st in stations_of(schedule):
            got = visit(eng, st, graph=schedule == "graph")
            try:
                _guard(st, got)
            except AssertionError as e:      # (reported with the rest: the walk goes on to the station's comparison)
                bad.append(f"({schedule}, {st.name}, vacuity guard: {(str(e).splitlines() or [''])[0][:120]})")
            if schedule == "split":
                ref, mine = split_reference(ref_eng, st), split_shape(st, got)
                assert sorted(ref) == sorted(mine), (st.name, sorted(set(ref) ^ set(mine)))
                diff = first_difference(collections.OrderedDict((k, ref[k]) for k in mine), mine)
                # beside it the default engine's WHOLE closure, at the figures of test_experiment_switches_agree_with_the_default:
                # the two smaller batches may pick other tile shapes than the one launch over all levels
                g0, g1 = _floats(whole[st.name]["gradient"]), _floats(got["gradient"])
                l0, l1 = _floats(whole[st.name]["loss row"]), _floats(got["loss row"])
                err = rel_l2(g1, g0)
                if not err < 1e-5:
                    bad.append(f"({schedule}, {st.name}, gradient rel-L2 {err:.2e} from the default whole closure, bound 1e-5)")
                if not np.allclose(l1, l0, rtol=1e-5, atol=0.0):
                    bad.append(f"({schedule}, {st.name}, loss row off the default whole closure: {l1} instead of {l0}, bound 1e-5)")
            else:
                diff = first_difference(trajectory(schedule, st, twin[st.name]), trajectory(schedule, st, got))
            why, counters = ran_check(schedule, eng, st)
            words = _words(got)
            report(f"schedule matrix, ({schedule}, {st.name}): {'bitwise its twin' if not diff else 'OFF: ' + diff}, {words} words, "
                   f"(side_forks, level_streams, graph_replay) = {counters}{'' if not why else ', SCHEDULE DID NOT RUN: ' + why}")
            if diff:
                bad.append(f"({schedule}, {st.name}, {diff})")
            if why:
                bad.append(f"({schedule}, {st.name}, the schedule did not run as planned: {why})")
        if schedule == "one_stream":
            # the twin's side of the same counter: the per-level schedule without single_stream forks to one stream per level
            t = StyleEngine(vgg_weights, 0, **sch.twin_opts)
            try:
                for name in ("plain3", "small_lap_blend"):
                    st = BY_NAME[name]
                    visit(t, st)
                    seen, _ = probe(t, st)
                    want = (0, st.nlev if st.nlev > 1 else 0, 0)
                    report(f"schedule matrix, (one_stream's twin, {name}): (side_forks, level_streams, graph_replay) = {seen[0]}")
                    if seen[0] != want:
                        bad.append(f"(one_stream's twin, {name}, counters {seen[0]} instead of {want})")
            finally:
                t.close()
    finally:
        eng.close()
        if ref_eng is not None:
            ref_eng.close()
    _RAN.append(schedule)
    assert not bad, "\n".join(bad)


# ---- part 2: persistent launches ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("h,w,nlev", PERSIST_GEOMETRIES)
def test_persistent_launches_give_the_one_tile_bits_under_every_setting(vgg_weights, h, w, nlev):
    """h2_persist needs more tiles than the chip holds workgroups: the two smallest geometries of
    test_persistent_launches_are_bitwise_the_one_tile_launches, four settings each.  The tile chain carries a per-image row
    bias (Gram shift, moments), a second K source, the average-pool epilogue and the guided addend.  The launch record of a
    timed closure must show a persistent launch on the persist engine and none on its twin."""
    from artstyletransfer_amd.engine import StyleEngine
    sch = SCHEDULES["persist"]
    bad = []
    eng, twin = StyleEngine(vgg_weights, 0, **sch.opts), StyleEngine(vgg_weights, 0, **sch.twin_opts)
    try:
        for st in PERSIST_STATIONS:
            if (st.h, st.w, st.nlev) != (h, w, nlev):
                continue
            ref, got = visit(twin, st), visit(eng, st)
            _guard(st, ref)
            diff = first_difference(ref, got)
            why, counters = ran_check("persist", eng, st)
            _, launches = probe(twin, st, timed=True)
            if any(l["h2_persist"] for l in launches):
                bad.append(f"(persist, {st.name}, the twin ran persistent launches itself)")
            report(f"schedule matrix, (persist, {st.name}): {'bitwise its twin' if not diff else 'OFF: ' + diff}, {_words(got)} words, "
                   f"(side_forks, level_streams, graph_replay) = {counters}{'' if not why else ', SCHEDULE DID NOT RUN: ' + why}")
            if diff:
                bad.append(f"(persist, {st.name}, {diff})")
            if why:
                bad.append(f"(persist, {st.name}, the schedule did not run as planned: {why})")
    finally:
        eng.close()
        twin.close()
    _RAN.append("persist")
    assert not bad, "\n".join(bad)


# ---- part 3: a captured graph and a setting that arrives on a kept job ----------------------------------------------------------------
@gpu
def test_captured_graph_does_not_outlive_a_moment_setting_on_a_kept_job(vgg_weights):
    """The walk configures every station anew, and nst_job_configure drops a captured graph by itself.  Here the job stays: the
    plain 68x260 three-level job is captured and replayed, then nst_job_set_moments arrives (no configure; the targets are set
    again, as the header asks) and the SAME image, gradient and loss buffers are passed again.  The first call after the setter
    must be no replay, and the third - a replay again - must give the default engine's bits of the moment job."""
    from artstyletransfer_amd.engine import StyleEngine
    plain, mom = BY_NAME["plain3"], BY_NAME["moments3"]
    assert plain._replace(name="") == mom._replace(name="", moments=None)
    ref = fresh("default", vgg_weights)
    x = _job(plain)["x"]
    grad = torch.full((1, 3, plain.h, plain.w), SENTINEL, device=x.device)
    losses = torch.full((4 * plain.nlev + 1,), SENTINEL, device=x.device)
    eng = StyleEngine(vgg_weights, 0, use_graph=True)
    try:
        _apply_settings(eng, plain)
        _apply_targets(eng, plain)
        seen = []
        for _ in range(3):
            eng.closure(x, CW, SW, TVW, grad=grad, losses=losses)
            seen.append(_counters(eng)[2])
        assert seen == [0, 1, 1], seen
        assert np.array_equal(_bits(grad), ref["plain3"]["gradient"]) and np.array_equal(_bits(losses), ref["plain3"]["loss row"])
        eng.set_moments(*mom.moments)
        _apply_targets(eng, mom)
        seen = []
        for _ in range(3):
            eng.closure(x, CW, SW, TVW, grad=grad, losses=losses)
            seen.append(_counters(eng)[2])
        torch.cuda.synchronize()
        assert seen == [0, 1, 1], f"graph replays after nst_job_set_moments: {seen}"
        assert np.array_equal(_bits(losses), ref["moments3"]["loss row"]), "loss row after the setter is not the moment job's"
        assert np.array_equal(_bits(grad), ref["moments3"]["gradient"]), "gradient after the setter is not the moment job's"
        assert np.array_equal(_bits(eng.moment_losses()), ref["moments3"]["moment_losses()"])
    finally:
        eng.close()
    _RAN.append("graph, kept job")
