"""GPU: closures of 4 to 8 pyramid levels and of all six style maps against the CPU oracle.

nst_job_configure takes levels_num up to NST_MAX_LEVELS = 8 and nst_job_set_taps a style_mask of up to six maps, and every
launcher is built for that: eight images in one conv launch (the tile_end prefix search of the h2, Winograd and bf16x3 batch
kernels), eight rows of the loss table, six style partials per level, a Gram batch that is cut after 16 / nstyle levels.  The
other oracle comparisons of the suite stop at three levels and five maps, where the Gram work is ONE batch and the prefix
search never goes past its third entry.  Here:

  1. jobs of 4, 5, 6 and 7 levels, the smallest that reach each depth, through hip_helpers.closure_vs_oracle_under_equal_decisions
     exactly as test_hip_parity.test_random_geometries_vs_oracle calls it (losses 1e-5, the whole gradient 2e-5 under the
     device's decisions, near-ties only, cap 1e-2 under each side's own decisions), on the default engine and - 4, 5 and 6
     levels - on the all-direct, banded per-level, bf16x3 and f32 per-level engines;
  2. eight levels, the cap, at 2048x2064 (a full oracle closure there is a minute and 10 GB of host memory) in pieces: loss-row
     identities, levels 2..7 against the oracle of exactly those levels (cpu_ref.closure_eval only_levels), additivity over the
     masks 0b00000011 + 0b11111100, the f32 per-level engine, the bf16x3 batch launches, idempotence; and what
     nst_job_configure refuses;
  3. all six style maps (two levels per Gram batch; conv4_2 a style map AND the content map) against the oracle with its
     STYLE_INDICES patched as tests/test_hip_taps.py patches them, with unequal layer weights against the restatement of
     tests/test_hip_style_blend.py;
  4. that the later Gram batches and the eight-image conv launches actually ran, read from the library's own launch record;
  5. the optimisers' loss rows on a five-level job, and level sharding of the eight-level job;
  6. a CPU guard on the geometry list.

Every tolerance is one the suite already holds the closure to (hip_helpers; test_full_size_job_properties;
test_level_sharded_closure_adds_up; test_adam_trajectory_vs_reference); none was chosen here."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import (BULK_RTOL, CW, GRAD_RTOL, NEAR_TIE, SW, TERMS, TVW, check_rows, closure_vs_oracle_under_equal_decisions, dev,
                         levels as _levels, masked_closure_vs_oracle_under_device_decisions, oracle_targets, rel_l2, report,
                         setup as _setup)

gpu = pytest.mark.gpu

SUM, STYLE, TV = TERMS[0], TERMS[2], TERMS[3]
# (h, w, levels, style h, style w) -> the loss terms the default engine is held on.  The smallest jobs that reach each depth
# with a lowest level of 16 .. 31 pixels; 1024x1040 and 2048x2064 add an odd tile column (1040 = 65 x 16) to the smallest size.
DEEP = {(136, 200, 4, 150, 180): TERMS,                    # 136x200, 68x100, 34x50, 17x25
        (264, 376, 5, 300, 280): TERMS,                    # ... 16x23; 99 264 pixels on top
        (512, 528, 6, 520, 560): (SUM, STYLE),             # ... 16x16: maps of 1x1 after the last pool
        (1024, 1040, 7, 1024, 1040): (SUM,)}               # two oracle evaluations, ~2.5 GB of activations to the host
EIGHT = (2048, 2064, 8, 2080, 2056)                        # 2048: the smallest size nst_job_configure admits at eight levels
SAME_SIZE_STYLE = {(1024, 1040, 7, 1024, 1040)}
GEOMETRIES = tuple(DEEP) + (EIGHT,)
SIX = (0, 1, 2, 3, 4, 5)
SIX_JOBS = {(68, 260, 3, 90, 140): TERMS,                  # two Gram batches, the second holding one level
            (136, 200, 4, 150, 180): (SUM, STYLE)}         # two full batches

# the other engines of the 4-, 5- and 6-level jobs; sum + TV as in test_random_geometries_vs_oracle (their TV signs are their
# own), the sum alone on six levels
DEFAULT = dict(conv_mode="f16x2", batched=True, h2_band_rows=0)
ENGINES = (("f32 per level", dict(conv_mode="f32", batched=False, h2_band_rows=0)),
           ("all direct", dict(conv_mode="f16x2", batched=True, h2_band_rows=0, h2_winograd=False)),
           ("16-row bands per level", dict(conv_mode="f16x2", batched=False, h2_band_rows=16)),
           ("bf16x3 batched", dict(conv_mode="bf16x3", batched=True)),      # (launch_conv_bf3_batch has its own prefix search)
           ("default", DEFAULT))

_JOBS = {}          # (geometry, oracle taps) -> (contents, styles, prepared x, oracle targets or None, {term: the oracle's own evaluation})


def _job(geo, weights, taps=None, targets=True):
    """The job of a geometry, made once.  taps: the oracle's (content index, style indices) its targets are made under (the
    caller has patched cpu_ref to them)."""
    if (geo, taps) not in _JOBS:
        h, w, nlev, hs, ws = geo
        c, s = _levels(h, w, nlev, 1), _levels(hs, ws, nlev, 2)
        xt = cpu_ref.prepare_img((0.7 * c[0] + 0.3 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32))
        _JOBS[(geo, taps)] = (c, s, xt, oracle_targets(c, s, weights) if targets else None, {})
    return _JOBS[(geo, taps)]


@pytest.fixture(scope="module", autouse=True)
def _release_jobs():
    """The shared jobs hold oracle targets and recorded pre-activations (gigabytes for the seven-level job): gone with the module."""
    yield
    _JOBS.clear()


def _engine(weights, **opts):
    from artstyletransfer_amd.engine import StyleEngine
    return StyleEngine(weights, 0, **opts)


def _report_losses(eng, xt, own, terms, what):
    """The loss errors the harness has just held to 1e-5 / 2e-5, written out: per term, total and worst level total against the
    oracle's own evaluation (`own`: the harness's cache)."""
    for name, (cw, sw, tvw) in terms:
        l = eng.closure(dev(xt), cw, sw, tvw)[1].cpu().numpy().astype(np.float64)
        loss, _, rows, _ = own[name]
        ref = np.array(rows)[:, 0]
        e_rows = float(np.max(np.abs(l[:-1].reshape(-1, 4)[:, 0] - ref) / np.abs(ref)))
        report(f"losses {what} [{name}]: total rel {abs(l[-1] - float(loss)) / abs(float(loss)):.2e}, worst level total rel {e_rows:.2e}")


def _launches(eng, x):
    """The launch record of one closure as the library reports it: (the records, Gram-class launch count)."""
    eng.set_timing(2)
    try:
        eng.closure(x, CW, SW, TVW)
        torch.cuda.synchronize()
        return eng.last_closure_launches(), eng.last_closure_class(1)[1]
    finally:
        eng.set_timing(0)


# ---- 6. the geometry list (CPU) -----------------------------------------------------------------------------------------------
def test_geometries_reach_every_depth_with_the_smallest_jobs():
    """CPU: the conditions the geometry list exists for - edits to it cannot thin it silently.  A job of each depth 4 .. 8;
    every lowest level 16 .. 31 on its shorter axis (one more level would be refused by nst_job_configure); a lowest level
    that is odd in each direction; the 4- and 5-level jobs at or below 100 000 pixels; styles of another size than the content
    (but for the seven-level job, whose style has the content's size) whose own lowest level nst_level_set_targets admits."""
    assert sorted(g[2] for g in GEOMETRIES) == [4, 5, 6, 7, 8]
    odd_h = odd_w = False
    for geo in GEOMETRIES:
        h, w, nlev, hs, ws = geo
        lh, lw = h >> (nlev - 1), w >> (nlev - 1)
        assert 16 <= min(lh, lw) <= 31, geo
        assert min(hs >> (nlev - 1), ws >> (nlev - 1)) >= 16, geo
        odd_h, odd_w = odd_h or lh % 2 == 1, odd_w or lw % 2 == 1
        if nlev <= 5:
            assert h * w <= 100_000, geo
        assert ((hs, ws) == (h, w)) == (geo in SAME_SIZE_STYLE), geo
    assert odd_h and odd_w
    assert EIGHT[0] >> 7 == 16 and (EIGHT[0] - 1) >> 7 < 16            # 2048 rows: the least that eight levels admit
    for geo in SIX_JOBS:
        assert min(geo[0] >> (geo[2] - 1), geo[1] >> (geo[2] - 1), geo[3] >> (geo[2] - 1), geo[4] >> (geo[2] - 1)) >= 16


# ---- 1. deep jobs against the oracle under equal decisions -----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("geo", list(DEEP), ids=[f"{g[0]}x{g[1]}x{g[2]}" for g in DEEP])
def test_deep_jobs_vs_oracle(vgg_weights, geo):
    """4 .. 7 levels, odd maps at the bottom, foreign-size styles: each engine against the oracle under equal decisions, called
    as test_random_geometries_vs_oracle calls the harness (cap 1e-2 under each side's own decisions: levels that are not
    exact halves turn flat regions into +-1 ulp noise whose signs the TV term takes).  4, 5 and 6 levels: five engines, the
    f16x2 / bf16x3 ones also against the f32 one (total 1e-5, level totals 2e-5).  7 levels: the default engine, two oracle
    evaluations; an indexing bug shows as errors of order 1."""
    h, w, nlev, hs, ws = geo
    c, s, xt, tg, own = _job(geo, vgg_weights)
    res = {}
    for name, opts in (ENGINES if nlev <= 6 else ENGINES[-1:]):
        e = _engine(vgg_weights, **opts)
        try:
            _setup(e, c, s)
            terms = DEEP[geo] if opts is DEFAULT else (SUM, TV) if nlev <= 5 else (SUM,)
            closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"deep {geo} {name}", terms=terms, cap=1e-2, own_cache=own)
            _report_losses(e, xt, own, terms, f"deep {geo} {name}")
            g, l = e.closure(dev(xt), CW, SW, TVW)
            res[name] = (g.cpu().numpy(), l.cpu().numpy())
        finally:
            e.close()
    assert np.isfinite(res["default"][0]).all()
    if nlev > 6:
        return
    g0, l0 = res["f32 per level"]
    for name, (g1, l1) in res.items():
        np.testing.assert_allclose(l1[-1], l0[-1], rtol=1e-5, err_msg=name)
        np.testing.assert_allclose(l1[:-1].reshape(nlev, 4)[:, 0], l0[:-1].reshape(nlev, 4)[:, 0], rtol=2e-5, err_msg=name)
        assert np.isfinite(g1).all(), name
    # the banded per-level launches compute what the batched launches of the same (direct) kernel compute
    np.testing.assert_allclose(res["16-row bands per level"][1], res["all direct"][1], rtol=1e-6)
    assert rel_l2(res["16-row bands per level"][0], res["all direct"][0]) < 1e-5


# ---- 2. eight levels ------------------------------------------------------------------------------------------------------------
class _Deep8:
    pass


@pytest.fixture(scope="module")
def deep8(vgg_weights):
    """The eight-level job on the default engine and ONE closure of it: the eight-image launches."""
    c, s, xt, _, _ = _job(EIGHT, vgg_weights, targets=False)
    d = _Deep8()
    d.c, d.s, d.xt, d.nlev = c, s, xt, EIGHT[2]
    d.eng = _engine(vgg_weights)
    try:
        _setup(d.eng, c, s)
        d.x = dev(xt)
        g, l = d.eng.closure(d.x, CW, SW, TVW)
        d.g0, d.l0 = g.clone(), l.clone()
        yield d
    finally:
        d.eng.close()


SHARE_UNITS = 10_000     # the smallest map on which one unit is no more than the 1e-4 share of test_full_size_job_properties
LOW6 = 0b11111100        # levels 2 .. 7: a six-image batch whose largest map is 512x516
TOP2 = 0b00000011


@gpu
def test_eight_levels_rows_additivity_idempotence(deep8):
    """(a) every row of the ONE closure obeys total = cw content + sw style + tvw tv (2e-6) and the grand total is the sum of the
    level totals (1e-6): the numbers of test_full_size_job_properties; (c) gradient and losses are the sums of those of the
    masks 0b00000011 and 0b11111100 (1e-6, as test_level_sharded_closure_adds_up); (e) a second evaluation is bitwise the
    first."""
    d = deep8
    n = d.nlev
    assert bool(torch.isfinite(d.g0).all()) and bool(torch.isfinite(d.l0).all())
    rows = d.l0[:-1].double().cpu().numpy().reshape(n, 4)
    assert (rows[:, 0] > 0).all() and (rows[:, 1:] > 0).all()
    np.testing.assert_allclose(rows[:, 0], CW * rows[:, 1] + SW * rows[:, 2] + TVW * rows[:, 3], rtol=2e-6)
    np.testing.assert_allclose(float(d.l0[-1]), rows[:, 0].sum(), rtol=1e-6)
    report("eight levels, level totals of one closure: " + np.array2string(rows[:, 0], precision=6))
    g_top, l_top = (t.clone() for t in d.eng.closure_levels(d.x, CW, SW, TVW, TOP2))
    g_low, l_low = d.eng.closure_levels(d.x, CW, SW, TVW, LOW6)
    add = float(((g_top.double() + g_low.double()) - d.g0.double()).norm() / d.g0.double().norm())
    report(f"eight levels: |g(0b00000011) + g(0b11111100) - g| / |g| = {add:.1e}")
    assert add < 1e-6
    np.testing.assert_allclose((l_top + l_low).cpu().numpy(), d.l0.cpu().numpy(), rtol=1e-6)
    assert not l_top[8:-1].cpu().numpy().any() and not l_low[:8].cpu().numpy().any()      # rows of foreign levels are zeros
    g1, l1 = d.eng.closure(d.x, CW, SW, TVW)
    assert torch.equal(g1, d.g0) and torch.equal(l1, d.l0)


@gpu
def test_eight_levels_low_six_vs_oracle(deep8, vgg_weights):
    """(b) nst_closure_levels of levels 2 .. 7 against the oracle of exactly those levels under the device's decisions, at the
    harness's tolerances; and the rows of those levels in the full closure are the rows of the masked one (1e-6)."""
    d = deep8
    own = range(2, d.nlev)
    tg = [cpu_ref.LevelTargets(cpu_ref.prepare_img(d.c[l]), cpu_ref.prepare_img(d.s[l]), vgg_weights) if l in own else None
          for l in range(d.nlev)]
    _, losses = masked_closure_vs_oracle_under_device_decisions(d.eng, d.xt, tg, vgg_weights, LOW6, f"eight levels {EIGHT}")
    np.testing.assert_allclose(d.l0.cpu().numpy()[8:-1], losses.cpu().numpy()[8:-1], rtol=1e-6)


@gpu
def test_eight_levels_vs_f32_per_level_engine(deep8, vgg_weights):
    """(d) the independent arithmetic on the per-level schedule: losses 1e-5, gradient within GRAD_RTOL, and the two engines'
    ReLU decisions differ only at near-ties, checked on the device per level and layer as test_full_size_job_properties does:
    the share of differing units of every (level, layer) below 1e-4, every differing unit within NEAR_TIE of zero.  A map of
    fewer than 10 000 units (the deep layers of the 64x64, 32x32 and 16x16 levels, down to the 512 units of conv5_1 at 16x16)
    cannot express a share of 1e-4 - one unit is more than that - so there the bound is the count it rounds to: at most one
    differing unit.  NEAR_TIE holds everywhere.  Every (level, layer) with a differing unit is reported with its counts."""
    d = deep8
    other = _engine(vgg_weights, conv_mode="f32", batched=False)
    try:
        assert other.conv_mode() == "f32"
        _setup(other, d.c, d.s)
        g2, l2 = other.closure(d.x, CW, SW, TVW)
        np.testing.assert_allclose(l2.cpu().numpy(), d.l0.cpu().numpy(), rtol=1e-5)
        e_modes = float((g2.double() - d.g0.double()).norm() / d.g0.double().norm())
        d.eng.closure(d.x, CW, SW, TVW)              # (the workspaces hold this pass again, whatever ran in between)
        worst, share, small_flips, differing = 0.0, 0.0, 0, []
        for lvl in range(d.nlev):
            for layer in range(13):
                a, b = d.eng.level_activation(lvl, layer), other.level_activation(lvl, layer)
                diff = (a > 0) != (b > 0)
                units = diff.numel()
                if bool(diff.any()):
                    rms = float(b.double().pow(2).mean().sqrt())
                    tie = float(torch.maximum(a, b)[diff].max()) / rms
                    flips = int(diff.sum())
                    worst = max(worst, tie)
                    differing.append(f"level {lvl} layer {layer}: {flips} of {units} units, largest value / rms {tie:.1e}")
                    if units >= SHARE_UNITS:
                        share = max(share, flips / units)
                    else:
                        small_flips = max(small_flips, flips)
                del a, b, diff
    finally:
        other.close()
    report(f"eight levels: f16x2 batched vs f32-MFMA per level, gradient rel-L2 {e_modes:.2e}; their ReLU decisions differ at up to "
           f"{share:.1e} of a layer's units (maps of >= {SHARE_UNITS} units) and at up to {small_flips} unit(s) of a smaller map, largest "
           f"value at such a unit / rms {worst:.1e}")
    for line in differing:
        report("eight levels, differing ReLU decisions, " + line)
    assert e_modes < GRAD_RTOL and share < 1e-4 and small_flips <= 1 and worst < NEAR_TIE


@gpu
def test_eight_levels_bf16x3_batch_launches(deep8, vgg_weights):
    """launch_conv_bf3_batch has a prefix search of its own, and no job of the suite hands it more than three images.  Six
    images: levels 2 .. 7 against the oracle of those levels, as (b).  Eight: losses within 1e-5 and the gradient within
    GRAD_RTOL of the default engine's (the numbers two arithmetics are held to on the full-size jobs), the two masks add
    up (1e-6), and the launch record holds 24 class-0 launches: the eight images went through one launch per layer."""
    d = deep8
    own = range(2, d.nlev)
    tg = [cpu_ref.LevelTargets(cpu_ref.prepare_img(d.c[l]), cpu_ref.prepare_img(d.s[l]), vgg_weights) if l in own else None
          for l in range(d.nlev)]
    e = _engine(vgg_weights, conv_mode="bf16x3", batched=True)
    try:
        assert e.conv_mode() == "bf16x3"
        _setup(e, d.c, d.s)
        g_low, l_low = (t.clone() for t in masked_closure_vs_oracle_under_device_decisions(e, d.xt, tg, vgg_weights, LOW6,
                                                                                            f"eight levels {EIGHT} bf16x3 batched"))
        g_top, l_top = (t.clone() for t in e.closure_levels(d.x, CW, SW, TVW, TOP2))
        g, l = e.closure(d.x, CW, SW, TVW)
        add = float(((g_top.double() + g_low.double()) - g.double()).norm() / g.double().norm())
        e_modes = float((g.double() - d.g0.double()).norm() / d.g0.double().norm())
        report(f"eight levels, bf16x3 batched: gradient rel-L2 to the default engine's {e_modes:.2e}; |g(0b00000011) + g(0b11111100) - g| / |g| = {add:.1e}")
        np.testing.assert_allclose(l.cpu().numpy(), d.l0.cpu().numpy(), rtol=1e-5)
        np.testing.assert_allclose((l_top + l_low).cpu().numpy(), l.cpu().numpy(), rtol=1e-6)
        assert add < 1e-6 and e_modes < GRAD_RTOL
        rec, _ = _launches(e, d.x)
        assert sum(r["cls"] == 0 for r in rec) == 24          # one launch per layer for the eight images here too
    finally:
        e.close()


@gpu
def test_configure_refusals_leave_the_engine_usable(vgg_weights):
    """Nine levels, and eight levels one pixel short in either direction, are refused with nst_job_configure's messages; the
    engine then evaluates a valid job to the bits of a fresh engine."""
    from artstyletransfer_amd._lib import NstError
    geo = next(iter(DEEP))
    c, s, xt, _, _ = _job(geo, vgg_weights)
    out = []
    for refused in (True, False):
        e = _engine(vgg_weights)
        try:
            if refused:
                _setup(e, c, s)
                with pytest.raises(NstError, match="levels_num out of range"):
                    e.configure(9, 4096, 4096)
                for hw in ((2047, 2048), (2048, 2047)):
                    with pytest.raises(NstError, match="coarsest pyramid level must be at least 16x16"):
                        e.configure(8, *hw)
                assert e.levels == geo[2] and e.shape == geo[:2]
            _setup(e, c, s)
            g, l = e.closure(dev(xt), CW, SW, TVW)
            out.append((g.clone(), l.clone()))
        finally:
            e.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][0].abs().max()) > 0


# ---- 3. six style maps -----------------------------------------------------------------------------------------------------------
def _setup_six(e, c, s, content=4):
    e.configure(len(c), *c[0].shape[:2])
    e.set_taps(content, list(SIX))
    for i in range(len(c)):
        e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))


@gpu
@pytest.mark.parametrize("geo", list(SIX_JOBS), ids=[f"{g[0]}x{g[1]}x{g[2]}" for g in SIX_JOBS])
def test_six_style_maps_vs_oracle(vgg_weights, monkeypatch, geo):
    """style_mask 0x3F: two levels per Gram batch, style_c / style_w / style_partial filled to the end, conv4_2 both the content
    map and a style map below the top of the chain.  The batched and the per-level engine against the oracle with its style
    indices set to the six maps, under equal decisions."""
    monkeypatch.setattr(cpu_ref, "STYLE_INDICES", SIX)
    c, s, xt, tg, own = _job(geo, vgg_weights, taps=(4, SIX))
    for opts in (dict(), dict(batched=False)):
        e = _engine(vgg_weights, **opts)
        try:
            _setup_six(e, c, s)
            closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"six maps {geo} {opts}", terms=SIX_JOBS[geo], cap=1e-2,
                                                    own_cache=own)
            _report_losses(e, xt, own, SIX_JOBS[geo], f"six maps {geo} {opts}")
        finally:
            e.close()


@gpu
def test_six_style_maps_with_a_content_map_below_the_top(vgg_weights, monkeypatch):
    """content = 2 (relu3_1) under the six style maps: content gradient and Gram backward meet at a layer far below the top."""
    geo = next(iter(SIX_JOBS))
    monkeypatch.setattr(cpu_ref, "STYLE_INDICES", SIX)
    monkeypatch.setattr(cpu_ref, "CONTENT_INDEX", 2)
    c, s, xt, tg, own = _job(geo, vgg_weights, taps=(2, SIX))
    e = _engine(vgg_weights)
    try:
        _setup_six(e, c, s, content=2)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"six maps, content 2, {geo}", cap=1e-2, own_cache=own)
        _report_losses(e, xt, own, TERMS, f"six maps, content 2, {geo}")
    finally:
        e.close()


W_SIX = (1.0, 0.5, 0.75, 2.0, 1.5, 0.25)          # the last weight is no other's: a weight read one slot off shows


@gpu
def test_six_style_maps_with_unequal_layer_weights(vgg_weights):
    """nst_job_set_style_weights over all six maps against the restatement of the weighted style term
    (tests/test_hip_style_blend.py: style = (sum_i w_i MSE_i) / nstyle) under the device's decisions, at the harness's
    tolerances (total 1e-5, rows 2e-5, the whole gradient 2e-5), for the style term alone and the weighted sum."""
    import test_hip_style_blend as blend
    geo = next(iter(SIX_JOBS))
    taps = (4, SIX)
    c, s, xt, _, _ = _job(geo, vgg_weights, targets=False)
    nlev = geo[2]
    tg = [blend.restated_targets(cpu_ref.prepare_img(c[l]), [cpu_ref.prepare_img(s[l])], [blend.ONES], vgg_weights, taps)
          for l in range(nlev)]
    assert len(set(W_SIX)) == 6
    e = _engine(vgg_weights)
    try:
        _setup_six(e, c, s)
        e.set_style_weights(W_SIX)
        assert e.style_weights() == W_SIX
        xd = dev(xt)
        for name, (cw, sw, tvw) in (STYLE, SUM):
            grad, losses = e.closure(xd, cw, sw, tvw)
            dec = blend.device_decisions(e, xd, vgg_weights, taps)
            loss, g_ref, rows = blend.restated_closure(xt, tg, vgg_weights, cw, sw, tvw, W_SIX, taps, dec)
            losses = losses.cpu().numpy()
            e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
            e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
            report(f"six maps, layer weights {W_SIX}, {geo} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}")
            assert e_l < 1e-5, (name, e_l)
            check_rows(losses[:-1].reshape(nlev, 4), np.array(rows), 2e-5, cw, sw, tvw)
            assert e_g < BULK_RTOL, (name, e_g)
    finally:
        e.close()


@gpu
def test_six_maps_then_default_taps_are_bitwise_the_default(vgg_weights):
    """An engine that set the six maps and then the default taps back computes the bits of one that never changed them."""
    geo = next(iter(SIX_JOBS))
    c, s, xt, _, _ = _job(geo, vgg_weights, targets=False)
    out = []
    for changed in (False, True):
        e = _engine(vgg_weights)
        try:
            if changed:
                _setup_six(e, c, s)
                e.closure(dev(xt), CW, SW, TVW)
                e.set_taps(4, [0, 1, 2, 3, 5])
            _setup(e, c, s)
            g, l = e.closure(dev(xt), CW, SW, TVW)
            out.append((g.clone(), l.clone()))
        finally:
            e.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 4. the later batches actually ran ------------------------------------------------------------------------------------------
@gpu
def test_launch_record_of_deep_and_six_map_closures(deep8, vgg_weights):
    """From the library's own launch record (set_timing(2); its event pool holds 1024 launches, an eight-level closure takes
    a fraction of that): the eight-level default closure has 24 class-0 launches - one per layer for all eight images, no
    per-level fallback - each reporting the top level's map; its Gram-class launch count exceeds that of a three-level job of
    default taps on the same engine, and that of six maps x three levels exceeds five maps x three levels."""
    from artstyletransfer_amd.engine import StyleEngine
    d = deep8
    geo3 = next(iter(SIX_JOBS))
    c3, s3, xt3, _, _ = _job(geo3, vgg_weights, targets=False)
    e = _engine(vgg_weights)
    try:
        _setup(e, c3, s3)
        _, gram_five_3 = _launches(e, dev(xt3))
        _setup_six(e, c3, s3)
        _, gram_six_3 = _launches(e, dev(xt3))
        e.set_taps(4, [0, 1, 2, 3, 5])
        _setup(e, d.c, d.s)
        rec, gram_five_8 = _launches(e, d.x)
    finally:
        e.close()
    conv = [r for r in rec if r["cls"] == 0]
    report(f"launch record: eight levels x five maps {len(rec)} launches, {len(conv)} of class 0, {gram_five_8} of the Gram class; "
           f"three levels x five maps {gram_five_3} of the Gram class, three levels x six maps {gram_six_3}")
    assert len(conv) == 24
    assert sorted(r["layer"] for r in conv) == sorted(list(range(1, 13)) + [-l for l in range(1, 13)])
    h0, w0 = EIGHT[:2]
    for r in conv:
        sc = StyleEngine.LAYER_SCALE[abs(r["layer"])]
        assert (r["h"], r["w"]) == (h0 >> sc, w0 >> sc), r
    assert gram_five_8 > gram_five_3 > 0
    assert gram_six_3 > gram_five_3


# ---- 5. the optimiser's rows on a deep job, level sharding -------------------------------------------------------------------------
FIVE = (264, 376, 5, 300, 280)


@gpu
def test_lbfgs_rows_on_a_five_level_job(vgg_weights):
    """Three L-BFGS steps (max_eval 26, lr 1) on the five-level job: every returned row has 4 * 5 + 1 entries whose last is the
    sum of the five level totals (1e-6), and the row of each step's first closure is, bitwise, what the closure returns at the
    image the step started from."""
    from artstyletransfer_amd.engine import PixelOptimizer
    c, s, xt, _, _ = _job(FIVE, vgg_weights)
    e = _engine(vgg_weights)
    try:
        _setup(e, c, s)
        x = dev(xt).clone()
        opt = PixelOptimizer(e, "lbfgs", 1.0, 26)
        starts, firsts, counts = [], [], []
        try:
            for _ in range(3):
                starts.append(x.clone())
                info, r = opt.step(x, CW, SW, TVW)
                assert r.shape == (info.closures, 4 * 5 + 1) and info.closures >= 1
                assert np.isfinite(r).all()
                np.testing.assert_allclose(r[:, -1], r[:, :-1].reshape(-1, 5, 4)[:, :, 0].astype(np.float64).sum(axis=1), rtol=1e-6)
                firsts.append(r[0].copy())
                counts.append(int(info.closures))
        finally:
            opt.close()
        report(f"L-BFGS (max_eval 26) on {FIVE}: closures per step {counts}, first-closure totals {[float(f[-1]) for f in firsts]}")
        assert firsts[2][-1] < firsts[0][-1]                            # the steps were taken
        for k, (x0, first) in enumerate(zip(starts, firsts)):
            _, l = e.closure(x0, CW, SW, TVW)
            assert np.array_equal(l.cpu().numpy(), first), k
    finally:
        e.close()


@gpu
def test_adam_rows_on_a_five_level_job_vs_reference_loop(vgg_weights):
    """Four Adam steps on the five-level job against cpu_ref.run_process on the same job: the first closure's rows to 2e-5, the
    free-running later ones to 1e-2 (the bounds of test_adam_trajectory_vs_reference)."""
    from artstyletransfer_amd.engine import PixelOptimizer
    c, s, _, _, _ = _job(FIVE, vgg_weights)
    start = (0.7 * c[0] + 0.3 * cpu_ref.synthetic_image(FIVE[0], FIVE[1], seed=9)).astype(np.float32)
    rec = []
    for _ in cpu_ref.run_process(c, s, start, vgg_weights, "adam", 4, record=rec):
        pass
    ref = np.array([r["rows"] for r in rec])
    assert ref.shape == (4, 5, 4)
    e = _engine(vgg_weights)
    try:
        _setup(e, c, s)
        x = dev(cpu_ref.prepare_img(start))
        opt = PixelOptimizer(e, "adam")
        rows = []
        try:
            for k in range(4):
                info, r = opt.step(x, CW, SW, TVW)
                assert info.closures == 1 and r.shape == (1, 4 * 5 + 1)
                np.testing.assert_allclose(r[0, -1], r[0, :-1].reshape(5, 4)[:, 0].astype(np.float64).sum(), rtol=1e-6)
                rows.append(r[0, :-1].reshape(5, 4))
        finally:
            opt.close()
    finally:
        e.close()
    rows = np.array(rows)
    err = np.abs(rows[:, :, 0] - ref[:, :, 0]) / ref[:, :, 0]
    report(f"Adam on {FIVE}, four steps free-running: level-total rel err per step " + np.array2string(err.max(axis=1), precision=1))
    check_rows(rows[:1], ref[:1], 2e-5)
    check_rows(rows, ref, 1e-2)


@gpu
def test_eight_levels_sharded_over_four_ranks_add_up(deep8):
    """One nst_closure_levels pass per rank of sharding.level_mask(8, r, 4): every level is owned exactly once and gradients
    and loss vectors add up to the full closure (1e-6)."""
    from artstyletransfer_amd import sharding
    d = deep8
    world = 4
    owned = [list(sharding.owned_levels(d.nlev, r, world)) for r in range(world)]
    assert sorted(l for o in owned for l in o) == list(range(d.nlev)) and owned[0] == [0]
    g_sum = torch.zeros_like(d.g0, dtype=torch.float64)
    l_sum = torch.zeros_like(d.l0)
    for r in range(world):
        mask = sharding.level_mask(d.nlev, r, world)
        assert mask == sum(1 << l for l in owned[r])
        g, l = d.eng.closure_levels(d.x, CW, SW, TVW, mask)
        rows = l[:-1].cpu().numpy().reshape(d.nlev, 4)
        assert all(rows[k].any() == (k in owned[r]) for k in range(d.nlev)), (r, owned[r])
        g_sum += g.double()
        l_sum += l
    add = float((g_sum - d.g0.double()).norm() / d.g0.double().norm())
    report(f"eight levels over four ranks {owned}: |sum of the ranks' gradients - g| / |g| = {add:.1e}")
    assert add < 1e-6
    np.testing.assert_allclose(l_sum.cpu().numpy(), d.l0.cpu().numpy(), rtol=1e-6)
