"""GPU: every size-selected tile shape of the f16x2 direct convolution (conv_h2.hip) against the CPU oracle on jobs with edge tiles.

conv_h2.hip picks the workgroup tile of a 128-channel-tile launch from the size of the job (h2_launch_shape): 4-row tiles for
small jobs, 8-row tiles in between, 16-row tiles from about half a megapixel up.  Every other oracle comparison of the suite
runs on jobs small enough for the 4-row (sometimes the 8-row) shape; the 16-row shape a photograph runs on was compared only
with itself.  nst_options.h2_tile_rows forces a shape onto any job, so here each shape is forced onto small odd geometries -
partial last tiles in both directions, maps smaller than one tile, odd pooling sources - and held to the oracle like every other
schedule: hip_helpers.closure_vs_oracle_under_equal_decisions at the project's tolerances (losses 1e-5, the whole gradient 2e-5
under the device's decisions, decisions differing at near-ties only).

That the forced shape actually ran is read from the launch record the launcher itself fills (nst_last_closure_launches), not
from a restatement of its rule: a forced option that a launcher ignored would otherwise pass everything here."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import (CW, SW, TERMS, TVW, closure_vs_oracle_under_equal_decisions, dev, levels as _levels, oracle_targets, report,
                         setup as _setup)

# (h, w, levels, style h, style w): at most ~100k pixels on the top level, a style of another size
GEOMETRIES = ((68, 260, 3, 90, 140), (124, 252, 2, 100, 200), (230, 318, 2, 150, 210))


# ---- which partial tiles a geometry has (pure Python) --------------------------------------------------------------------------
def level_maps(h, w, nlev):
    """(level, k, rows, cols) of the feature maps at 1/2^k, k = 0 ... 4, of every pyramid level: floor halving, as the pyramid
    and the four pools do.  k = 0 is the level image's own size (the 64-channel layers)."""
    out = []
    for l in range(nlev):
        for k in range(5):
            out.append((l, k, (h >> l) >> k, (w >> l) >> k))
    return out


def geometry_residues(h, w, nlev):
    """What the wide launches of a job see at their edges.  Over the maps at 1/2, 1/4, 1/8 and 1/16 of every level: the row and
    column counts modulo 16 (a 16-column tile; 4-, 8- or 16-row tiles all divide 16) and the smallest row count; over the pools
    whose epilogue and un-pooling loader run in the wide launches (the sources at 1/4 and 1/8): whether a source has an odd
    height / an odd width (its last row / column belongs to no window)."""
    maps = [m for m in level_maps(h, w, nlev) if m[1] >= 1]
    src = [m for m in level_maps(h, w, nlev) if m[1] in (2, 3)]
    return {"rows_mod16": {m[2] % 16 for m in maps}, "cols_mod16": {m[3] % 16 for m in maps},
            "min_rows": min(m[2] for m in maps), "min_cols": min(m[3] for m in maps),
            "odd_source_rows": any(m[2] % 2 for m in src), "odd_source_cols": any(m[3] % 2 for m in src)}


def test_geometries_cover_every_kind_of_partial_tile():
    """CPU: the conditions the geometry list exists for - edits to it cannot thin it silently.  Over all geometries: rows
    modulo 16 include 1, 15 and a value in 7..9; columns modulo 16 include 1 and 15; a map has fewer than 16 rows and one fewer
    than 4; a pool has an odd source height and one an odd source width; every job stays at or below ~100k pixels with 2-3
    levels, a lowest level of at least 16 x 16 (nst_job_configure's minimum) and a style of another size."""
    rows, cols = set(), set()
    least, odd_r, odd_c = 1 << 30, False, False
    for h, w, nlev, hs, ws in GEOMETRIES:
        r = geometry_residues(h, w, nlev)
        rows |= r["rows_mod16"]
        cols |= r["cols_mod16"]
        least = min(least, r["min_rows"])
        odd_r, odd_c = odd_r or r["odd_source_rows"], odd_c or r["odd_source_cols"]
        assert h * w <= 100_000 and nlev in (2, 3) and (hs, ws) != (h, w)
        assert min(h >> (nlev - 1), w >> (nlev - 1), hs >> (nlev - 1), ws >> (nlev - 1)) >= 16
        assert r["min_rows"] >= 1 and r["min_cols"] >= 1
    assert {1, 15} <= rows and rows & {7, 8, 9}, sorted(rows)
    assert {1, 15} <= cols, sorted(cols)
    assert least < 4                        # (and with it a map of fewer than 16 rows)
    assert any(4 <= m[2] < 16 for g in GEOMETRIES for m in level_maps(*g[:3]) if m[1] >= 1)
    assert odd_r and odd_c
    # the helper itself, on the two maps the list was started from
    assert (0, 2, 17, 65) in level_maps(68, 260, 3) and (0, 2, 31, 63) in level_maps(124, 252, 2)
    assert geometry_residues(64, 128, 1) == {"rows_mod16": {0, 8, 4}, "cols_mod16": {0, 8}, "min_rows": 4, "min_cols": 8,
                                             "odd_source_rows": False, "odd_source_cols": False}


# ---- the shapes -------------------------------------------------------------------------------------------------------------------
DIRECT = dict(h2_winograd=False)
# name -> (StyleEngine options, loss terms).  "direct": every convolution is a conv_h2 launch, so the option reaches forward,
# input-gradient, second-source and un-pooling launches; without it (the Winograd default) it reaches the launches that carry a
# Gram source.  The experiment shapes (wg256, the other MFMA form) are run both ways: as the options stand alone, and direct,
# where alone they would never meet an un-pooling or a forward launch.
SUM_STYLE = (TERMS[0], TERMS[2])
SHAPES = {
    "rows4-direct": (dict(h2_tile_rows=4, **DIRECT), SUM_STYLE),
    "rows4": (dict(h2_tile_rows=4), SUM_STYLE),
    "rows8-direct": (dict(h2_tile_rows=8, **DIRECT), SUM_STYLE),
    "rows8": (dict(h2_tile_rows=8), SUM_STYLE),
    "rows16-direct": (dict(h2_tile_rows=16, **DIRECT), TERMS),
    "rows16": (dict(h2_tile_rows=16), TERMS),
    "rows16-wg256": (dict(h2_tile_rows=16, h2_wg256=True), SUM_STYLE),
    "rows16-wg256-direct": (dict(h2_tile_rows=16, h2_wg256=True, **DIRECT), SUM_STYLE),
    "rows16-mfma16x16": (dict(h2_tile_rows=16, h2_mfma16=2), SUM_STYLE),
    "rows16-mfma16x16-direct": (dict(h2_tile_rows=16, h2_mfma16=2, **DIRECT), SUM_STYLE),
    "rows4-mfma16x16": (dict(h2_tile_rows=4, h2_mfma16=3), SUM_STYLE),
    "rows4-mfma16x16-direct": (dict(h2_tile_rows=4, h2_mfma16=3, **DIRECT), SUM_STYLE),
    "rows8-mfma32x32": (dict(h2_tile_rows=8, h2_mfma16=0), SUM_STYLE),
    "rows8-mfma32x32-direct": (dict(h2_tile_rows=8, h2_mfma16=0, **DIRECT), SUM_STYLE),
    "rows16-per-level": (dict(batched=False, h2_tile_rows=16), SUM_STYLE),
    "rows16-bands16": (dict(batched=False, h2_tile_rows=16, h2_band_rows=16), SUM_STYLE),
    "rows16-bands32": (dict(batched=False, h2_tile_rows=16, h2_band_rows=32), SUM_STYLE),
}

_JOBS = {}          # geometry (+ network) -> (contents, styles, x, oracle targets, the oracle's own-decision evaluations per term)


def _job(geo, weights, key=None):
    if (geo, key) not in _JOBS:
        h, w, nlev, hs, ws = geo
        c, s = _levels(h, w, nlev, 1), _levels(hs, ws, nlev, 2)
        xt = cpu_ref.prepare_img((0.7 * c[0] + 0.3 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32))
        _JOBS[(geo, key)] = (c, s, xt, oracle_targets(c, s, weights), {})
    return _JOBS[(geo, key)]


def _forcible(launches):
    """The launches nst_options.h2_tile_rows applies to, by what the launcher reported: 128-channel tiles, 32-channel chunks."""
    return [r for r in launches if r["h2_rows"] > 0 and r["h2_bn"] == 128 and r["h2_chunk"] == 32]


def _kinds(recs):
    return {"forward": sum(r["layer"] > 0 for r in recs), "input-gradient": sum(r["layer"] < 0 for r in recs),
            "second-source": sum(r["h2_second"] for r in recs), "un-pooling": sum(r["h2_unpool"] for r in recs)}


def _launch_record(eng, x):
    eng.set_timing(2)
    try:
        eng.closure(x, CW, SW, TVW)
        torch.cuda.synchronize()
        return eng.last_closure_launches()
    finally:
        eng.set_timing(0)


def _assert_forced_shape_ran(eng, x, opts, what, top_rows):
    """From the launch record: every launch the option applies to ran at opts['h2_tile_rows'] rows, in the workgroup / MFMA form
    the options name, and - direct and batched - each of the four launch kinds is among them."""
    rows = opts["h2_tile_rows"]
    launches = _launch_record(eng, x)
    recs = _forcible(launches)
    kinds = _kinds(recs)
    report(f"shape record {what}: {len(recs)} of {len(launches)} launches are 128-channel x 32-chunk conv_h2 launches, rows "
           f"{sorted({r['h2_rows'] for r in recs})}, 32-channel tiles per wave {sorted({r['h2_ntw'] for r in recs})}, 16x16x32 form "
           f"on {sum(r['h2_mfma16'] for r in recs)}, kinds {kinds}, most bands {max(r['h2_bands'] for r in recs)}")
    assert recs and all(r["h2_rows"] == rows for r in recs), (what, recs)
    batched, direct = opts.get("batched", True), opts.get("h2_winograd", True) is False
    assert kinds["second-source"] >= 1
    if direct or not batched:                    # (the per-level launches are all direct)
        assert kinds["forward"] >= 1 and kinds["input-gradient"] >= 1, (what, kinds)
    if direct and batched:
        assert kinds["un-pooling"] >= 1, (what, kinds)
    if not batched:                              # the per-level walker un-pools in a kernel of its own
        assert kinds["un-pooling"] == 0 and all(r["h2_persist"] == 0 for r in recs)
    want_ntw = 1 if rows < 16 else (4 if opts.get("h2_wg256") else 2)
    assert all(r["h2_ntw"] == want_ntw for r in recs), (what, want_ntw)
    m16 = opts.get("h2_mfma16", 1)
    for r in recs:
        if opts.get("h2_wg256") or m16 == 0:
            want = 0
        elif m16 == 3:
            want = 1                             # also on the un-pooling launches
        elif m16 == 2:
            want = int(rows == 8 or (rows == 16 and not r["h2_unpool"]))
        else:
            want = int(rows == 8)
        assert r["h2_mfma16"] == want, (what, r)
    band = opts.get("h2_band_rows", 0)
    top = [r for r in recs if r["h"] == top_rows]          # the launches on the largest 256-channel map
    if band:
        assert top and all(r["h2_bands"] == -(-top_rows // band) for r in top), (what, band, top)
    else:
        assert all(r["h2_bands"] == 1 for r in recs)


@pytest.mark.gpu
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}L{g[2]}")
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forced_tile_shape_vs_oracle(vgg_weights, shape, geo):
    """One forced shape on one geometry against the oracle under equal decisions (losses 1e-5, whole gradient 2e-5, near-tie
    limits, cap 1e-2 on the comparison under each side's own decisions as in test_random_geometries_vs_oracle), on the weighted
    sum and the style term - the term that drives the second K source; the plain 16-row shape on every term alone.  Then the
    launch record: the shape ran."""
    from artstyletransfer_amd.engine import StyleEngine
    opts, terms = SHAPES[shape]
    c, s, xt, tg, own = _job(geo, vgg_weights)
    e = StyleEngine(vgg_weights, 0, **opts)
    try:
        _setup(e, c, s)
        what = f"{shape} {geo[0]}x{geo[1]} L{geo[2] - 1}"
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "tile shape " + what, terms=terms, cap=1e-2, own_cache=own)
        _assert_forced_shape_ran(e, dev(xt), opts, what, geo[0] >> 2)
    finally:
        e.close()


@pytest.mark.gpu
def test_forced_16_row_shape_with_average_pooling_vs_oracle(vgg_weights, monkeypatch):
    """pooling="avg" on the 16-row shape, every convolution direct: the average-pool epilogue and the multi-hot code of the
    un-pooling loader at partial tiles and odd pooling sources (124x252: 31x63 and 15x31), against the oracle with the
    average-pool network of tests/test_hip_pooling.py."""
    from artstyletransfer_amd.engine import StyleEngine
    from test_hip_pooling import avg_vgg19_features
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    geo = GEOMETRIES[1]
    c, s, xt, tg, own = _job(geo, vgg_weights, "avg")         # (targets and own-decision evaluations of the OTHER network)
    opts = dict(h2_tile_rows=16, **DIRECT)
    e = StyleEngine(vgg_weights, 0, **opts)
    try:
        e.configure(geo[2], geo[0], geo[1])
        e.set_pooling("avg")
        for i in range(geo[2]):
            e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
        what = f"rows16-direct avg-pool {geo[0]}x{geo[1]} L{geo[2] - 1}"
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "tile shape " + what, terms=SUM_STYLE, cap=1e-2, own_cache=own)
        _assert_forced_shape_ran(e, dev(xt), opts, what, geo[0] >> 2)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}L{g[2]}")
def test_unforced_small_jobs_run_4_rows_and_forcing_4_is_bitwise(vgg_weights, geo):
    """h2_tile_rows = 0 on these jobs: the record shows every launch the option applies to at 4 rows, all four kinds among them
    (every convolution direct).  Forcing the shape the rule picks anyway changes nothing: gradient and loss rows bitwise."""
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt, _, _ = _job(geo, vgg_weights)
    x = dev(xt)
    out = []
    for opts in (dict(**DIRECT), dict(h2_tile_rows=4, **DIRECT)):
        e = StyleEngine(vgg_weights, 0, **opts)
        try:
            _setup(e, c, s)
            g, l = e.closure(x, CW, SW, TVW)
            out.append((g.cpu().numpy().copy(), l.cpu().numpy().copy()))
            recs = _forcible(_launch_record(e, x))
            assert recs and all(r["h2_rows"] == 4 and r["h2_ntw"] == 1 and r["h2_mfma16"] == 0 for r in recs), recs
            assert all(n >= 1 for n in _kinds(recs).values()), _kinds(recs)
        finally:
            e.close()
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0]).max() > 0
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_launch_record_names_the_other_shapes_too(vgg_weights):
    """The record on the default engine (Winograd launches on): the short-K launches (Cin <= 128) keep their <8, 128, 2, 16>
    shape and the 64-channel layers their <16, 64, 2, 16> whatever h2_tile_rows says, the Winograd launches report no conv_h2
    shape, and without timing there is no record."""
    from artstyletransfer_amd.engine import StyleEngine
    geo = GEOMETRIES[0]
    c, s, xt, _, _ = _job(geo, vgg_weights)
    e = StyleEngine(vgg_weights, 0, h2_tile_rows=16)
    try:
        _setup(e, c, s)
        e.closure(dev(xt), CW, SW, TVW)
        assert e.last_closure_launches() == []
        launches = _launch_record(e, dev(xt))
        conv = [r for r in launches if r["cls"] == 0]
        assert len(conv) == 24
        shapes = {(r["h2_rows"], r["h2_bn"], r["h2_ntw"], r["h2_chunk"]) for r in conv}
        assert shapes == {(0, 0, 0, 0), (16, 128, 2, 32), (8, 128, 2, 16), (16, 64, 2, 16)}, shapes
        assert sum(r["h2_rows"] == 0 for r in conv) == 15                     # the Winograd launches
        for r in conv:
            if r["h2_rows"] and r["cin"] <= 128:
                assert r["h2_chunk"] == 16, r
        assert all(r["h2_rows"] == 0 for r in launches if r["cls"] in (2, 3))
    finally:
        e.close()


# ---- the f32 / bf16x3 launches that do not split K ----------------------------------------------------------------------------
UNSPLIT_GEO = (256, 384, 1, 200, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_unsplit_f32_and_bf16x3_launches_vs_oracle(vgg_weights, mode):
    """conv_mfma.hip splits K only on launches of fewer than 384 blocks (conv_ksplit), and conv_bf3.hip's cost rule stops
    splitting where a launch fills the chip; the other oracle-held f32 / bf16x3 jobs stay below that on the full-resolution
    layers.  256x384 on one level: 16 x 24 = 384 blocks there, the unsplit path - against the oracle on the weighted sum (one
    own-decision evaluation for both modes)."""
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt, tg, own = _job(UNSPLIT_GEO, vgg_weights)
    e = StyleEngine(vgg_weights, 0, conv_mode=mode)
    try:
        assert e.conv_mode() == mode
        _setup(e, c, s)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"unsplit {mode} 256x384 L0", terms=TERMS[:1], cap=1e-2,
                                                own_cache=own)
    finally:
        e.close()
