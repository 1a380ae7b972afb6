"""GPU: a per-level closure run in row bands returns the bits of the same closure run whole.

conv_h2.hip promises that the arithmetic of a tile does not depend on how it was reached.  The per-level launcher reaches a tile
of a banded launch through a one-image batch whose first tile row is not 0 and whose tensor pointers are moved to the band's
first row minus a 16-row halo: here nst_options.h2_band_rows forces 16- and 32-row bands onto a small job, and loss rows and
gradient are held bit for bit to the unbanded closure of the same engine options.

70x52 on two levels: 70 rows are five 16-row bands with a ragged last one on the 64-channel layers, 35 rows three and 17 rows
two; 52 columns leave a partial tile column; the pool sources of 35 and 17 rows lose their last row.  Tile heights 4, 8 and 16
put a band's first tile row (after the 16-row halo) at 4, 2 and 1; the 16x16x32 MFMA form rides on the 4- and 16-row shapes;
every case under max and under average pooling.

That the bands ran is read from the launch record (nst_last_closure_launches): an ignored hook would otherwise pass."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels as _levels

H, W, NLEV, HS, WS = 70, 52, 2, 48, 80
BANDS = (0, 16, 32)
SHAPES = {
    "rows4": dict(h2_tile_rows=4),
    "rows8": dict(h2_tile_rows=8),
    "rows16": dict(h2_tile_rows=16),
    "rows4-mfma16x16": dict(h2_tile_rows=4, h2_mfma16=3),
    "rows16-mfma16x16": dict(h2_tile_rows=16, h2_mfma16=2),
}

_JOB = []


def _job():
    if not _JOB:
        c, s = _levels(H, W, NLEV, 1), _levels(HS, WS, NLEV, 2)
        xt = cpu_ref.prepare_img((0.7 * c[0] + 0.3 * cpu_ref.synthetic_image(H, W, seed=9)).astype(np.float32))
        _JOB.append((c, s, xt))
    return _JOB[0]


def _closure(weights, opts, pooling, band):
    """(gradient, loss rows, launch record) of one timed closure of a fresh engine."""
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt = _job()
    e = StyleEngine(weights, 0, batched=False, h2_band_rows=band, **opts)
    try:
        e.configure(NLEV, H, W)
        e.set_pooling(pooling)
        for i in range(NLEV):
            e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
        e.set_timing(2)
        g, l = e.closure(dev(xt), CW, SW, TVW)
        torch.cuda.synchronize()
        return g.clone(), l.clone(), e.last_closure_launches()
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pooling", ["max", "avg"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_banded_per_level_closure_is_bitwise_the_unbanded_one(vgg_weights, shape, pooling):
    runs = {band: _closure(vgg_weights, SHAPES[shape], pooling, band) for band in BANDS}
    g0, l0, rec0 = runs[0]
    assert torch.isfinite(g0).all() and float(g0.abs().max()) > 0 and torch.isfinite(l0).all()
    assert rec0 and all(r["h2_bands"] == 1 for r in rec0 if r["h2_rows"] > 0)
    for band in BANDS[1:]:
        g, l, rec = runs[band]
        # the 64-channel launches on the level-0 image: 70 rows in bands of `band`
        top = [r for r in rec if r["h2_rows"] > 0 and r["h2_bn"] == 64 and r["h"] == H]
        assert top and all(r["h2_bands"] == -(-H // band) and r["h2_bands"] > 1 for r in top), (band, top)
        # ... and the forced tile height on the wide launches that take it
        wide = [r for r in rec if r["h2_rows"] > 0 and r["h2_bn"] == 128 and r["h2_chunk"] == 32]
        assert wide and all(r["h2_rows"] == SHAPES[shape]["h2_tile_rows"] for r in wide), (band, wide)
        if band == 16:      # (their largest map has 17 rows: two 16-row bands, one 32-row band)
            assert any(r["h2_bands"] == 2 for r in wide), (band, wide)
        assert torch.equal(l, l0), (shape, pooling, band, l, l0)
        assert torch.equal(g, g0), (shape, pooling, band, int((g != g0).sum()))
