"""GPU: the short-K forward launches with weight fragments from L2 (nst_ctx_set_h2_direct_weights, on by default) against
their switch-off twin in the same build.

conv1_2 runs on conv_h2_batch_kernel<16, 64, 2, 16> and conv2_1, conv2_2, conv3_1 on <8, 128, 2, 16>.  Switched on, a forward
launch of theirs takes its B fragments from a fragment-order image of the layer's fp16 pieces (one 16-byte buffer load per
32-channel tile and piece) and keeps only the patch in LDS: one workgroup barrier per 16-channel chunk instead of one per tap.
The pieces are the same bits and every accumulator sees the same MFMAs in the same order, so EVERYTHING here is bitwise, the
engine with both shapes switched on against StyleEngine(h2_direct_weights=False) in one process: no tolerance.  That the new
loop ran is read from the launcher's own count (nst_ctx_h2_direct_launches), closure by closure.

What is compared per job: every stored activation - nst_level_activation of all 13 layers of every level (for the maps a
default job does not store that is nst_level_activation's repeat launch), and nst_vgg_activations of the start image (the
per-level walker's forward) - which takes in the outputs of the four launches and the pooled maps behind conv1_2 and conv2_2
through the layers that read them; and the closure's loss row and pixel gradient, whose backward half consumes the ReLU
masks, pool codes and absmax records those launches write.

Shapes: single-level jobs at 16x16 (exactly one 16x16 tile, two 8x16 tiles), 24x40 (a row and a column remainder), 50x76
(ragged: edge tiles take the general epilogue, pooling meets odd sizes) and 18x42; a two- and a three-level job at 64x96
(batched launch, small levels in the tail of the grid, a 16x24 level whose 8x12 and 4x6 maps are smaller than a tile).
18x42 stands for "9x21: smaller than either tile": an image must have 16 pixels per side (asserted below), so the 9x21
map is the one conv2_1 and conv2_2 run on there, and conv3_1 runs on 4x10.

One case holds the job at 50x76 to the CPU oracle the way tests/test_hip_tile_shapes.py holds every tile shape
(hip_helpers.closure_vs_oracle_under_equal_decisions with cap 1e-2 on the weighted sum and the style term: losses 1e-5, the
whole gradient 2e-5 under the device's decisions, and the device's ReLU decisions - conv1_2's and conv3_1's among them -
differing from the oracle's at near-ties only), and the two layers' maps themselves to the oracle's at the rel-L2 bound of
tests/test_hip_parity.py::test_vgg_features_vs_oracle, 3e-6."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import (CW, SW, TERMS, TVW, closure_vs_oracle_under_equal_decisions, dev, levels, oracle_targets, rel_l2, report,
                         setup)

pytestmark = pytest.mark.gpu

GEOMETRIES = {"18x42_L1": (18, 42, 1), "16x16_L1": (16, 16, 1), "24x40_L1": (24, 40, 1), "50x76_L1": (50, 76, 1),
              "64x96_L2": (64, 96, 2), "64x96_L3": (64, 96, 3)}
CONV1_2, CONV3_1 = 1, 4          # layer indices of the two layers the oracle case names


def _pair(vgg_weights, **opts):
    from artstyletransfer_amd.engine import StyleEngine
    a, b = StyleEngine(vgg_weights, 0, h2_direct_weights=True, **opts), StyleEngine(vgg_weights, 0, h2_direct_weights=False, **opts)
    assert a.lib.nst_ctx_h2_direct_weights(a.ctx) == 3 and b.lib.nst_ctx_h2_direct_weights(b.ctx) == 0
    return a, b


@pytest.fixture(scope="module")
def pair(vgg_weights):
    """(fragments from L2 on both kernel shapes, switch-off engine) on the same synthetic weights, batched schedule."""
    a, b = _pair(vgg_weights)
    yield a, b
    a.close()
    b.close()


@pytest.fixture(scope="module")
def pair_per_level(vgg_weights):
    """The same on the per-level walker (NST_BATCH=0)."""
    a, b = _pair(vgg_weights, batched=False)
    yield a, b
    a.close()
    b.close()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _start(c0, seed=9):
    h, w = c0.shape[:2]
    return (0.6 * c0 + 0.4 * cpu_ref.synthetic_image(h, w, seed=seed)).astype(np.float32)


def _rgb_job(engines, h, w, nlev):
    c, s = levels(h, w, nlev, 1), levels(h, w, nlev, 2)
    for e in engines:
        setup(e, c, s)
    return dev(cpu_ref.prepare_img(_start(c[0])))


def _luminance_job(engines, h, w, nlev):
    from artstyletransfer_amd import host_image
    c, s = levels(h, w, nlev, 5), levels(h, w, nlev, 6)
    alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
    for e in engines:
        e.configure(nlev, h, w)
        e.set_color("luminance")
        for i in range(nlev):
            e.set_targets(i, dev(torch.from_numpy(host_image.luminance(c[i]))),
                          dev(torch.from_numpy(host_image.luminance(s[i], alpha, beta))))
    return dev(torch.from_numpy(host_image.luminance(_start(c[0]))).reshape(1, 1, h, w))


def _everything(e, x, nlev, rgb, per_level=False):
    """Bit patterns of the closure's gradient and loss row, of all 13 activations of every level, and (an RGB image) of
    nst_vgg_activations of x."""
    ran = e.lib.nst_ctx_h2_direct_launches(e.ctx)
    g, l = e.closure(x, CW, SW, TVW)
    torch.cuda.synchronize()
    # the launcher's own count of launches on the new loop: conv1_2, conv2_1, conv2_2, conv3_1 - once for all levels in the
    # batched schedule, once per level in the per-level one - under the shapes' bits of the setting, and none without
    mask = e.lib.nst_ctx_h2_direct_weights(e.ctx)
    per_pass = (1 if mask & 1 else 0) + (3 if mask & 2 else 0)
    assert e.lib.nst_ctx_h2_direct_launches(e.ctx) - ran == per_pass * (nlev if per_level else 1), (mask, ran)
    assert np.isfinite(l.cpu().numpy()).all() and float(g.abs().max()) > 0
    out = {"gradient": _bits(g), "loss rows": _bits(l)}
    for lv in range(nlev):
        for i, a in enumerate(e.level_activations(lv)):
            out[f"level {lv} layer {i}"] = _bits(a)
    if rgb:
        for i, a in enumerate(e.vgg_activations(x)):
            out[f"vgg_activations layer {i}"] = _bits(a)
    return out


def _assert_same(engines, x, nlev, rgb=True, per_level=False):
    on, off = (_everything(e, x, nlev, rgb, per_level) for e in engines)
    assert on.keys() == off.keys()
    for what in on:
        assert on[what].shape == off[what].shape and np.array_equal(on[what], off[what]), what
    # (the maps are not trivially equal: the two layers' outputs are there and alive)
    assert on[f"level 0 layer {CONV1_2}"].any() and on[f"level 0 layer {CONV3_1}"].any()


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_jobs_are_bitwise_those_of_the_switch_off(pair, geo):
    h, w, nlev = GEOMETRIES[geo]
    _assert_same(pair, _rgb_job(pair, h, w, nlev), nlev)


def test_an_image_below_16_pixels_per_side_is_refused(pair):
    """Why the 9x21 case is the 9x21 MAP of an 18x42 job: the network has no 9x21 image."""
    from artstyletransfer_amd.engine import NstError
    with pytest.raises(NstError, match="too small"):
        pair[0].vgg_activations(dev(torch.zeros(1, 3, 9, 21)))
    with pytest.raises(NstError, match="at least 16x16"):
        pair[0].configure(1, 9, 21)


@pytest.mark.parametrize("geo", ["50x76_L1", "64x96_L2"])
def test_average_pooling_is_bitwise_that_of_the_switch_off(pair, geo):
    """The average-pool epilogue and its multi-hot code behind conv1_2 and conv2_2."""
    h, w, nlev = GEOMETRIES[geo]
    try:
        for e in pair:
            e.configure(nlev, h, w)
            e.set_pooling("avg")
        _assert_same(pair, _rgb_job(pair, h, w, nlev), nlev)
    finally:
        for e in pair:
            e.reset_pooling()


@pytest.mark.parametrize("geo", ["24x40_L1", "64x96_L2"])
def test_luminance_mode_is_bitwise_that_of_the_switch_off(pair, geo):
    h, w, nlev = GEOMETRIES[geo]
    try:
        _assert_same(pair, _luminance_job(pair, h, w, nlev), nlev, rgb=False)
    finally:
        for e in pair:
            e.reset_color()


@pytest.mark.parametrize("geo", ["50x76_L1", "64x96_L2"])
def test_per_level_walker_is_bitwise_that_of_the_switch_off(pair_per_level, geo):
    """NST_BATCH=0: launch_conv_h2, one image per launch."""
    h, w, nlev = GEOMETRIES[geo]
    _assert_same(pair_per_level, _rgb_job(pair_per_level, h, w, nlev), nlev, per_level=True)


def test_per_level_and_batched_walkers_agree_bitwise(pair, pair_per_level):
    """A schedule keeps its twin's bits: conv1_1 .. conv3_1 of the per-level walker are the batched walker's (from conv3_2 on
    the batched walker runs the Winograd kernel and the per-level one the direct kernel: equal to rounding, not bitwise)."""
    h, w, nlev = GEOMETRIES["64x96_L2"]
    both = (pair[0], pair_per_level[0])
    x = _rgb_job(both, h, w, nlev)
    acts = []
    for e in both:
        e.closure(x, CW, SW, TVW)
        acts.append([_bits(e.level_activation(lv, l)) for lv in range(nlev) for l in range(CONV3_1 + 1)])
    for i, (a, b) in enumerate(zip(*acts)):
        assert a.any() and np.array_equal(a, b), i


def test_job_at_50x76_vs_oracle(pair, vgg_weights):
    """The default engine (fragments from L2) at 50x76 against the CPU oracle, as test_hip_tile_shapes.py holds a tile shape:
    closure_vs_oracle_under_equal_decisions, weighted sum and style term, cap 1e-2.  conv1_2's and conv3_1's maps against the
    oracle's: test_hip_tile_shapes.py has no bound for a map, so the two are held to the bound tests/test_hip_parity.py holds
    the device's feature maps to against this oracle (test_vgg_features_vs_oracle, 50x76 among its sizes): rel-L2 < 3e-6.
    Measured: conv1_2 2.1e-7, conv3_1 4.9e-7."""
    h, w, nlev = GEOMETRIES["50x76_L1"]
    c, s = levels(h, w, nlev, 1), levels(h + 10, w - 6, nlev, 2)
    xt = cpu_ref.prepare_img((0.7 * c[0] + 0.3 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32))
    tg = oracle_targets(c, s, vgg_weights)
    e = pair[0]
    setup(e, c, s)
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "h2 direct weights 50x76 L0", terms=(TERMS[0], TERMS[2]), cap=1e-2)
    rec = []
    cpu_ref.vgg19_features(xt, vgg_weights, record=rec)
    e.closure(dev(xt), CW, SW, TVW)
    for name, l in (("conv1_2", CONV1_2), ("conv3_1", CONV3_1)):
        got = e.level_activation(0, l).cpu().numpy()
        err = rel_l2(got, torch.relu(rec[l]).numpy())
        report(f"h2 direct weights 50x76: {name} output vs the oracle's, rel-L2 {err:.2e}")
        assert err < 3e-6, (name, err)
    assert e.lib.nst_ctx_h2_direct_launches(e.ctx) > 0


def test_the_environment_variable_and_the_setter(vgg_weights, monkeypatch):
    from artstyletransfer_amd.engine import StyleEngine
    monkeypatch.setenv("NST_H2_DIRECT_WEIGHTS", "0")
    e = StyleEngine(vgg_weights, 0)
    try:
        assert e.lib.nst_ctx_h2_direct_weights(e.ctx) == 0
        assert e.lib.nst_ctx_h2_direct_launches(e.ctx) == 0
        for mask in (1, 2, 3):
            assert e.lib.nst_ctx_set_h2_direct_weights(e.ctx, mask) == 0 and e.lib.nst_ctx_h2_direct_weights(e.ctx) == mask
        assert e.lib.nst_ctx_set_h2_direct_weights(e.ctx, 4) != 0 and e.lib.nst_ctx_h2_direct_weights(e.ctx) == 3
        assert e.lib.nst_ctx_h2_direct_weights(None) == -1 and e.lib.nst_ctx_h2_direct_launches(None) == -1
    finally:
        e.close()


def test_switching_within_one_context_keeps_the_bits(vgg_weights):
    """The setter on a live job: both shapes, off, each shape alone, both again - one context, the same maps and closure
    each time (and, in _everything, the launch count of each mask)."""
    from artstyletransfer_amd.engine import StyleEngine
    h, w, nlev = GEOMETRIES["64x96_L2"]
    e = StyleEngine(vgg_weights, 0)
    try:
        x = _rgb_job((e,), h, w, nlev)
        runs = []
        for mask in (3, 0, 1, 2, 3):
            assert e.lib.nst_ctx_set_h2_direct_weights(e.ctx, mask) == 0
            runs.append(_everything(e, x, nlev, True))
        for what in runs[0]:
            for other in runs[1:]:
                assert np.array_equal(runs[0][what], other[what]), what
    finally:
        e.close()
