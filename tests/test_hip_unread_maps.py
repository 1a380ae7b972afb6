"""GPU: the batched f16x2 forward pass leaves out the full-resolution maps nothing reads (conv1_2, conv2_2, conv3_4, conv4_4
with the default taps: only their pooled forms, ReLU masks and pool codes are written).  An engine that elides and one that
keeps every map (keep_all_maps=True, the behaviour before the elision) must agree BITWISE in everything a job returns, and
nst_level_activation must still hand out every map exactly.

Geometries: 88x136 with 3 levels (edge tiles in both dimensions for the 8x16 Winograd tile and the direct shapes at every
level; the lowest level is 22x34) and 64x96 with 2 levels (the job of tests/test_hip_lazy_backward.py).

The taps of a job (nst_job_set_taps) are chosen among relu1_1, relu2_1, relu3_1, relu4_1, conv4_2 and relu5_1: no map in
front of a pooling layer can be made a tap through the C ABI (nst_closure.cpp asserts it at compile time), so a job with such
a tap does not exist and has no case here; test_no_taps_choice_reaches_a_pre_pool_map runs other taps than the default."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels, setup

pytestmark = pytest.mark.gpu

UNREAD = (1, 3, 7, 11)                       # conv1_2, conv2_2, conv3_4, conv4_4
ALL_MAPS = (1 << 13) - 1
DEFAULT_STORED = ALL_MAPS & ~sum(1 << l for l in UNREAD)
GEOMETRIES = {"88x136_L3": (88, 136, 3), "64x96_L2": (64, 96, 2)}
FIELDS = ("closures", "total_closures", "accepted", "loss", "lr", "t", "history")


@pytest.fixture(scope="module")
def pair(vgg_weights):
    """(eliding engine, keep-all engine) on the same synthetic weights (non-zero biases)."""
    from artstyletransfer_amd.engine import StyleEngine
    a, b = StyleEngine(vgg_weights, 0), StyleEngine(vgg_weights, 0, keep_all_maps=True)
    # the test hooks of nst_ctx.cpp (not part of include/nst_hip.h): declared once, on the library object all engines share
    a.lib.nst_internal_map_fill.restype = a.lib.nst_internal_map_read.restype = C.c_int
    a.lib.nst_internal_map_fill.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    a.lib.nst_internal_map_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert a.lib.nst_ctx_keep_all_maps(a.ctx) == 0 and b.lib.nst_ctx_keep_all_maps(b.ctx) == 1
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


def _closure_and_halves(e, x):
    g0, l0 = e.closure(x, CW, SW, TVW)
    l1 = e.closure_forward(x, CW, SW, TVW)
    g1 = torch.full_like(g0, -12345.0)
    e.closure_backward(x, CW, SW, TVW, grad=g1)
    torch.cuda.synchronize()
    assert np.isfinite(l0.cpu().numpy()).all() and float(g0.abs().max()) > 0
    return _bits(g0), _bits(l0), _bits(g1), _bits(l1)


def _assert_same_closure(elide, keep, x):
    got, ref = _closure_and_halves(elide, x), _closure_and_halves(keep, x)
    for what, a, b in zip(("gradient", "loss row", "gradient of the halves", "loss row of the forward half"), got, ref):
        assert np.array_equal(a, b), what
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_closure_is_bitwise_that_of_keep_all(pair, geo):
    h, w, nlev = GEOMETRIES[geo]
    x = _rgb_job(pair, h, w, nlev)
    _assert_same_closure(*pair, x)
    for l in range(nlev):
        assert pair[0].map_stats(l) == DEFAULT_STORED and pair[1].map_stats(l) == ALL_MAPS


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_level_activations_are_bitwise_and_leave_the_job_as_it_was(pair, geo):
    elide, keep = pair
    h, w, nlev = GEOMETRIES[geo]
    x = _rgb_job(pair, h, w, nlev)
    g0, l0 = elide.closure(x, CW, SW, TVW)
    keep.closure(x, CW, SW, TVW)
    g0, l0 = _bits(g0), _bits(l0)
    for lvl in range(nlev):
        assert elide.map_stats(lvl) == DEFAULT_STORED
    for lvl in range(nlev):
        got, ref = elide.level_activations(lvl), keep.level_activations(lvl)
        assert len(got) == 13
        for l, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(_bits(a), _bits(b)), (lvl, l)
            if l in UNREAD:
                assert float(a.abs().max()) > 0, (lvl, l)
    # (one request repeats a layer's launch over all levels of the pass: every level has the map afterwards)
    for lvl in range(nlev):
        assert elide.map_stats(lvl) == ALL_MAPS
    g1, l1 = elide.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), g0) and np.array_equal(_bits(l1), l0)
    assert elide.map_stats(0) == DEFAULT_STORED
    # a single map on request, after a forward half: only that layer is written
    elide.closure_forward(x, CW, SW, TVW)
    a = elide.level_activation(nlev - 1, 7)
    keep.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(a), _bits(keep.level_activation(nlev - 1, 7)))
    assert elide.map_stats(0) == DEFAULT_STORED | (1 << 7)
    g2, l2 = elide.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g2), g0) and np.array_equal(_bits(l2), l0)


def test_map_stats_before_a_pass_and_after_set_up_calls(pair):
    elide, _ = pair
    _rgb_job((elide,), 64, 96, 2)
    assert elide.map_stats(0) == 0 and elide.map_stats(1) == 0       # (set_targets ran a pass of its own: not a closure's)
    elide.level_activations(0)                                      # copies what the buffers hold, as it always did
    assert elide.map_stats(0) == 0
    m = C.c_uint(0)
    assert elide.lib.nst_job_map_stats(elide.ctx, 5, C.byref(m)) < 0
    assert elide.lib.nst_job_map_stats(elide.ctx, 0, None) < 0


def test_no_taps_choice_reaches_a_pre_pool_map(pair):
    """Other taps than the default: bitwise parity, and bits 1, 3, 7 (11 lies above the top of this job) stay clear - the six
    maps nst_job_set_taps chooses among are conv layers 0, 2, 4, 8, 9, 12, none of them in front of a pooling layer."""
    try:
        for e in pair:
            e.configure(2, 64, 96)
            e.set_taps(2, [2, 3], True)
        x = _rgb_job(pair, 64, 96, 2)
        _assert_same_closure(*pair, x)
        top = 8                                                      # relu4_1
        want = sum(1 << l for l in range(top + 1) if l not in UNREAD)
        assert pair[0].map_stats(0) == want and pair[1].map_stats(0) == (1 << (top + 1)) - 1
    finally:
        for e in pair:
            e.reset_taps()


def _raw(e, level, layer):
    h, w = e.level_shape(level)
    n = (h >> e.LAYER_SCALE[layer]) * (w >> e.LAYER_SCALE[layer]) * e.LAYER_CHANNELS[layer]
    t = torch.empty(n, dtype=torch.int32, device=e.device)
    assert e.lib.nst_internal_map_read(e.ctx, level, layer, C.c_void_p(t.data_ptr())) == 0
    return t.cpu().numpy()


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_the_store_is_gone(pair, geo):
    """The four buffers filled with a sentinel byte pattern, a forward half, the buffers read back raw."""
    h, w, nlev = GEOMETRIES[geo]
    x = _rgb_job(pair, h, w, nlev)
    sentinel = np.int32(0x5A5A5A5A)
    for e in pair:
        for lvl in range(nlev):
            for l in UNREAD:
                assert e.lib.nst_internal_map_fill(e.ctx, lvl, l, 0x5A) == 0
                assert (_raw(e, lvl, l) == sentinel).all()
        e.closure_forward(x, CW, SW, TVW)
    elide, keep = pair
    for lvl in range(nlev):
        for l in UNREAD:
            assert (_raw(elide, lvl, l) == sentinel).all(), (lvl, l)
            assert not (_raw(keep, lvl, l) == sentinel).any(), (lvl, l)


def _luminance_job(engines, h, w):
    from artstyletransfer_amd import host_image
    c, s = levels(h, w, 2, 5), levels(h, w, 2, 6)
    alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
    for e in engines:
        e.configure(2, h, w)
        e.set_color("luminance")
        for i in range(2):
            e.set_targets(i, dev(torch.from_numpy(host_image.luminance(c[i]))),
                          dev(torch.from_numpy(host_image.luminance(s[i], alpha, beta))))
    return dev(torch.from_numpy(host_image.luminance(_start(c[0]))).reshape(1, 1, h, w))


def _guided_job(engines, h, w):
    c, s = levels(h, w, 2, 1), levels(h, w, 2, 2)
    for e in engines:
        e.configure(2, h, w)
        for l in range(2):
            hl, wl = h >> l, w >> l
            left = np.zeros((hl, wl), dtype=np.float32)
            left[:, : wl // 2] = 1.0
            planes = dev(torch.from_numpy(np.stack([left, 1.0 - left])))          # R = 2: the two halves
            e.set_guidance(l, planes)
            e.set_targets_guided(l, dev(cpu_ref.prepare_img(c[l])), dev(cpu_ref.prepare_img(s[l])), planes)
    return dev(cpu_ref.prepare_img(_start(c[0])))


@pytest.mark.parametrize("mode", ("avg_pool", "luminance", "guided"))
def test_other_job_modes_are_bitwise_those_of_keep_all(pair, mode):
    try:
        if mode == "avg_pool":
            for e in pair:
                e.configure(2, 64, 96)
                e.set_pooling("avg")
            x = _rgb_job(pair, 64, 96, 2)
        elif mode == "luminance":
            x = _luminance_job(pair, 64, 96)
        else:
            x = _guided_job(pair, 64, 96)
        _assert_same_closure(*pair, x)
        assert pair[0].map_stats(0) == DEFAULT_STORED and pair[1].map_stats(1) == ALL_MAPS
        for l in UNREAD:
            assert np.array_equal(_bits(pair[0].level_activation(1, l)), _bits(pair[1].level_activation(1, l))), l
    finally:
        for e in pair:
            e.reset_color()
            e.reset_pooling()
            e.configure(2, 64, 96)          # (drops the guidance)


def _info_tuple(info):
    f32 = lambda v: int(np.asarray(v, dtype=np.float32).view(np.uint32))      # noqa: E731
    return tuple(f32(getattr(info, f)) if f in ("loss", "lr", "t") else int(getattr(info, f)) for f in FIELDS)


def test_lbfgs_driver_is_bitwise_that_of_keep_all(pair):
    """8 L-BFGS steps with max_eval 1 on the job of tests/test_hip_lazy_backward.py (steps 1 and 2 accepted, the later ones
    rejected): a taken trial point runs its backward half on a forward half that elided."""
    from artstyletransfer_amd.engine import PixelOptimizer
    c, s = levels(64, 96, 2, 1), levels(64, 96, 2, 2)
    runs = []
    for e in pair:
        setup(e, c, s)
        x = dev(cpu_ref.prepare_img(c[0]))
        opt = PixelOptimizer(e, "lbfgs", 10.0, 1)
        try:
            out = []
            for _ in range(8):
                info, rows = opt.step(x, CW, SW, TVW)
                out.append((_info_tuple(info), rows.view(np.uint32).copy(), _bits(x)))
            runs.append((out, opt.closure_stats(), opt.backward_stats()))
        finally:
            opt.close()
    (a, sa, ba), (b, sb, bb) = runs
    for k, (p, q) in enumerate(zip(a, b)):
        assert p[0] == q[0], (k, p[0], q[0])
        assert p[1].shape == q[1].shape and np.array_equal(p[1], q[1]), k
        assert np.array_equal(p[2], q[2]), k
    assert sa == sb and ba == bb
    accepted = sum(i[0][2] for i in a)
    assert 1 <= accepted < 8 and ba[0] - ba[1] > 0, (accepted, ba)       # lazy points taken: a backward half on an elided forward


def test_level_split_passes_remember_their_own_levels(vgg_weights, pair):
    """nst_options.level_split: the top level and the lower levels are two forward passes of one closure; a left-out map of
    either is restored over the levels of ITS pass."""
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, level_split=True)
    try:
        keep = pair[1]
        x = _rgb_job((e, keep), 88, 136, 3)
        g, l = e.closure(x, CW, SW, TVW)
        gk, lk = keep.closure(x, CW, SW, TVW)
        assert np.array_equal(_bits(g), _bits(gk)) and np.array_equal(_bits(l), _bits(lk))
        assert [e.map_stats(lvl) for lvl in range(3)] == [DEFAULT_STORED] * 3
        for lvl in range(3):
            for layer in UNREAD:
                assert np.array_equal(_bits(e.level_activation(lvl, layer)), _bits(keep.level_activation(lvl, layer))), (lvl, layer)
        assert [e.map_stats(lvl) for lvl in range(3)] == [ALL_MAPS] * 3
        g2, l2 = e.closure(x, CW, SW, TVW)
        assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(l2), _bits(l))
    finally:
        e.close()


def test_a_request_after_a_later_pass_of_other_levels_is_refused(pair):
    """The one sequence that cannot be served: a closure over levels {0, 1}, then one over level 1 alone.  Level 0's left-out
    maps would need the launch of the first pass repeated over both levels, and level 1 no longer holds that pass:
    NST_E_STATE, nothing written; the maps that were stored, and level 1's own, are still handed out; a closure over all
    levels makes the request good again."""
    from artstyletransfer_amd import _lib
    elide, keep = pair
    x = _rgb_job(pair, 64, 96, 2)
    elide.closure(x, CW, SW, TVW)
    elide.closure_levels(x, CW, SW, TVW, 0b10)
    keep.closure(x, CW, SW, TVW)
    out = torch.full((1, 64, 64, 96), -12345.0, device=x.device)
    rc = elide.lib.nst_level_activation(elide.ctx, 0, 1, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.NST_E_STATE and b"keep_all_maps" in elide.lib.nst_last_error(elide.ctx)
    assert bool((out == -12345.0).all())
    assert elide.map_stats(0) == DEFAULT_STORED
    assert np.array_equal(_bits(elide.level_activation(0, 2)), _bits(keep.level_activation(0, 2)))
    assert np.array_equal(_bits(elide.level_activation(1, 3)), _bits(keep.level_activation(1, 3)))
    elide.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(elide.level_activation(0, 1)), _bits(keep.level_activation(0, 1)))


def test_a_captured_graph_keeps_every_map(vgg_weights, pair):
    """use_graph: a replay runs no host code, so nothing could refresh the record of what a pass stored - such a context
    stores every map.  The image changes in place between replays and the map asked for a second time is the new image's."""
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, use_graph=True)
    try:
        keep = pair[1]
        x = _rgb_job((e, keep), 64, 96, 2)
        g = torch.empty((1, 3, 64, 96), device=x.device)
        rows = torch.empty(9, device=x.device)
        for _ in range(3):                                   # (captured the second time the same buffers are seen)
            e.closure(x, CW, SW, TVW, grad=g, losses=rows)
        gk, lk = keep.closure(x, CW, SW, TVW)
        assert np.array_equal(_bits(g), _bits(gk)) and np.array_equal(_bits(rows), _bits(lk))
        assert e.map_stats(0) == ALL_MAPS
        first = e.level_activation(0, 1)
        assert np.array_equal(_bits(first), _bits(keep.level_activation(0, 1)))
        x.add_(3.0 * torch.sin(torch.arange(x.numel(), device=x.device, dtype=torch.float32)).reshape(x.shape))
        for _ in range(2):
            e.closure(x, CW, SW, TVW, grad=g, losses=rows)
        gk, lk = keep.closure(x, CW, SW, TVW)
        assert np.array_equal(_bits(g), _bits(gk)) and np.array_equal(_bits(rows), _bits(lk))
        second = e.level_activation(0, 1)
        assert e.map_stats(0) == ALL_MAPS
        assert np.array_equal(_bits(second), _bits(keep.level_activation(0, 1)))
        assert not np.array_equal(_bits(second), _bits(first))
    finally:
        e.close()
