"""nst_ctx_bytes is a function of the context's current state, not of the path to it: every device allocation of the context
belongs to an owner that credits on release exactly what was charged (csrc/nst_devmem.h).  Integer and bitwise equalities
only.  The job is the smallest nst_job_configure accepts at two levels (32x48 over 16x24), the style image 32x40, f16x2."""
import ctypes as C

import numpy as np
import pytest
import torch

from hip_helpers import CW, SW, TVW, dev, levels
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

H, W, HS, WS, NLEV = 32, 48, 32, 40, 2
E_ARG = -1


def _job():
    contents, styles = levels(H, W, NLEV, 1), levels(HS, WS, NLEV, 2)
    x = (0.6 * contents[0] + 0.4 * cpu_ref.synthetic_image(H, W, 9)).astype(np.float32)
    return contents, styles, dev(cpu_ref.prepare_img(x))


def _targets(e, contents, styles):
    for i in range(NLEV):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))


def _planes():
    """Two regions, the left and the right half: every scale down to 2x3 keeps a mass above one pixel's worth."""
    p = torch.zeros((2, H, W), dtype=torch.float32)
    p[0, :, :W // 2] = 1.0
    p[1, :, W // 2:] = 1.0
    return dev(p)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# name -> (switch the block on, switch it off)
TERMS = {
    "laplacian": (lambda e: e.set_laplacian((1, 2), (1.0, 0.5)), lambda e: e.reset_laplacian()),
    "matting": (lambda e: e.set_matting(100.0), lambda e: e.reset_matting()),
    "gram_shift": (lambda e: e.set_gram_shift(None, center_mask=1), lambda e: e.reset_gram_shift()),
    "moments": (lambda e: e.set_moments(1.0), lambda e: e.reset_moments()),
    "guidance": (lambda e: e.set_guidance(0, _planes()), lambda e: e.set_guidance(0, None)),
}


def _fresh(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    e.configure(NLEV, H, W)
    return e


@pytest.fixture(scope="module")
def eng(vgg_weights):
    """A context with history: configured, targets made, one closure run; the tests below keep using it."""
    e = _fresh(vgg_weights)
    contents, styles, x = _job()
    _targets(e, contents, styles)
    e.closure(x, CW, SW, TVW)
    yield e
    e.close()


# ---- 1. path independence --------------------------------------------------------------------------------------------------------
def test_a_long_walk_ends_at_the_count_and_the_bits_of_a_fresh_context(vgg_weights):
    contents, styles, x = _job()
    a, b = _fresh(vgg_weights), _fresh(vgg_weights)
    try:
        _targets(a, contents, styles)
        for on, off in TERMS.values():
            on(a)
            off(a)
        a.set_taps(4, (0, 1, 2))
        a.reset_taps()
        a.set_color("luminance")
        a.set_color("rgb")
        a.configure(1, 32, 32)
        a.configure(NLEV, H, W)
        for _ in range(3):
            _targets(a, contents, styles)
        ga, la = a.closure(x, CW, SW, TVW)
        _targets(b, contents, styles)
        gb, lb = b.closure(x, CW, SW, TVW)
        print(f"bytes after the walk {a.bytes()}, fresh {b.bytes()}")
        assert a.bytes() == b.bytes()
        assert np.array_equal(_bits(ga), _bits(gb)) and np.array_equal(_bits(la), _bits(lb))
    finally:
        a.close()
        b.close()


# ---- 2. each block alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("term", list(TERMS))
def test_a_block_costs_the_same_however_often_it_was_switched(eng, vgg_weights, term):
    on, off = TERMS[term]
    before = eng.bytes()
    on(eng)
    off(eng)
    assert eng.bytes() == before
    on(eng)
    held = eng.bytes()
    b = _fresh(vgg_weights)
    try:
        base = b.bytes()
        on(b)
        print(f"{term}: {held - before} bytes on the walked context, {b.bytes() - base} on a fresh one")
        assert held - before == b.bytes() - base and held > before
        off(b)
        assert b.bytes() == base
    finally:
        b.close()
    off(eng)
    assert eng.bytes() == before


# ---- 3. standalone calls leave the count where it was -------------------------------------------------------------------------------
def test_standalone_calls_leave_the_count_where_it_was(eng):
    contents, styles, x = _job()
    g = torch.Generator().manual_seed(3)
    f = dev(torch.rand((1, 64, 16, 24), generator=g))
    hwc = dev(torch.from_numpy(contents[0]))
    noise = dev(torch.rand((H, W, 3), generator=g) * 255.0)
    guide = dev(torch.rand((1, 3, H, W), generator=g))
    content_t = dev(cpu_ref.prepare_img(contents[0]))
    _targets(eng, contents, styles)       # (the setters of the tests before dropped them)
    eng.closure(x, CW, SW, TVW)
    eng.color_stats(hwc)                  # (its scratch is made on first use and kept)
    calls = {
        "nst_gram": lambda: eng.gram(f),
        "nst_gram_shifted (shift)": lambda: eng.gram_shifted(f, shift=0.5),
        "nst_gram_shifted (center)": lambda: eng.gram_shifted(f, center=True),
        "nst_gram_shifted (plain)": lambda: eng.gram_shifted(f),
        "nst_gram_batch": lambda: eng.gram_batch([f, f], targets=[eng.gram(f)[0].contiguous(), None], coefs=[1.0, 0.0], want_S_bf=True),
        "nst_moments": lambda: eng.moments(f),
        "nst_level_activation (a map the pass left out)": lambda: eng.level_activation(0, 1),
        "nst_level_activation": lambda: eng.level_activation(1, 9),
        "nst_total_variation": lambda: eng.total_variation(x, want_grad=True),
        "nst_noise_blend": lambda: eng.noise_blend(hwc, noise, 0.5),
        "nst_laplacian_loss": lambda: eng.laplacian_loss(x, content_t, 2, want_grad=True),
        "nst_matting_loss": lambda: eng.matting_loss(x, guide, want_grad=True),
        "nst_vgg_features": lambda: eng.vgg_features(x),
        "nst_color_stats (second call)": lambda: eng.color_stats(hwc),
        "nst_level_set_targets": lambda: _targets(eng, contents, styles),
        "nst_closure": lambda: eng.closure(x, CW, SW, TVW),
    }
    before = eng.bytes()
    moved = {}
    for name, call in calls.items():
        call()
        torch.cuda.synchronize()
        if eng.bytes() != before:
            moved[name] = eng.bytes() - before
            before = eng.bytes()
    print(f"count {before}; calls that moved it: {moved}")
    assert not moved, moved


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_a_refused_setter_leaves_the_count_and_the_setting(eng):
    from artstyletransfer_amd.engine import _stream
    lib, ctx = eng.lib, eng.ctx
    f6 = C.c_float * 6
    # two terms that go together with their blocks on, then the other two
    eng.set_laplacian((1, 2), (1.0, 0.5))
    eng.set_matting(100.0)
    eng.set_gram_shift(None, center_mask=1)
    eng.set_moments(1.0)
    state = lambda: (eng.bytes(), lib.nst_job_color(ctx), lib.nst_job_pooling(ctx), eng.style_weights(), eng.laplacian_setting(),
                     eng.matting_setting(), eng.gram_shift_setting(), eng.moments_setting(), eng.guidance(0)[:2])
    before = state()
    refused = {
        "configure: no level": lambda: lib.nst_job_configure(ctx, 0, H, W),
        "configure: coarsest level below 16x16": lambda: lib.nst_job_configure(ctx, 3, H, W),
        "taps: content index": lambda: lib.nst_job_set_taps(ctx, 9, 0x2F, 1),
        "taps: empty style set": lambda: lib.nst_job_set_taps(ctx, 4, 0, 1),
        "color": lambda: lib.nst_job_set_color(ctx, 7),
        "pooling": lambda: lib.nst_job_set_pooling(ctx, 7),
        "style weights": lambda: lib.nst_job_set_style_weights(ctx, f6(-1, 1, 1, 1, 1, 1)),
        "laplacian: level 1 too small": lambda: lib.nst_job_set_laplacian(ctx, 1, (C.c_int * 1)(8), (C.c_float * 1)(1.0)),
        "laplacian: all weights zero": lambda: lib.nst_job_set_laplacian(ctx, 1, (C.c_int * 1)(2), (C.c_float * 1)(0.0)),
        "matting": lambda: lib.nst_job_set_matting(ctx, -1.0, 1e-7),
        "gram shift: not finite": lambda: lib.nst_job_set_gram_shift(ctx, f6(float("nan"), 0, 0, 0, 0, 0), 0),
        "gram shift: shift on a centred map": lambda: lib.nst_job_set_gram_shift(ctx, f6(1, 0, 0, 0, 0, 0), 1),
        "moments: negative weight": lambda: lib.nst_job_set_moments(ctx, f6(-1, 0, 0, 0, 0, 0), f6(), 1e-5),
        "moments: not a style map": lambda: lib.nst_job_set_moments(ctx, f6(0, 0, 0, 0, 1, 0), f6(), 1e-5),
        "guidance: too many regions": lambda: lib.nst_level_set_guidance(ctx, 0, 9, None, None, _stream(eng.device)),
    }
    for name, call in refused.items():
        assert call() == E_ARG, name
        assert state() == before, name
    eng.reset_gram_shift()
    eng.reset_moments()
    # guidance, on a level that is guided already: refused after the new pyramid was allocated and built
    eng.set_guidance(0, _planes(), (1.0, 0.5))
    before = state()
    mass = eng.guidance(0)[2].copy()
    bad = _planes()
    bad[0, 3, 5] = 2.0
    empty = _planes()
    empty[1] = 0.0
    three = dev(torch.full((3, H, W), 0.5))
    for name, planes in (("a value outside [0,1]", bad), ("a region without mass", empty), ("another R, outside [0,1]", three * 4.0)):
        rc = lib.nst_level_set_guidance(ctx, 0, planes.shape[0], C.c_void_p(planes.data_ptr()), None, _stream(eng.device))
        assert rc == E_ARG, name
        assert state() == before and np.array_equal(eng.guidance(0)[2], mass), name
    eng.set_guidance(0, None)
    eng.reset_laplacian()
    eng.reset_matting()
