"""GPU: the packed Gram pass (nst_ctx_set_gram_pack, on by default) against its switch-off twin in the same build.

Packed, the fp16-piece partial kernels do not compute the 32x32 blocks strictly below the diagonal of a diagonal tile - the
finish pass reads elements with j >= i only and mirrors them - and leave that part of a slab unwritten; the ten kept blocks
of a 128-wide diagonal tile are dealt 3 / 2 / 2 / 3 to the four waves.  A plain batch takes its 64-channel and its
128-channel-tile maps in one partial launch.  A kept block sees the same MFMAs in the same order and every workgroup keeps
its (item, tile pair, split), so everything must agree BITWISE with the switch-off engine: single Gram matrices, loss rows
and gradients of whole jobs.  (That the waves' blocks are exactly the upper triangle, each once, is a static_assert in
gram.hip: a build that breaks it does not compile.)

Single maps: the smallest shapes that reach each branch (splits follow gram_nsplit) - less than one chunk, ragged last
chunks, one and two chunks per split, one / two / three / four tiles per side (diagonal and off-diagonal pairs, an odd tile
count).  Stale slabs: a Gram of huge values first, so that the unwritten blocks of the partial buffer hold them.
Jobs: the geometries of test_hip_forward_pack.py, where items of both tile shapes and of every level lie in one grid."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels, rel_l2, setup

pytestmark = pytest.mark.gpu

# C, h, w
SHAPES = [(64, 3, 5), (64, 150, 230), (128, 17, 9), (128, 96, 100), (256, 50, 61), (384, 9, 11), (512, 30, 31), (512, 3, 5)]
GEOMETRIES = {"72x104_L3": (72, 104, 3), "50x76_L2": (50, 76, 2)}


@pytest.fixture(scope="module")
def pair(vgg_weights):
    """(packed engine - the default, switch-off engine) on the same synthetic weights."""
    from artstyletransfer_amd.engine import StyleEngine
    a, b = StyleEngine(vgg_weights, 0), StyleEngine(vgg_weights, 0, gram_pack=False)
    assert a.lib.nst_ctx_gram_pack(a.ctx) == 1 and b.lib.nst_ctx_gram_pack(b.ctx) == 0
    yield a, b
    a.close()
    b.close()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _map(C, h, w):
    g = torch.Generator().manual_seed(C + h)
    return torch.randn(1, C, h, w, generator=g).clamp_min(0) + 0.1 * torch.randn(1, C, h, w, generator=g)


@pytest.mark.parametrize("C,h,w", SHAPES, ids=[f"{c}x{h}x{w}" for c, h, w in SHAPES])
def test_single_map_is_bitwise_that_of_the_switch_off_and_holds_the_fp64_bounds(pair, C, h, w):
    f = _map(C, h, w)
    ref = cpu_ref.gram_matrix(f.double()).float()
    fd = dev(f)
    outs = [e.gram(fd).cpu() for e in pair]
    for what, out in zip(("packed", "switch-off"), outs):
        # test_gram_mfma's bounds
        err = rel_l2(out, ref)
        print(f"{what} C={C} {h}x{w}: rel_l2 {err:.3e}")
        assert err < 2e-6, what
        np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-4, atol=1e-6 * float(ref.abs().max()), err_msg=what)
        assert torch.equal(out[0], out[0].t()), what
    assert torch.equal(outs[0], outs[1])
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


def test_stale_slabs_are_never_read(pair, vgg_weights):
    """The blocks below the diagonal of a diagonal tile keep what the partial buffer held: after a Gram of the map times 2^40
    they hold values 2^80 times too large.  The Gram of the map itself must still be bitwise that of a fresh engine."""
    from artstyletransfer_amd.engine import StyleEngine
    eng = pair[0]
    f = dev(_map(128, 96, 100))
    big = eng.gram(f * float(2.0 ** 40)).cpu()
    assert torch.isfinite(big).all() and float(big.abs().max()) > 2.0 ** 60
    again = eng.gram(f).cpu()
    fresh_eng = StyleEngine(vgg_weights, 0)
    try:
        assert fresh_eng.lib.nst_ctx_gram_pack(fresh_eng.ctx) == 1
        fresh = fresh_eng.gram(f).cpu()
    finally:
        fresh_eng.close()
    assert np.array_equal(_bits(again), _bits(fresh))
    assert torch.equal(again[0], again[0].t())


def _start(c0, seed=9):
    h, w = c0.shape[:2]
    return (0.6 * c0 + 0.4 * cpu_ref.synthetic_image(h, w, seed=seed)).astype(np.float32)


def _rgb_job(engines, h, w, nlev):
    c, s = levels(h, w, nlev, 1), levels(h, w, nlev, 2)
    for e in engines:
        setup(e, c, s)
    return dev(cpu_ref.prepare_img(_start(c[0])))


def _guided_job(engines, h, w, nlev):
    c, s = levels(h, w, nlev, 1), levels(h, w, nlev, 2)
    for e in engines:
        e.configure(nlev, h, w)
        for l in range(nlev):
            hl, wl = h >> l, w >> l
            # R = 2, soft planes as in test_hip_forward_pack.py: 0.9 on the own half and 0.7 on the other
            left = np.full((hl, wl), 0.7, dtype=np.float32)
            left[:, : wl // 2] = 0.9
            planes = dev(torch.from_numpy(np.stack([left, 1.6 - left]).astype(np.float32)))
            e.set_guidance(l, planes)
            e.set_targets_guided(l, dev(cpu_ref.prepare_img(c[l])), dev(cpu_ref.prepare_img(s[l])), planes)
    return dev(cpu_ref.prepare_img(_start(c[0])))


def _centred_job(engines, h, w, nlev):
    c, s = levels(h, w, nlev, 1), levels(h, w, nlev, 2)
    for e in engines:
        e.configure(nlev, h, w)
        e.set_gram_shift("mean")          # every style map centred
        for i in range(nlev):
            e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
    return dev(cpu_ref.prepare_img(_start(c[0])))


def _closure_and_halves(e, x):
    g0, l0 = e.closure(x, CW, SW, TVW)
    l1 = e.closure_forward(x, CW, SW, TVW)
    g1 = torch.full_like(g0, -12345.0)
    e.closure_backward(x, CW, SW, TVW, grad=g1)
    torch.cuda.synchronize()
    assert np.isfinite(l0.cpu().numpy()).all() and float(g0.abs().max()) > 0
    return [_bits(g0), _bits(l0), _bits(g1), _bits(l1)]


def _assert_same(packed, plain, x):
    got, ref = _closure_and_halves(packed, x), _closure_and_halves(plain, x)
    for what, a, b in zip(("gradient", "loss rows", "gradient of the halves", "loss rows of the forward half"), got, ref):
        assert a.shape == b.shape and np.array_equal(a, b), what
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_jobs_are_bitwise_those_of_the_switch_off(pair, geo):
    h, w, nlev = GEOMETRIES[geo]
    _assert_same(*pair, _rgb_job(pair, h, w, nlev))


@pytest.mark.parametrize("mode", ["guided", "centred"])
def test_guided_and_centred_jobs_are_bitwise_those_of_the_switch_off(pair, mode):
    """The diagonal-tile rule is part of the shared body: it reaches the guided and the shifted kernels too (two levels: on
    the 1x1 relu5_1 map of an 18x26 level no region but t = 1 has one pixel's worth of mass)."""
    h, w, nlev = GEOMETRIES["50x76_L2"]
    try:
        x = _guided_job(pair, h, w, nlev) if mode == "guided" else _centred_job(pair, h, w, nlev)
        _assert_same(*pair, x)
    finally:
        for e in pair:
            e.configure(nlev, h, w)          # (drops the guidance and the Gram shift)


def test_the_environment_variable_and_the_setter(vgg_weights, monkeypatch):
    from artstyletransfer_amd.engine import StyleEngine
    monkeypatch.setenv("NST_GRAM_PACK", "0")
    e = StyleEngine(vgg_weights, 0)
    try:
        assert e.lib.nst_ctx_gram_pack(e.ctx) == 0
        assert e.lib.nst_ctx_set_gram_pack(e.ctx, 1) == 0 and e.lib.nst_ctx_gram_pack(e.ctx) == 1
        assert e.lib.nst_ctx_gram_pack(None) == -1
    finally:
        e.close()
