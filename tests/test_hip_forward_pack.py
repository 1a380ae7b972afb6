"""GPU: the packed forward half (nst_ctx_set_forward_pack, on by default) against its switch-off twin in the same build.

Packed, the batched f16x2 schedule clears the absmax records, takes the TV partial sums and runs conv1_1 in one launch each
for all pyramid levels, a forward half takes its content / TV loss terms in one launch each, and the bf16 pieces of S that no
f16x2 launch reads are not written.  Switched off, the launch sequence is the parent's.  Only which workgroup does a piece of
work and how many launches carry it changes, so everything a job returns must agree BITWISE: loss rows, the whole gradient
(whole closures and forward half + backward half), and the maps read back through nst_level_activation - relu1_1, which the
batched conv1_1 writes, and relu5_1, the deepest style map.

Geometries: 72x104 with 3 levels (72x104, 36x52, 18x26: every level has ragged 16x16 edge tiles in both dimensions, and the
last tiles of a level and the first of the next share conv1_1 workgroups), 50x76 with 2 levels (50x76, 25x38) and 256x384
with one level, which has nothing to pack at the front.

A work order of the 128-channel-tile Gram launch that keeps the tile pairs of a pixel split on one XCD was built with this
and taken out again (fewer bytes fetched, no faster), and with it the launcher-level case that compared the two
orders."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels, setup

pytestmark = pytest.mark.gpu

GEOMETRIES = {"72x104_L3": (72, 104, 3), "50x76_L2": (50, 76, 2)}
RELU1_1, RELU5_1 = 0, 12


@pytest.fixture(scope="module")
def pair(vgg_weights):
    """(packed engine - the default, switch-off engine) on the same synthetic weights."""
    from artstyletransfer_amd.engine import StyleEngine
    a, b = StyleEngine(vgg_weights, 0), StyleEngine(vgg_weights, 0, forward_pack=False)
    assert a.lib.nst_ctx_forward_pack(a.ctx) == 1 and b.lib.nst_ctx_forward_pack(b.ctx) == 0
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


def _guided_job(engines, h, w, nlev):
    c, s = levels(h, w, nlev, 1), levels(h, w, nlev, 2)
    for e in engines:
        e.configure(nlev, h, w)
        for l in range(nlev):
            hl, wl = h >> l, w >> l
            # R = 2, soft: 0.9 on the own half and 0.7 on the other, so that each region keeps a mass of one pixel's worth on
            # the 1x2 relu5_1 map of the 25x38 level (0.81 + 0.49)
            left = np.full((hl, wl), 0.7, dtype=np.float32)
            left[:, : wl // 2] = 0.9
            planes = dev(torch.from_numpy(np.stack([left, 1.6 - left]).astype(np.float32)))
            e.set_guidance(l, planes)
            e.set_targets_guided(l, dev(cpu_ref.prepare_img(c[l])), dev(cpu_ref.prepare_img(s[l])), planes)
    return dev(cpu_ref.prepare_img(_start(c[0])))


def _everything(e, x, nlev):
    """Whole closure, forward half + backward half, and the two maps of every level after the forward half."""
    g0, l0 = e.closure(x, CW, SW, TVW)
    l1 = e.closure_forward(x, CW, SW, TVW)
    maps = [_bits(e.level_activation(lvl, layer)) for lvl in range(nlev) for layer in (RELU1_1, RELU5_1)]
    l1 = e.closure_forward(x, CW, SW, TVW)          # (the read-backs used the context: the halves go together)
    g1 = torch.full_like(g0, -12345.0)
    e.closure_backward(x, CW, SW, TVW, grad=g1)
    torch.cuda.synchronize()
    assert np.isfinite(l0.cpu().numpy()).all() and float(g0.abs().max()) > 0
    return [_bits(g0), _bits(l0), _bits(g1), _bits(l1)] + maps


def _assert_same(packed, plain, x, nlev):
    got, ref = _everything(packed, x, nlev), _everything(plain, x, nlev)
    names = ["gradient", "loss row", "gradient of the halves", "loss row of the forward half"]
    names += [f"level {lvl} {m}" for lvl in range(nlev) for m in ("relu1_1", "relu5_1")]
    for what, a, b in zip(names, got, ref):
        assert a.shape == b.shape and np.array_equal(a, b), what
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])
    for m in got[4:]:
        assert m.any()


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_closure_halves_and_maps_are_bitwise_those_of_the_switch_off(pair, geo):
    h, w, nlev = GEOMETRIES[geo]
    _assert_same(*pair, _rgb_job(pair, h, w, nlev), nlev)


MODE_CASES = [(m, g) for g in sorted(GEOMETRIES) for m in ("luminance", "avg_pool", "gram_shift")] + [("guided", "50x76_L2")]


@pytest.mark.parametrize("mode,geo", MODE_CASES)
def test_other_job_modes_are_bitwise_those_of_the_switch_off(pair, mode, geo):
    """luminance: the one-plane conv1_1 and TV forms; gram_shift: relu2_1 .. relu5_1 centred or shifted (the offsets pass reads
    the absmax records the packed front cleared); guided: the guided Gram batch (two levels only: on the 1x1 relu5_1 map of
    an 18x26 level no region but t = 1 has one pixel's worth of mass)."""
    h, w, nlev = GEOMETRIES[geo]
    try:
        if mode == "luminance":
            x = _luminance_job(pair, h, w, nlev)
        elif mode == "avg_pool":
            for e in pair:
                e.configure(nlev, h, w)
                e.set_pooling("avg")
            x = _rgb_job(pair, h, w, nlev)
        elif mode == "gram_shift":
            for e in pair:
                e.configure(nlev, h, w)
                e.set_gram_shift([0.0, "mean", -1.0, "mean", 0.0, 0.5])
            c, s = levels(h, w, nlev, 1), levels(h, w, nlev, 2)
            for e in pair:
                for i in range(nlev):
                    e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
            x = dev(cpu_ref.prepare_img(_start(c[0])))
        else:
            x = _guided_job(pair, h, w, nlev)
        _assert_same(*pair, x, nlev)
    finally:
        for e in pair:
            e.reset_color()
            e.reset_pooling()
            e.configure(nlev, h, w)          # (drops the guidance and the Gram shift)


def test_single_level_256x384_has_nothing_to_pack_but_the_bf16_pieces(pair):
    """One level: the front and the loss terms stay per level; what differs is that S is not cut into bf16 pieces."""
    _assert_same(*pair, _rgb_job(pair, 256, 384, 1), 1)


def test_the_environment_variable_and_the_setter(vgg_weights, monkeypatch):
    from artstyletransfer_amd.engine import StyleEngine
    monkeypatch.setenv("NST_FORWARD_PACK", "0")
    e = StyleEngine(vgg_weights, 0)
    try:
        assert e.lib.nst_ctx_forward_pack(e.ctx) == 0
        assert e.lib.nst_ctx_set_forward_pack(e.ctx, 1) == 0 and e.lib.nst_ctx_forward_pack(e.ctx) == 1
        assert e.lib.nst_ctx_forward_pack(None) == -1
    finally:
        e.close()
