"""CPU: colour preservation (Gatys, Bethge, Hertzmann & Shechtman 2016) on the host - host_image's fp64 restatements
against independent formulations, the C ABI's host-only transfer matrix, validation of preserve_color, the Config field
and its way through Task.  No GPU."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

from artstyletransfer_amd import _lib, host_image


def _img(h, w, seed, tint=(1.0, 1.0, 1.0)):
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3))
    mix = np.array([[0.7, 0.2, 0.1], [0.3, 0.5, 0.2], [0.1, 0.3, 0.6]])      # correlated channels
    return ((base @ mix.T) * np.array(tint)).astype(np.float32)


def _stats(img):
    p = np.asarray(img, np.float64).reshape(-1, 3)
    return p.mean(axis=0), np.cov(p, rowvar=False, bias=True)


def test_color_stats_match_numpy_cov():
    img = _img(31, 47, 1)
    mu, cov = host_image.color_stats(img)
    mu_r, cov_r = _stats(img)
    np.testing.assert_allclose(mu, mu_r, rtol=1e-12)
    np.testing.assert_allclose(cov, cov_r, rtol=1e-12)


def test_recoloured_style_has_the_content_statistics():
    c, s = _img(40, 60, 1), _img(50, 30, 2, tint=(1.0, 0.5, 0.2))
    A, b = host_image.color_transfer_matrix(host_image.color_stats(c), host_image.color_stats(s))
    # in fp64 (the float32 store of color_affine rounds at 6e-8)
    p = np.asarray(s, np.float64).reshape(-1, 3) @ A.T + b
    mu, cov = _stats(p.reshape(s.shape))
    mu_c, cov_c = _stats(c)
    np.testing.assert_allclose(mu, mu_c, rtol=1e-9)
    np.testing.assert_allclose(cov, cov_c, rtol=1e-9)
    np.testing.assert_allclose(host_image.color_affine(s, A, b), p.reshape(s.shape).astype(np.float32), rtol=0, atol=0)


def test_transfer_matrix_against_sqrtm():
    c, s = _img(40, 60, 3), _img(50, 30, 4, tint=(0.3, 0.9, 0.6))
    sc, ss = host_image.color_stats(c), host_image.color_stats(s)
    A, b = host_image.color_transfer_matrix(sc, ss)
    A_ref = np.real(scipy.linalg.sqrtm(sc[1])) @ np.linalg.inv(np.real(scipy.linalg.sqrtm(ss[1])))
    np.testing.assert_allclose(A, A_ref, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(b, sc[0] - A_ref @ ss[0], rtol=1e-8, atol=1e-12)


def test_c_transfer_matrix_is_the_host_restatement():
    """nst_color_transfer_matrix (host-only C, Jacobi) against host_image (numpy eigh), incl. a grey (singular) style."""
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    grey = np.repeat(_img(30, 30, 6)[..., :1], 3, axis=2)
    for s in (_img(50, 30, 5, tint=(1.0, 0.4, 0.7)), grey):
        sc, ss = host_image.color_stats(_img(40, 60, 1)), host_image.color_stats(s)
        args = [np.ascontiguousarray(a, np.float64) for a in (sc[0], sc[1], ss[0], ss[1])]
        A, b = np.zeros(9), np.zeros(3)
        assert lib.nst_color_transfer_matrix(*[a.ctypes.data_as(dp) for a in args], A.ctypes.data_as(dp), b.ctypes.data_as(dp)) == 0
        Ah, bh = host_image.color_transfer_matrix(sc, ss)
        scale = np.abs(Ah).max()
        np.testing.assert_allclose(A.reshape(3, 3), Ah, rtol=0, atol=1e-9 * scale)
        np.testing.assert_allclose(b, bh, rtol=0, atol=1e-9 * scale)


def test_grey_style_histogram_is_finite():
    """A grey style (R = G = B: singular covariance) does not divide by zero: eigenvalues clamped at 1e-10."""
    c = _img(40, 60, 1)
    grey = np.repeat(_img(30, 30, 6)[..., :1], 3, axis=2)
    A, b = host_image.color_transfer_matrix(host_image.color_stats(c), host_image.color_stats(grey))
    out = host_image.color_affine(grey, A, b)
    assert np.isfinite(A).all() and np.isfinite(out).all()
    # the luminance direction (1,1,1) of the grey image is carried; the mean matches the content's
    np.testing.assert_allclose(out.reshape(-1, 3).astype(np.float64).mean(0), host_image.color_stats(c)[0], rtol=1e-6)


def test_recombine_of_the_content_luminance_is_the_content():
    c = _img(23, 41, 7)
    u = 255.0 * (c.astype(np.float64) @ host_image.LUMA)
    np.testing.assert_allclose(host_image.luminance_recombine(u, c.astype(np.float64)), c, rtol=0, atol=1e-6)
    # fp64 throughout (before the float32 store): the round trip is exact to 1e-12
    c64 = c.astype(np.float64)
    yiq = c64 @ host_image.YIQ.T
    yiq[..., 0] = u / 255.0
    np.testing.assert_allclose(yiq @ host_image.YIQ_INV.T, c64, rtol=0, atol=1e-12)
    np.testing.assert_allclose(host_image.YIQ_INV, np.linalg.inv(host_image.YIQ), rtol=0, atol=0)


def test_luminance_params():
    c, s = _img(40, 60, 1), _img(50, 30, 2, tint=(0.5, 0.5, 0.5))
    alpha, beta = host_image.luminance_params(host_image.color_stats(c), host_image.color_stats(s))
    yc = c.astype(np.float64) @ host_image.LUMA
    ys = s.astype(np.float64) @ host_image.LUMA
    matched = alpha * ys + beta
    assert matched.mean() == pytest.approx(yc.mean(), rel=1e-9)
    assert matched.std() == pytest.approx(yc.std(), rel=1e-9)
    np.testing.assert_allclose(host_image.luminance(s, alpha, beta)[0], (255.0 * matched).astype(np.float32))
    flat = np.full((20, 20, 3), 0.4, np.float32)
    alpha, beta = host_image.luminance_params(host_image.color_stats(c), host_image.color_stats(flat))
    assert alpha == 0.0 and beta == pytest.approx(yc.mean(), rel=1e-9)


BAD = ["rgb", "Luminance", "", 1, True, ("luminance",), "hist"]


@pytest.mark.parametrize("bad", BAD)
def test_preserve_color_is_validated_before_any_gpu_work(bad):
    import neural_style_transfer as nst
    from artstyletransfer_amd import config

    async def run():
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (),
                                                  preserve_color=bad):
            pass

    with pytest.raises(ValueError):
        asyncio.run(run())
    with pytest.raises(ValueError):
        config.Config(preserve_color=bad)
    with pytest.raises(ValueError):
        nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam").set_preserve_color(bad)


def test_config_preserve_color_field():
    from artstyletransfer_amd import config
    before = repr(config.Config())
    c = config.Config(preserve_color="luminance")
    assert c.preserve_color == "luminance" and config.Config().preserve_color is None
    assert repr(c) == before and "preserve_color" not in before
    for mode in (None, "luminance", "histogram"):
        config.Config(preserve_color=mode)
        import neural_style_transfer as nst
        nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam").set_preserve_color(mode)


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"preserve_color": "histogram"}, {"device", "preserve_color"}),
    ({"preserve_color": "luminance", "content_layer": 2}, {"device", "preserve_color", "content_layer"}),
])
def test_task_passes_preserve_color_through(monkeypatch, fields, expected):
    from artstyletransfer_amd import config, task_executor as te
    seen = []

    async def fake_nst(pair, *args, **kw):
        seen.append(kw)
        yield 100.0, np.zeros((2, 2, 3), "float32")

    monkeypatch.setattr(te, "neural_style_transfer", fake_nst)

    async def main():
        ex = te.Executor(config.Config(iters_num=1, **fields), gpu_slots=te.GpuSlots(per_gpu=1, n_gpus=1))
        await ex.add_task("t", None)
        await ex.wait_all()

    asyncio.run(main())
    assert len(seen) == 1 and set(seen[0]) == expected
    for k, v in fields.items():
        assert seen[0][k] == v


def test_color_bindings_match_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert "#define NST_COLOR_RGB 0" in hdr and "#define NST_COLOR_LUMINANCE 1" in hdr
    for name in ("nst_job_set_color", "nst_job_color", "nst_color_stats", "nst_color_transfer_matrix", "nst_color_affine",
                 "nst_luminance", "nst_luminance_recombine"):
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", hdr), name
