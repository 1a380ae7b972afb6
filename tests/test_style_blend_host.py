"""CPU: per-layer style weights and the blend of several style images on the host layers - validation and normalisation
(artstyletransfer_amd/style_modes.py), the Config fields and their way through Task, ValueError before any GPU work, and the
binding of nst_job_set_style_weights / nst_job_style_weights / nst_level_set_targets_blend against the header and the built
library.  No GPU."""
import asyncio
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from artstyletransfer_amd import _lib
from artstyletransfer_amd import style_modes as sm

BAD_WEIGHTS = [[1] * 5, [1] * 7, [1, 1, 1, 1, 1, -1], [1, 1, float("nan"), 1, 1, 1], [1, float("inf"), 1, 1, 1, 1], [0] * 6,
               [0, 0, 0, 0, 2.0, 0], {6: 1.0}, {"relu9_9": 1.0}, {0: -1.0}, {0: "2"}, "111111", 1.0, [1, 1, 1, 1, 1, True]]
# (K, blend)
BAD_BLENDS = [(2, [1.0]), (2, [1.0, 1.0, 1.0]), (2, [1.0, -1.0]), (2, [1.0, float("nan")]), (2, [0.0, 0.0]),
              (2, [[1, 1, 0, 1, 1, 1], [1, 1, 0, 1, 1, 1]]), (2, [[1] * 6, [1] * 5]), (2, "ab"), (2, {0: 1})]


def test_layer_weights_normalisation():
    assert sm.check_style_layer_weights(None) == (1.0,) * 6
    assert sm.check_style_layer_weights([1, 0.5, 0, 2, 1, 0.25]) == (1.0, 0.5, 0.0, 2.0, 1.0, 0.25)
    assert sm.check_style_layer_weights(np.array([1, 0.5, 0, 2, 1, 0.25], np.float32)) == (1.0, 0.5, 0.0, 2.0, 1.0, 0.25)
    assert sm.check_style_layer_weights({0: 2.0}) == (2.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    assert sm.check_style_layer_weights({"relu5_1": 0.5, "conv4_2": 3, 1: 0}) == (1.0, 0.0, 1.0, 1.0, 3.0, 0.5)
    assert sm.check_style_layer_weights({"conv5_1": 0.5}, use_relu=False)[5] == 0.5
    with pytest.raises(ValueError):
        sm.check_style_layer_weights({"relu5_1": 0.5}, use_relu=False)       # the other flavour's name
    # the style set decides which maps must carry weight
    assert sm.check_style_layer_weights([0, 0, 0, 0, 2.0, 0], style_indices=(4,)) == (0.0, 0.0, 0.0, 0.0, 2.0, 0.0)
    assert sm.is_unit(None) and sm.is_unit([1] * 6) and not sm.is_unit([1, 1, 1, 1, 1, 2])


@pytest.mark.parametrize("bad", BAD_WEIGHTS, ids=[str(i) for i in range(len(BAD_WEIGHTS))])
def test_bad_layer_weights_raise(bad):
    with pytest.raises(ValueError):
        sm.check_style_layer_weights(bad)


def test_blend_normalisation():
    assert sm.check_style_blend([0.5, 0.5], 2) == ((0.5,) * 6, (0.5,) * 6)
    assert sm.check_style_blend(None, 3) == ((1.0,) * 6,) * 3
    B = sm.check_style_blend([[1, 0.6, 0, 0, 0, 0], [0, 0.4, 1, 1, 0, 0.5], [0, 0, 0, 0, 0, 1.5]], 3)     # (map 4: not in the set)
    bh = sm.normalized_blend(B)
    assert bh.dtype == np.float32 and bh.shape == (3, 6)
    # b^ = B / column sum in fp64 from the float32 entries, then float32; a column without weight stays zero
    b32 = np.asarray(B, np.float32).astype(np.float64)
    np.testing.assert_array_equal(bh[:, 1], (b32[:, 1] / b32[:, 1].sum()).astype(np.float32))
    np.testing.assert_array_equal(bh[:, 5], np.array([0, 0.5 / 2.0, 1.5 / 2.0], np.float32))
    assert not bh[:, 4].any()
    # K = 1: whatever the positive entries, b^ is exactly 1
    assert (sm.normalized_blend(sm.check_style_blend([0.37], 1)) == 1.0).all()
    # a zero column is an error only for a map of the style set
    sm.check_style_blend([[1, 1, 0, 1, 1, 1]] * 2, 2, style_indices=(0, 1))
    for k in (0, 9, True, 2.0, None):
        with pytest.raises(ValueError):
            sm.check_style_blend(None, k)


@pytest.mark.parametrize("k,bad", BAD_BLENDS, ids=[str(i) for i in range(len(BAD_BLENDS))])
def test_bad_blends_raise(k, bad):
    with pytest.raises(ValueError):
        sm.check_style_blend(bad, k)


def test_style_settings_are_validated_before_any_gpu_work(monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import config, engine, neural_nets

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the style settings were validated")

    monkeypatch.setattr(engine.StyleEngine, "__init__", no_engine)
    monkeypatch.setattr(neural_nets, "_weights_cache", [])
    img = np.zeros((32, 32, 3), np.float32)

    def run(**kw):
        async def go():
            async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (), **kw):
                pass
        asyncio.run(go())

    for kw in (dict(style_layer_weights=[1] * 5), dict(style_layer_weights=[0] * 6), dict(style_layer_weights={0: -1}),
               dict(style_layer_weights=[0, 0, 0, 0, 1, 0]),                       # no map of the default style set
               dict(style_layer_weights=[1, 0, 0, 0, 0, 0], style_layers=[1, 2]),  # no map of the chosen style set
               dict(extra_styles=[img], style_blend=[1.0]), dict(extra_styles=[img], style_blend=[1.0, 1.0, 1.0]),
               dict(style_blend=[1.0, 1.0]), dict(extra_styles=[img], style_blend=[0.0, 0.0]),
               dict(extra_styles=[img], style_blend=[1.0, float("inf")]), dict(extra_styles=[img] * 8),
               dict(extra_styles=[np.zeros((32, 32), np.float32)])):
        with pytest.raises(ValueError):
            run(**kw)
    for kw in (dict(style_layer_weights=[1] * 5), dict(style_layer_weights=[0] * 6), dict(style_blend=[1.0, 1.0]),
               dict(extra_styles=[img], style_blend=[1.0, -1.0])):
        with pytest.raises(ValueError):
            config.Config(**kw)
    job = nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam")
    with pytest.raises(ValueError):
        job.set_style_layer_weights([1] * 5)
    with pytest.raises(ValueError):
        job.set_style_blend([[img]], [1.0])
    with pytest.raises(ValueError):
        job.set_style_blend([[img]] * 8)
    # the engine's own setters validate before they touch the context
    eng = object.__new__(engine.StyleEngine)
    eng.taps = engine.DEFAULT_TAPS
    with pytest.raises(ValueError):
        eng.set_style_weights([1, 1, 1, 1, 1, -1])


def test_style_settings_are_keyword_only_in_the_job_driver():
    import neural_style_transfer as nst
    for name in ("extra_styles", "style_blend", "style_layer_weights"):
        par = inspect.signature(nst.neural_style_transfer).parameters[name]
        assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None


def test_config_style_fields():
    from artstyletransfer_amd import config
    before = repr(config.Config())
    c = config.Config(extra_styles=[np.zeros((4, 4, 3), np.float32)], style_blend=[1, 3], style_layer_weights={0: 2.0})
    assert c.style_blend == [1, 3] and c.style_layer_weights == {0: 2.0} and len(c.extra_styles) == 1
    d = config.Config()
    assert d.extra_styles is None and d.style_blend is None and d.style_layer_weights is None
    assert repr(c) == before
    assert config.Config(*range(13)).style_blend is None


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"style_layer_weights": [1, 2, 1, 1, 1, 1]}, {"device", "style_layer_weights"}),
    ({"extra_styles": [np.zeros((4, 4, 3), np.float32)], "style_blend": np.ones((2, 6))}, {"device", "extra_styles", "style_blend"}),
    ({"extra_styles": [np.zeros((4, 4, 3), np.float32)], "pooling": "avg"}, {"device", "extra_styles", "pooling"}),
])
def test_task_passes_style_settings_through(monkeypatch, fields, expected):
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
    for k in expected - {"device"}:
        assert seen[0][k] is fields[k]


def test_process_hands_the_style_settings_to_the_job(monkeypatch):
    """set_style_layer_weights / set_style_blend reach the device job (a fake in its place); unit weights and no extra style
    pass nothing: the default job."""
    import torch
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def close(self):
            pass

    def fake_make_job(device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, **extra):
        seen.append(extra)
        return FakeJob()

    monkeypatch.setattr(impl, "_make_job", fake_make_job)
    monkeypatch.setattr(math_utils, "prepare_model", lambda name, device: None)

    def run(job):
        async def go():
            async for _ in job.process(["c"], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
                pass
        asyncio.run(go())

    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", ["s0"], "adam")
    job.set_style_layer_weights([1] * 6)
    job.set_style_blend(None, None)
    run(job)
    job.set_style_layer_weights({5: 0.5})
    job.set_style_blend([["b0"]], [1, 3])
    run(job)
    assert seen[0] == {}
    assert seen[1] == {"style_weights": (1.0, 1.0, 1.0, 1.0, 1.0, 0.5), "blend": ([["b0"]], ((1.0,) * 6, (3.0,) * 6))}
    # against the style set of the job: map 5 alone carries weight, the style set leaves it out
    job.set_feature_maps(4, [0, 1])
    job.set_style_layer_weights([0, 0, 0, 0, 0, 1])
    with pytest.raises(ValueError):
        run(job)
    # an extra style needs one image per level
    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", ["s0", "s1"], "adam")
    job.set_style_blend([["b0"]], None)
    with pytest.raises(ValueError):
        run(job)


def test_style_bindings_match_header_and_library():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert "#define NST_MAX_STYLES 8" in hdr and _lib.NST_MAX_STYLES == sm.MAX_STYLES == 8
    assert re.search(r"int nst_job_set_style_weights\(nst_ctx\* ctx, const float w\[6\]\);", hdr)
    assert re.search(r"int nst_job_style_weights\(const nst_ctx\* ctx, float w\[6\]\);", hdr)
    assert re.search(r"int nst_level_set_targets_blend\(nst_ctx\* ctx, int level, const float\* content, int K, const float\* const\* styles,\s*"
                     r"const int\* hs, const int\* ws, const float\* blend( /\*[^/]*\*/)?, void\* stream\);", hdr)
    fp, vp, ip = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int)
    assert _lib.SYMBOLS["nst_job_set_style_weights"] == (C.c_int, [vp, fp])
    assert _lib.SYMBOLS["nst_job_style_weights"] == (C.c_int, [vp, fp])
    assert _lib.SYMBOLS["nst_level_set_targets_blend"] == (C.c_int, [vp, C.c_int, vp, C.c_int, C.POINTER(vp), ip, ip, fp, vp])
    lib = C.CDLL(_lib.LIB_PATH)                      # the built library exports all three
    for name in ("nst_job_set_style_weights", "nst_job_style_weights", "nst_level_set_targets_blend"):
        assert hasattr(lib, name), name
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SYMBOLS[name]
    # without a context: an error code, no crash (bind() refuses a null context)
    w = (C.c_float * 6)(*[1.0] * 6)
    assert lib.nst_job_set_style_weights(None, w) < 0 and lib.nst_job_style_weights(None, w) < 0
    assert lib.nst_level_set_targets_blend(None, 0, None, 1, None, None, None, None, None) < 0
