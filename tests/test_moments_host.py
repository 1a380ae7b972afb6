"""CPU: the moment loss (moment_weight=, moment_terms=, moment_epsilon=) on the host layers - the one normaliser
(artstyletransfer_amd/moment_modes.py) with every accepted form and every refusal, validation before any GPU work, the Config
fields and their way through Task, NeuralStyleTransfer.set_moments down to the device job (a fake in its place), the refusals
together with regions and stripe sharding, and the bindings against the header and the built library.  No GPU."""
import asyncio
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from artstyletransfer_amd import _lib
from artstyletransfer_amd import moment_modes as mm

Z = 0.0
ZEROS = (Z,) * 6
DEFAULT_1E3 = (1e3, 1e3, 1e3, 1e3, Z, 1e3)         # a number: that weight on the job's style maps (default taps 0, 1, 2, 3, 5)
EPS = mm.DEFAULT_EPSILON


# ---- the normaliser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [None, 0, 0.0, [0] * 6, (0.0,) * 6, {}, {2: 0}, np.zeros(6), np.float32(0)])
def test_normaliser_off(value):
    assert mm.normalize_moments(value) is None
    assert mm.normalize_weights(value) == ZEROS


@pytest.mark.parametrize("value,expected", [
    (1e3, DEFAULT_1E3), (1000, DEFAULT_1E3), (np.float64(1e3), DEFAULT_1E3),
    ([1e3, 1e3, 1e3, 1e3, 0, 1e3], DEFAULT_1E3), (np.array(DEFAULT_1E3), DEFAULT_1E3),
    ({0: 1e3, 1: 1e3, 2: 1e3, 3: 1e3, 5: 1e3}, DEFAULT_1E3),
    ({"relu1_1": 1e3, "relu2_1": 1e3, "relu3_1": 1e3, "relu4_1": 1e3, "relu5_1": 1e3}, DEFAULT_1E3),
    ({"conv1_1": 1e3, 1: 1e3, "conv3_1": 1e3, 3: 1e3, "conv5_1": 1e3}, DEFAULT_1E3),      # names of the pre-ReLU flavour, mixed with indices
    ({np.int64(5): 0.25}, (Z, Z, Z, Z, Z, 0.25)), ({"relu3_1": 2}, (Z, Z, 2.0, Z, Z, Z)),
    ([0, 0, 0, 0, 0, 7], (Z, Z, Z, Z, Z, 7.0)),
])
def test_normaliser_accepts(value, expected):
    assert mm.normalize_weights(value) == expected
    assert mm.normalize_moments(value) == (expected, expected, EPS)
    assert mm.normalize_moments(value, "both", 1e-3) == (expected, expected, 1e-3)
    assert mm.normalize_moments(value, "mean") == (expected, ZEROS, EPS)
    assert mm.normalize_moments(value, "std") == (ZEROS, expected, EPS)


def test_a_number_goes_on_the_style_maps_of_the_job():
    assert mm.normalize_weights(2.0, style_indices=(1, 4)) == (Z, 2.0, Z, Z, 2.0, Z)
    assert mm.normalize_weights(2.0, style_indices=range(6)) == (2.0,) * 6
    assert mm.normalize_moments(2.0, "mean", style_indices=[5, 0, 0]) == ((2.0, Z, Z, Z, Z, 2.0), ZEROS, EPS)
    # six numbers and a dict are by map index: a positive weight outside the style set is refused where the set is known
    assert mm.normalize_weights([1, 0, 0, 0, 0, 0], style_indices=(0, 1)) == (1.0, Z, Z, Z, Z, Z)
    for bad in ([0, 0, 1, 0, 0, 0], {4: 1.0}, {"conv4_2": 1.0}):
        with pytest.raises(ValueError, match="not a style map"):
            mm.normalize_weights(bad, style_indices=(0, 1))
        assert mm.normalize_weights(bad) is not None                      # (not checked while the set is not known)
    assert mm.normalize_weights({4: 0.0}, style_indices=(0, 1)) == ZEROS      # a zero weight names no map


BAD_WEIGHTS = [float("nan"), float("inf"), -1.0, -float("inf"), "mean", "", b"1", True, 1j, [0] * 5, [0] * 7, (),
               [0, 0, float("nan"), 0, 0, 0], [0, 0, -1e-9, 0, 0, 0], [0, 0, None, 0, 0, 0], [0, 0, True, 0, 0, 0], [0, 0, "1", 0, 0, 0],
               {6: 1.0}, {-1: 1.0}, {"relu6_1": 1.0}, {1.5: 1.0}, {True: 1.0}, {0: float("inf")}, {0: -1}, {0: "1"}, {0: None},
               {1, 2, 3, 4, 5, 6}, object()]


# (a bare object's repr carries its address: an id of its own, so that the test has one name in every run)
@pytest.mark.parametrize("value", BAD_WEIGHTS, ids=["object()" if type(v) is object else repr(v)[:30] for v in BAD_WEIGHTS])
def test_normaliser_refuses_weights(value):
    with pytest.raises(ValueError):
        mm.normalize_moments(value)
    with pytest.raises(ValueError):
        mm.normalize_weights(value)


@pytest.mark.parametrize("terms", ["", "Both", "variance", None, 0, ("mean",), b"std"])
def test_normaliser_refuses_terms(terms):
    for w in (None, 1.0):                                  # validated whether the term is on or off
        with pytest.raises(ValueError, match="moment_terms"):
            mm.normalize_moments(w, terms)


@pytest.mark.parametrize("eps", [0, 0.0, -1e-5, float("nan"), float("inf"), None, "1e-5", True, [1e-5]])
def test_normaliser_refuses_epsilon(eps):
    for w in (None, 1.0):
        with pytest.raises(ValueError, match="moment_epsilon"):
            mm.normalize_moments(w, "both", eps)
    with pytest.raises(ValueError, match="moment_epsilon"):
        mm.check_setting(1.0, 1.0, eps)


def test_map_names_follow_the_flavour():
    assert mm.normalize_weights({"relu5_1": 3}, use_relu=True) == (Z,) * 5 + (3.0,)
    assert mm.normalize_weights({"conv5_1": 3}, use_relu=False) == (Z,) * 5 + (3.0,)
    with pytest.raises(ValueError):
        mm.normalize_weights({"conv5_1": 3}, use_relu=True)
    with pytest.raises(ValueError):
        mm.normalize_weights({"relu5_1": 3}, use_relu=False)
    assert mm.NUM_MAPS == 6 and mm.TERMS == ("both", "mean", "std") and mm.DEFAULT_EPSILON == 1e-5


def test_the_explicit_form_of_the_engine():
    assert mm.check_setting(None, None) is None and mm.check_setting(0, [0] * 6, 1e-3) is None
    assert mm.check_setting(1.0, None, style_indices=(0, 2)) == ((1.0, Z, 1.0, Z, Z, Z), ZEROS, EPS)
    assert mm.check_setting({0: 2}, 3.0, 1e-4, style_indices=(0, 2)) == ((2.0, Z, Z, Z, Z, Z), (3.0, Z, 3.0, Z, Z, Z), 1e-4)
    with pytest.raises(ValueError):
        mm.check_setting(None, {1: 1.0}, style_indices=(0, 2))


def test_regions_and_stripes_together_with_the_term_raise():
    on = mm.normalize_moments(1.0)
    mm.check_exclusive(None, regions=object(), stripes=True)                       # off: nothing to refuse
    mm.check_exclusive(on)
    with pytest.raises(ValueError, match="content_regions"):
        mm.check_exclusive(on, regions=object())
    with pytest.raises(ValueError, match="stripe sharding"):
        mm.check_exclusive(on, stripes=True)


# ---- before any GPU work ----------------------------------------------------------------------------------------------------
LABELS = np.zeros((8, 8), np.int64)


@pytest.mark.parametrize("kw", [{"moment_weight": float("nan")}, {"moment_weight": -1.0}, {"moment_weight": [1] * 5},
                                {"moment_weight": {"relu9_9": 1}}, {"moment_weight": {"conv5_1": 1}},      # (use_relu=True: no such name)
                                {"moment_weight": 1.0, "moment_terms": "variance"}, {"moment_terms": "variance"},
                                {"moment_weight": 1.0, "moment_epsilon": 0.0}, {"moment_epsilon": -1.0},
                                {"moment_weight": 1.0, "content_regions": LABELS, "style_regions": LABELS}])
def test_moments_are_validated_before_any_gpu_work(kw, monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import config, engine, neural_nets

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the moment loss was validated")

    monkeypatch.setattr(engine.StyleEngine, "__init__", no_engine)
    monkeypatch.setattr(neural_nets, "_weights_cache", [])

    async def run():
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (), **kw):
            pass

    with pytest.raises(ValueError):
        asyncio.run(run())
    with pytest.raises(ValueError):
        config.Config(**kw)
    if "content_regions" not in kw and not isinstance(kw.get("moment_weight"), dict):
        with pytest.raises(ValueError):
            nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam").set_moments(**kw)


def test_a_weight_outside_the_jobs_style_set_is_refused_before_any_gpu_work(monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import engine, neural_nets

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the moment loss was validated")

    monkeypatch.setattr(engine.StyleEngine, "__init__", no_engine)
    monkeypatch.setattr(neural_nets, "_weights_cache", [])

    async def run(**kw):
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (), **kw):
            pass

    with pytest.raises(ValueError, match="not a style map"):
        asyncio.run(run(moment_weight={"conv4_2": 1.0}))                       # the default style set leaves map 4 out
    with pytest.raises(ValueError, match="not a style map"):
        asyncio.run(run(moment_weight=[1, 1, 1, 0, 0, 0], style_layers=[0, 1]))


def test_engine_setter_validates_before_the_context():
    from artstyletransfer_amd import engine
    eng = object.__new__(engine.StyleEngine)              # no context: anything that reached it would fail differently
    for args in ((float("nan"),), (-1.0,), ([1] * 5,), (1.0, "x"), (1.0, 1.0, 0.0), ({4: 1.0},), (None, [0, 0, 0, 0, 1, 0])):
        with pytest.raises(ValueError):
            eng.set_moments(*args)
    with pytest.raises(ValueError):
        eng.moments(torch.zeros((1, 64, 4, 4)), epsilon=0.0)


def test_process_refuses_the_term_together_with_regions(monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl

    def no_job(*a, **k):
        raise AssertionError("a device job was made before the setting was checked against the regions")

    monkeypatch.setattr(impl, "_make_job", no_job)
    monkeypatch.setattr(math_utils, "prepare_model", lambda name, device: None)
    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", [np.zeros((256, 384, 3), np.float32)], "adam")
    job.set_moments(1e3)
    job.set_regions(LABELS, LABELS)

    async def run():
        async for _ in job.process([np.zeros((256, 384, 3), np.float32)], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    with pytest.raises(ValueError, match="moment_weight"):
        asyncio.run(run())


def test_moment_fields_are_keyword_only_in_the_job_driver():
    import neural_style_transfer as nst
    pars = inspect.signature(nst.neural_style_transfer).parameters
    for name, default in (("moment_weight", None), ("moment_terms", "both"), ("moment_epsilon", 1e-5)):
        assert pars[name].kind is inspect.Parameter.KEYWORD_ONLY and pars[name].default == default
    for cls in (nst.LossBuilder, nst.NeuralStyleTransfer):
        assert list(inspect.signature(cls.set_moments).parameters)[1:] == ["moment_weight", "moment_terms", "moment_epsilon"]
    from artstyletransfer_amd import engine
    assert list(inspect.signature(engine.StyleEngine.set_moments).parameters)[1:] == ["mean_w", "std_w", "epsilon"]
    assert list(inspect.signature(engine.StyleEngine.moments).parameters)[1:] == ["f", "epsilon"]
    assert hasattr(engine.StyleEngine, "moment_losses")


# ---- Config / Task ------------------------------------------------------------------------------------------------------------
def test_config_moment_fields():
    from artstyletransfer_amd import config
    before = repr(config.Config())
    c = config.Config(moment_weight={"relu1_1": 5, 2: 1e3}, moment_terms="std", moment_epsilon=1e-4)
    assert (c.moment_weight, c.moment_terms, c.moment_epsilon) == ({"relu1_1": 5, 2: 1e3}, "std", 1e-4)
    d = config.Config()
    assert (d.moment_weight, d.moment_terms, d.moment_epsilon) == (None, "both", 1e-5)
    assert repr(c) == before and "moment" not in before
    assert config.Config(*range(13)).moment_weight is None
    assert config.Config(moment_weight={"conv5_1": 1}, use_relu=False).moment_weight == {"conv5_1": 1}
    import config as dropin                       # the drop-in module name re-exports the same class
    assert dropin.Config(moment_weight=3).moment_weight == 3


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"moment_weight": 1e3}, {"device", "moment_weight", "moment_terms", "moment_epsilon"}),
    ({"moment_weight": 0}, {"device", "moment_weight", "moment_terms", "moment_epsilon"}),      # handed on as given; the driver normalises it to off
    ({"moment_terms": "mean"}, {"device"}),                                                   # no weight: nothing to hand on
    ({"moment_weight": [1, 0, 0, 0, 0, 0], "moment_terms": "mean", "gram_shift": "mean"},
     {"device", "moment_weight", "moment_terms", "moment_epsilon", "gram_shift"}),
])
def test_task_passes_the_moment_fields_through(monkeypatch, fields, expected):
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
    if "moment_weight" in fields:
        assert seen[0]["moment_weight"] == fields["moment_weight"]
        assert seen[0]["moment_terms"] == fields.get("moment_terms", "both") and seen[0]["moment_epsilon"] == 1e-5


@pytest.mark.parametrize("args,expected", [
    ((None,), {}), ((0,), {}), (([0.0] * 6, "std"), {}),
    ((1e3,), {"moments": (DEFAULT_1E3, DEFAULT_1E3, EPS)}),
    ((1e3, "mean", 1e-3), {"moments": (DEFAULT_1E3, ZEROS, 1e-3)}),
    (({0: 2, "relu3_1": 4}, "std"), {"moments": (ZEROS, (2.0, Z, 4.0, Z, Z, Z), EPS)}),
])
def test_process_hands_the_moments_to_the_job(monkeypatch, args, expected):
    """NeuralStyleTransfer.set_moments reaches the device job (a fake in its place), normalised against the job's style set;
    off passes nothing."""
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []
    # (the real one takes what process passes: every key the table can emit, consumed by job_settings.apply or by _DeviceJob)
    from artstyletransfer_amd import job_settings
    assert "moments" in job_settings.KEYS and set(job_settings.KEYS) <= set(job_settings.APPLY_ORDER) | set(impl._DeviceJob.CONSUMES)
    assert inspect.signature(impl._make_job).parameters["settings"].kind is inspect.Parameter.VAR_KEYWORD

    class FakeJob:
        def close(self):
            pass

    def fake_make_job(device, optimizer_name, style_imgs, content_imgs, init_img, lr_start, **extra):
        seen.append(extra)
        return FakeJob()

    monkeypatch.setattr(impl, "_make_job", fake_make_job)
    monkeypatch.setattr(math_utils, "prepare_model", lambda name, device: None)
    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", [], "adam")
    job.set_moments(*args)

    async def run():
        async for _ in job.process([np.zeros((256, 384, 3), np.float32)], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    asyncio.run(run())
    assert seen == [expected]


def test_process_puts_a_number_on_the_style_maps_of_its_taps(monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def close(self):
            pass

    monkeypatch.setattr(impl, "_make_job", lambda *a, **extra: seen.append(extra) or FakeJob())
    monkeypatch.setattr(math_utils, "prepare_model", lambda name, device: None)
    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", [], "adam")
    job.set_feature_maps(4, [1, 4])
    job.set_moments(2.0, "mean")

    async def run():
        async for _ in job.process([np.zeros((256, 384, 3), np.float32)], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    asyncio.run(run())
    assert seen[0]["moments"] == ((Z, 2.0, Z, Z, 2.0, Z), ZEROS, EPS)
    job.set_moments({0: 1.0})                              # map 0 is not a style map of these taps: refused in process
    with pytest.raises(ValueError, match="not a style map"):
        asyncio.run(run())


# ---- stripe sharding ----------------------------------------------------------------------------------------------------------
def test_stripe_sharding_refuses_the_setting():
    """PixelOptimizer.shard_stripes on an engine that carries the setting: ValueError before any stripe engine is made."""
    from artstyletransfer_amd import engine, style_modes

    class FakeEngine:
        levels = 1
        layer_weights = style_modes.UNIT_WEIGHTS
        laplacian = None
        gram_shift = None
        moment_loss = (DEFAULT_1E3, DEFAULT_1E3, EPS)
        channels = 3

        def guidance(self, level):
            return 0, (), None

    opt = object.__new__(engine.PixelOptimizer)
    opt.engine = FakeEngine()
    with pytest.raises(ValueError, match="moment_weight cannot be combined with stripe sharding"):
        opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
    src = inspect.getsource(engine.PixelOptimizer.shard_stripes)
    assert src.index("_mom.check_exclusive") < src.index("StyleEngine(weights")


def test_pooled_engine_is_reset():
    """return_engine undoes the job settings through StyleEngine.reset_job_settings, which switches the moment loss off."""
    from artstyletransfer_amd import engine, neural_nets
    assert "eng.reset_job_settings()" in inspect.getsource(neural_nets.return_engine)
    calls = []
    fake = type("RecordingEngine", (), {"__getattr__": lambda self, method: lambda: calls.append(method)})()
    engine.StyleEngine.reset_job_settings(fake)
    assert "reset_moments" in calls


# ---- bindings -------------------------------------------------------------------------------------------------------------------
def test_moment_bindings_match_header_and_library():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert re.search(r"int nst_job_set_moments\(nst_ctx\* ctx, const float mean_w\[6\], const float std_w\[6\], float epsilon\);", hdr)
    assert re.search(r"int nst_job_moments\(const nst_ctx\* ctx, float mean_w\[6\], float std_w\[6\], float\* epsilon\);", hdr)
    assert re.search(r"int nst_job_moment_losses\(nst_ctx\* ctx, float\* out[^;]*void\* stream\);", hdr)
    assert re.search(r"int nst_moments\(nst_ctx\* ctx, const float\* f, int C, int h, int w, float epsilon, float\* mean_out, "
                     r"float\* std_out, void\* stream\);", hdr)
    fp = C.POINTER(C.c_float)
    assert _lib.SYMBOLS["nst_job_set_moments"] == (C.c_int, [C.c_void_p, fp, fp, C.c_float])
    assert _lib.SYMBOLS["nst_job_moments"] == (C.c_int, [C.c_void_p, fp, fp, fp])
    assert _lib.SYMBOLS["nst_job_moment_losses"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["nst_moments"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p,
                                                     C.c_void_p, C.c_void_p])
    lib = C.CDLL(_lib.LIB_PATH)                      # the built library exports all four
    for name in ("nst_job_set_moments", "nst_job_moments", "nst_job_moment_losses", "nst_moments"):
        assert hasattr(lib, name), name
    # without a context: an error code, no crash (bind() refuses a null context)
    lib.nst_job_set_moments.restype = C.c_int
    lib.nst_job_set_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
    lib.nst_job_moments.restype = C.c_int
    lib.nst_job_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.nst_job_set_moments(None, None, None, 1e-5) < 0 and lib.nst_job_moments(None, None, None, None) < 0
