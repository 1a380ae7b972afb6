"""CPU: the Gram shift option (gram_shift=) on the host layers - the one normaliser (artstyletransfer_amd/gram_modes.py) with
every accepted spelling and every refusal, validation before any GPU work, the Config field and its way through Task,
NeuralStyleTransfer.set_gram_shift down to the device job (a fake in its place), the refusals together with regions and
stripe sharding, and the bindings against the header and the built library.  No GPU."""
import ast
import asyncio
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from artstyletransfer_amd import _lib
from artstyletransfer_amd import gram_modes as gm

Z = 0.0
ALL_M1 = ((-1.0,) * 6, 0)
ALL_MEAN = ((Z,) * 6, 63)
MIXED = ((Z, Z, -1.0, Z, Z, Z), 0b001001)          # maps 0 and 3 centred, map 2 shifted by -1


# ---- the normaliser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value,expected", [
    (None, None), (0, None), (0.0, None), ([0] * 6, None), ((0.0,) * 6, None), ({}, None), ({2: 0}, None), (np.zeros(6), None),
    (-1, ALL_M1), (-1.0, ALL_M1), (np.float32(-1), ALL_M1), ([-1] * 6, ALL_M1), (np.full(6, -1.0), ALL_M1),
    ({i: -1 for i in range(6)}, ALL_M1),
    ("mean", ALL_MEAN), (["mean"] * 6, ALL_MEAN), ({i: "mean" for i in range(6)}, ALL_MEAN),
    ({"relu1_1": "mean", "relu2_1": "mean", "relu3_1": "mean", "relu4_1": "mean", "conv4_2": "mean", "relu5_1": "mean"}, ALL_MEAN),
    (["mean", 0, -1, "mean", 0, 0], MIXED), (("mean", 0.0, -1.0, "mean", 0.0, 0.0), MIXED),
    ({0: "mean", 2: -1, 3: "mean"}, MIXED), ({"relu1_1": "mean", "relu3_1": -1.0, "relu4_1": "mean"}, MIXED),
    ({"conv1_1": "mean", "conv3_1": -1.0, 3: "mean"}, MIXED),                       # names of the pre-ReLU flavour, mixed with indices
    ({np.int64(0): "mean", 2: np.float64(-1), 3: "mean", 5: 0}, MIXED),
    ({5: 0.25}, ((Z, Z, Z, Z, Z, 0.25), 0)),
])
def test_normaliser_accepts(value, expected):
    assert gm.normalize_gram_shift(value) == expected


BAD = [float("nan"), float("inf"), -float("inf"), "median", "Mean", "", b"mean", True, 1j, [0] * 5, [0] * 7, (), ["mean"] * 5,
       [0, 0, float("nan"), 0, 0, 0], [0, 0, "centre", 0, 0, 0], [0, 0, None, 0, 0, 0], [0, 0, True, 0, 0, 0],
       {6: 1.0}, {-1: 1.0}, {"relu6_1": 1.0}, {1.5: 1.0}, {True: 1.0}, {0: float("inf")}, {0: "avg"}, {0: None},
       {1, 2, 3, 4, 5, 6}, object()]


# (a bare object's repr carries its address: an id of its own, so that the test has one name in every run)
@pytest.mark.parametrize("value", BAD, ids=["object()" if type(v) is object else repr(v)[:30] for v in BAD])
def test_normaliser_refuses(value):
    with pytest.raises(ValueError):
        gm.normalize_gram_shift(value)


def test_map_names_follow_the_flavour():
    assert gm.normalize_gram_shift({"relu5_1": -1}, use_relu=True) == ((Z,) * 5 + (-1.0,), 0)
    assert gm.normalize_gram_shift({"conv5_1": -1}, use_relu=False) == ((Z,) * 5 + (-1.0,), 0)
    with pytest.raises(ValueError):
        gm.normalize_gram_shift({"conv5_1": -1}, use_relu=True)
    with pytest.raises(ValueError):
        gm.normalize_gram_shift({"relu5_1": -1}, use_relu=False)
    assert gm.NUM_MAPS == 6 and gm.MEAN == "mean"


def test_regions_and_stripes_together_with_a_shift_raise():
    gm.check_exclusive(None, regions=object(), stripes=True)                       # off: nothing to refuse
    gm.check_exclusive(ALL_M1)
    with pytest.raises(ValueError, match="content_regions"):
        gm.check_exclusive(ALL_M1, regions=object())
    with pytest.raises(ValueError, match="stripe sharding"):
        gm.check_exclusive(ALL_MEAN, stripes=True)


# ---- before any GPU work ----------------------------------------------------------------------------------------------------
LABELS = np.zeros((8, 8), np.int64)


@pytest.mark.parametrize("kw", [{"gram_shift": float("nan")}, {"gram_shift": "median"}, {"gram_shift": [0] * 5},
                                {"gram_shift": {"relu9_9": 1}}, {"gram_shift": {"conv5_1": -1}},      # (use_relu=True: no such name)
                                {"gram_shift": -1, "content_regions": LABELS, "style_regions": LABELS}])
def test_gram_shift_is_validated_before_any_gpu_work(kw, monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import config, engine, neural_nets

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the Gram shift was validated")

    monkeypatch.setattr(engine.StyleEngine, "__init__", no_engine)
    monkeypatch.setattr(neural_nets, "_weights_cache", [])

    async def run():
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (), **kw):
            pass

    with pytest.raises(ValueError):
        asyncio.run(run())
    with pytest.raises(ValueError):
        config.Config(**kw)
    if len(kw) == 1 and not isinstance(kw["gram_shift"], dict):
        with pytest.raises(ValueError):
            nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam").set_gram_shift(kw["gram_shift"])
        eng = object.__new__(engine.StyleEngine)                  # the engine's own setter validates before it touches the context
        with pytest.raises(ValueError):
            eng.set_gram_shift(kw["gram_shift"])


def test_engine_setter_checks_the_mask_before_the_context():
    from artstyletransfer_amd import engine
    eng = object.__new__(engine.StyleEngine)
    for shift, mask in (((0.0,) * 6, 64), ((0.0,) * 6, -1), ((1.0, 0, 0, 0, 0, 0), 1)):
        with pytest.raises(ValueError):
            eng.set_gram_shift(shift, mask)


def test_process_refuses_a_shift_together_with_regions(monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl

    def no_job(*a, **k):
        raise AssertionError("a device job was made before the setting was checked against the regions")

    monkeypatch.setattr(impl, "_make_job", no_job)
    monkeypatch.setattr(math_utils, "prepare_model", lambda name, device: None)
    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", [np.zeros((256, 384, 3), np.float32)], "adam")
    job.set_gram_shift("mean")
    job.set_regions(LABELS, LABELS)

    async def run():
        async for _ in job.process([np.zeros((256, 384, 3), np.float32)], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    with pytest.raises(ValueError, match="gram_shift"):
        asyncio.run(run())


def test_gram_shift_is_keyword_only_in_the_job_driver():
    import neural_style_transfer as nst
    par = inspect.signature(nst.neural_style_transfer).parameters["gram_shift"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
    for cls in (nst.LossBuilder, nst.NeuralStyleTransfer):
        assert hasattr(cls, "set_gram_shift")
    from artstyletransfer_amd import engine
    assert list(inspect.signature(engine.StyleEngine.set_gram_shift).parameters)[1:] == ["shift", "center_mask"]


# ---- Config / Task ------------------------------------------------------------------------------------------------------------
def test_config_gram_shift_field():
    from artstyletransfer_amd import config
    before = repr(config.Config())
    c = config.Config(gram_shift={"relu1_1": "mean", 2: -1})
    assert c.gram_shift == {"relu1_1": "mean", 2: -1}
    assert config.Config().gram_shift is None
    assert repr(c) == before and "gram_shift" not in before
    assert config.Config(*range(13)).gram_shift is None
    assert config.Config(gram_shift={"conv5_1": -1}, use_relu=False).gram_shift == {"conv5_1": -1}
    import config as dropin                       # the drop-in module name re-exports the same class
    assert dropin.Config(gram_shift="mean").gram_shift == "mean"


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"gram_shift": -1.0}, {"device", "gram_shift"}),
    ({"gram_shift": 0}, {"device", "gram_shift"}),                               # handed on as given; the driver normalises it to off
    ({"gram_shift": "mean", "pooling": "avg"}, {"device", "gram_shift", "pooling"}),
    ({"gram_shift": ["mean", 0, -1, "mean", 0, 0], "laplacian_weight": 5.0}, {"device", "gram_shift", "laplacian_weight", "laplacian_pool"}),
])
def test_task_passes_gram_shift_through(monkeypatch, fields, expected):
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
    if "gram_shift" in fields:
        assert seen[0]["gram_shift"] == fields["gram_shift"]


@pytest.mark.parametrize("value,expected", [
    (None, {}), (0, {}), ([0.0] * 6, {}),
    (-1, {"gram_shift": ALL_M1}), ("mean", {"gram_shift": ALL_MEAN}), ({0: "mean", "relu3_1": -1, 3: "mean"}, {"gram_shift": MIXED}),
])
def test_process_hands_gram_shift_to_the_job(monkeypatch, value, expected):
    """NeuralStyleTransfer.set_gram_shift reaches the device job (a fake in its place), normalised; off passes nothing."""
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []
    # (the real one takes what process passes: every key the table can emit, consumed by job_settings.apply or by _DeviceJob)
    from artstyletransfer_amd import job_settings
    assert "gram_shift" in job_settings.KEYS and set(job_settings.KEYS) <= set(job_settings.APPLY_ORDER) | set(impl._DeviceJob.CONSUMES)
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
    job.set_gram_shift(value)

    async def run():
        async for _ in job.process([np.zeros((256, 384, 3), np.float32)], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    asyncio.run(run())
    assert seen == [expected]


# ---- stripe sharding ----------------------------------------------------------------------------------------------------------
def test_stripe_sharding_refuses_the_setting():
    """PixelOptimizer.shard_stripes on an engine that carries the setting: ValueError before any stripe engine is made."""
    from artstyletransfer_amd import engine, style_modes

    class FakeEngine:
        levels = 1
        layer_weights = style_modes.UNIT_WEIGHTS
        laplacian = None
        gram_shift = ALL_M1
        channels = 3

        def guidance(self, level):
            return 0, (), None

    opt = object.__new__(engine.PixelOptimizer)
    opt.engine = FakeEngine()
    with pytest.raises(ValueError, match="gram_shift cannot be combined with stripe sharding"):
        opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
    src = inspect.getsource(engine.PixelOptimizer.shard_stripes)
    assert src.index("_gram.check_exclusive") < src.index("StyleEngine(weights")


def test_pooled_engine_is_reset():
    """return_engine undoes the job settings through StyleEngine.reset_job_settings, which switches the Gram shift off."""
    from artstyletransfer_amd import engine, neural_nets
    assert "eng.reset_job_settings()" in inspect.getsource(neural_nets.return_engine)
    calls = []
    fake = type("RecordingEngine", (), {"__getattr__": lambda self, method: lambda: calls.append(method)})()
    engine.StyleEngine.reset_job_settings(fake)
    assert "reset_gram_shift" in calls


# ---- the package does not import the oracle -------------------------------------------------------------------------------------
def test_nothing_in_the_package_imports_the_oracle():
    root = os.path.dirname(_lib._HERE)
    pkg = os.path.join(root, "artstyletransfer_amd")
    for name in sorted(os.listdir(pkg)):
        if not name.endswith(".py"):
            continue
        tree = ast.parse(open(os.path.join(pkg, name)).read())
        for node in ast.walk(tree):
            mods = []
            if isinstance(node, ast.Import):
                mods = [a.name for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                mods = [node.module or ""] + [a.name for a in node.names]
            assert not any(m == "oracle" or m.startswith("oracle.") or m == "cpu_ref" for m in mods), (name, mods)


# ---- bindings -------------------------------------------------------------------------------------------------------------------
def test_gram_shift_bindings_match_header_and_library():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert re.search(r"int nst_job_set_gram_shift\(nst_ctx\* ctx, const float shift\[6\], unsigned center_mask\);", hdr)
    assert re.search(r"int nst_job_gram_shift\(const nst_ctx\* ctx, float shift\[6\], unsigned\* center_mask\);", hdr)
    assert re.search(r"int nst_level_gram_offsets\(nst_ctx\* ctx, int level, int slot, float\* out, void\* stream\);", hdr)
    assert re.search(r"int nst_gram_shifted\(nst_ctx\* ctx, const float\* f, int C, int h, int w, int normalize, int center, float shift, "
                     r"float\* gram,\s+float\* offset_out[^;]*void\* stream\);", hdr)
    assert _lib.SYMBOLS["nst_job_set_gram_shift"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_uint])
    assert _lib.SYMBOLS["nst_level_gram_offsets"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p])
    lib = C.CDLL(_lib.LIB_PATH)                      # the built library exports all four
    for name in ("nst_job_set_gram_shift", "nst_job_gram_shift", "nst_level_gram_offsets", "nst_gram_shifted"):
        assert hasattr(lib, name), name
    # without a context: an error code, no crash (bind() refuses a null context)
    lib.nst_job_set_gram_shift.restype = C.c_int
    lib.nst_job_set_gram_shift.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    lib.nst_job_gram_shift.restype = C.c_int
    lib.nst_job_gram_shift.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.nst_job_set_gram_shift(None, None, 0) < 0 and lib.nst_job_gram_shift(None, None, None) < 0
