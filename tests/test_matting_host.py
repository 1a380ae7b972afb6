"""The matting term option on the host: the one normaliser (matting_modes), its refusal before any GPU work in every layer that
takes the option, the Config fields, what Task and NeuralStyleTransfer pass on, the refusal together with stripe sharding, the
bindings against the header and the built library - and the yardstick of tests/test_hip_matting.py: its torch restatement of
the term, held to a dense Levin matrix built entry by entry.  No GPU."""
import asyncio
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from artstyletransfer_amd import _lib
from artstyletransfer_amd import matting_modes as mat


# ---- the normaliser -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight,eps,expected", [
    (None, 1e-7, None),
    (0, 1e-7, None),
    (0.0, 1e-4, None),
    (5, 1e-7, (5.0, 1e-7)),
    (2.5e8, 1e-4, (2.5e8, 1e-4)),
    (np.float32(3.0), np.float64(1e-5), (3.0, 1e-5)),
    (1.0, None, (1.0, 1e-7)),
])
def test_normaliser_accepts(weight, eps, expected):
    assert mat.normalize_matting(weight, eps) == expected


def test_normaliser_defaults():
    assert mat.DEFAULT_EPSILON == 1e-7
    assert mat.normalize_matting() is None
    assert mat.normalize_matting(2.0) == (2.0, 1e-7)


@pytest.mark.parametrize("weight,eps", [
    (-1.0, 1e-7), (float("nan"), 1e-7), (float("inf"), 1e-7), ("1", 1e-7), (True, 1e-7), ((1.0, 2.0), 1e-7), (1e39, 1e-7),
    (1.0, 0.0), (1.0, -1e-7), (1.0, float("nan")), (1.0, float("inf")), (1.0, "tiny"), (1.0, False),
    (None, 0.0), (0.0, -1.0),                      # the epsilon is checked even while the term is off
])
def test_normaliser_refuses(weight, eps):
    with pytest.raises(ValueError):
        mat.normalize_matting(weight, eps)


def test_level_sizes():
    mat.check_levels(1, 3, 3)
    mat.check_levels(2, 64, 96)
    mat.check_levels(5, 50, 76)                    # 50x76 -> 25x38 -> 12x19 -> 6x9 -> 3x4
    with pytest.raises(ValueError, match=r"level 5 is 1x2"):
        mat.check_levels(6, 50, 76)
    with pytest.raises(ValueError, match=r"level 0 is 2x9"):
        mat.check_levels(1, 2, 9)


# ---- before any GPU work ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight,eps", [(-1.0, 1e-7), (float("nan"), 1e-7), (1.0, 0.0), (1.0, float("inf")), ("x", 1e-7)])
def test_matting_is_validated_before_any_gpu_work(weight, eps, monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import config, engine, neural_nets

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the matting setting was validated")

    monkeypatch.setattr(engine.StyleEngine, "__init__", no_engine)
    monkeypatch.setattr(neural_nets, "_weights_cache", [])

    async def run():
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (),
                                                  matting_weight=weight, matting_epsilon=eps):
            pass

    with pytest.raises(ValueError):
        asyncio.run(run())
    with pytest.raises(ValueError):
        config.Config(matting_weight=weight, matting_epsilon=eps)
    with pytest.raises(ValueError):
        nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam").set_matting(weight, eps)
    eng = object.__new__(engine.StyleEngine)       # the engine's own setters validate before they touch the context
    with pytest.raises(ValueError):
        eng.set_matting(weight, eps)
    with pytest.raises(ValueError):
        eng.matting_loss(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), -1.0)


def test_matting_is_keyword_only_in_the_job_driver():
    import neural_style_transfer as nst
    pars = inspect.signature(nst.neural_style_transfer).parameters
    assert pars["matting_weight"].kind is inspect.Parameter.KEYWORD_ONLY and pars["matting_weight"].default is None
    assert pars["matting_epsilon"].kind is inspect.Parameter.KEYWORD_ONLY and pars["matting_epsilon"].default == 1e-7
    assert hasattr(nst.LossBuilder, "set_matting") and hasattr(nst.NeuralStyleTransfer, "set_matting")


# ---- Config / Task ------------------------------------------------------------------------------------------------------------
def test_config_matting_fields():
    from artstyletransfer_amd import config
    before = repr(config.Config())
    c = config.Config(matting_weight=1e4, matting_epsilon=1e-5)
    assert c.matting_weight == 1e4 and c.matting_epsilon == 1e-5
    d = config.Config()
    assert d.matting_weight is None and d.matting_epsilon == 1e-7
    assert repr(c) == before and "matting" not in before
    assert config.Config(*range(13)).matting_weight is None
    with pytest.raises(TypeError):
        config.Config(*range(14))
    import config as dropin                       # the drop-in module name re-exports the same class
    assert dropin.Config(matting_weight=3.0).matting_weight == 3.0


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"matting_epsilon": 1e-4}, {"device"}),                              # no weight: the term is off, nothing is passed
    ({"matting_weight": 5.0}, {"device", "matting_weight", "matting_epsilon"}),
    ({"matting_weight": 5.0, "matting_epsilon": 1e-4, "pooling": "avg"}, {"device", "matting_weight", "matting_epsilon", "pooling"}),
])
def test_task_passes_matting_through(monkeypatch, fields, expected):
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
        assert seen[0][k] == fields.get(k, 1e-7)


@pytest.mark.parametrize("args,expected", [
    ((None, 1e-7), {}),
    ((0.0, 1e-4), {}),
    ((5.0, 1e-7), {"matting": (5.0, 1e-7)}),
    ((2e8, 1e-4), {"matting": (2e8, 1e-4)}),
])
def test_process_hands_matting_to_the_job(monkeypatch, args, expected):
    """NeuralStyleTransfer.set_matting reaches the device job (a fake in its place), normalised; off passes nothing."""
    import neural_style_transfer as nst
    from artstyletransfer_amd import math_utils
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []
    # (the real one takes what process passes: every key the table can emit, consumed by job_settings.apply or by _DeviceJob)
    from artstyletransfer_amd import job_settings
    assert "matting" in job_settings.KEYS and set(job_settings.KEYS) <= set(job_settings.APPLY_ORDER) | set(impl._DeviceJob.CONSUMES)
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
    job.set_matting(*args)

    async def run():
        async for _ in job.process([np.zeros((256, 384, 3), np.float32)], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    asyncio.run(run())
    assert seen == [expected]


# ---- stripe sharding ----------------------------------------------------------------------------------------------------------
def test_stripe_sharding_refuses_the_matting_term():
    """PixelOptimizer.shard_stripes on an engine that carries the setting: ValueError before any stripe engine is made."""
    from artstyletransfer_amd import engine, style_modes

    class FakeEngine:
        levels = 1
        layer_weights = style_modes.UNIT_WEIGHTS
        laplacian = None
        gram_shift = None
        matting = (1.0, 1e-7)
        channels = 3

        def guidance(self, level):
            return 0, (), None

    opt = object.__new__(engine.PixelOptimizer)
    opt.engine = FakeEngine()
    with pytest.raises(ValueError, match="matting_weight cannot be combined with stripe sharding"):
        opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
    src = inspect.getsource(engine.PixelOptimizer.shard_stripes)
    assert src.index('"matting", None) is not None') < src.index("StyleEngine(weights")


# ---- bindings -------------------------------------------------------------------------------------------------------------------
def test_matting_bindings_match_header_and_library():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert "#define NST_LOSS_ROW 4 " in hdr                           # the loss row keeps its layout
    assert re.search(r"int nst_job_set_matting\(nst_ctx\* ctx, float gamma, double epsilon\);", hdr)
    assert re.search(r"int nst_job_matting\(const nst_ctx\* ctx, float\* gamma, double\* epsilon\);", hdr)
    assert re.search(r"int nst_job_matting_losses\(nst_ctx\* ctx, float\* out[^;]*void\* stream\);", hdr)
    assert re.search(r"int nst_matting_loss\(nst_ctx\* ctx, const float\* y, const float\* guide, int C, int h, int w, double epsilon, float\* value,", hdr)
    assert re.search(r"nst_job_set_laplacian, nst_job_set_matting, nst_job_set_gram_shift", hdr)      # the closure-reuse list
    assert _lib.SYMBOLS["nst_job_set_matting"] == (C.c_int, [C.c_void_p, C.c_float, C.c_double])
    assert _lib.SYMBOLS["nst_job_matting_losses"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    lib = C.CDLL(_lib.LIB_PATH)                      # the built library exports all four
    for name in ("nst_job_set_matting", "nst_job_matting", "nst_job_matting_losses", "nst_matting_loss"):
        assert hasattr(lib, name), name
    # without a context: an error code, no crash (bind() refuses a null context)
    lib.nst_job_set_matting.restype = C.c_int
    lib.nst_job_set_matting.argtypes = [C.c_void_p, C.c_float, C.c_double]
    lib.nst_job_matting.restype = C.c_int
    lib.nst_job_matting.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.nst_job_set_matting(None, 1.0, 1e-7) < 0 and lib.nst_job_matting(None, None, None) < 0


# ---- the yardstick --------------------------------------------------------------------------------------------------------------
def dense_levin(guide, eps):
    """Levin's matting Laplacian of an (h,w,3) float64 guide with 3x3 windows, entry by entry: (h w, h w)."""
    h, w, _ = guide.shape
    L = np.zeros((h * w, h * w))
    for i in range(h - 2):
        for j in range(w - 2):
            idx = [(i + a) * w + (j + b) for a in range(3) for b in range(3)]
            win = np.array([guide[i + a, j + b] for a in range(3) for b in range(3)])
            mu = win.mean(axis=0)
            cov = (win - mu).T @ (win - mu) / 9.0
            inv = np.linalg.inv(cov + eps / 9.0 * np.eye(3))
            for p in range(9):
                for q in range(9):
                    L[idx[p], idx[q]] += (1.0 if p == q else 0.0) - (1.0 + (win[p] - mu) @ inv @ (win[q] - mu)) / 9.0
    return L


@pytest.mark.parametrize("kind", ["noise", "ramp", "constant", "quantised"])
@pytest.mark.parametrize("eps", [1e-7, 1e-4])
def test_restatement_equals_the_dense_levin_form(kind, eps):
    """tests/test_hip_matting.py's mat_term on an 8x9 image in fp64: value = (1/n) sum_c V_c^T L V_c and gradient =
    (2 / (255 n)) L V_c with the dense L, for each of the GPU test's guides."""
    import test_hip_matting as gpu
    h, w = 8, 9
    guide = gpu._guide(kind, h, w, 5)
    y = gpu._image("noise", guide, 6)
    v, g = gpu.mat_piece(y, gpu._chw(guide), eps, torch.float64)
    L = dense_levin(guide.astype(np.float64), eps)
    n = 3.0 * (h - 2) * (w - 2)
    V = y[0].double().numpy().reshape(3, -1) / 255.0
    want_v = sum(V[c] @ L @ V[c] for c in range(3)) / n
    want_g = np.stack([2.0 * (L @ V[c]) / (255.0 * n) for c in range(3)]).reshape(1, 3, h, w)
    # both sides are fp64; what separates them is the inverse of M_k, whose condition number reaches (guide variance) /
    # (eps / 9) = 1e7 on the near-rank-1 guides: 1e7 x 2.2e-16 = 2e-9 per entry, an order of magnitude of slack for the sums
    assert np.allclose(L, L.T, rtol=0, atol=2e-8 * np.abs(L).max())
    assert abs(v - want_v) <= 2e-8 * abs(want_v)
    assert np.linalg.norm(g.numpy() - want_g) <= 2e-8 * np.linalg.norm(want_g)
    # the luminance rule: three equal guide channels reduce to the scalar form with epsilon / 3
    gu = torch.from_numpy(guide[:, :, :1].astype(np.float64)).permute(2, 0, 1).unsqueeze(0)
    u = y[:, :1].double()
    three = float(gpu.mat_term(u.expand(-1, 3, -1, -1), gu.expand(-1, 3, -1, -1), eps))
    uw, gw = gpu.windows(u / 255.0)[:, :, 0], gpu.windows(gu)[:, :, 0]
    uc, gc = uw - uw.mean(dim=1, keepdim=True), gw - gw.mean(dim=1, keepdim=True)
    t = (uc * gc).sum(dim=1)
    scalar = float(((uc * uc).sum(dim=1) - t * t / ((gc * gc).sum(dim=1) + eps / 3.0)).sum() / ((h - 2) * (w - 2)))
    assert abs(three - scalar) <= 1e-9 * abs(scalar)
