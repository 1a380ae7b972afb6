"""CPU: the pooling option of the feature network (pooling="max" | "avg") on the host layers - validation before any GPU work,
the Config field and its way through Task, the binding of nst_job_set_pooling / nst_job_pooling, Vgg19(pooling=...) - and
the committed pool_avg_* fixtures (what the reference's LossBuilder computed on its network with every MaxPool2d replaced by
AvgPool2d(2, 2): tests/golden/make_fixtures_pool.py) against the CPU oracle with a test-local average-pool network, to the
bounds tests/test_oracle_vs_golden.py holds the oracle to: the fixtures are what the definition in include/nst_hip.h says.
No GPU."""
import asyncio
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from artstyletransfer_amd import _lib
from oracle import cpu_ref

BAD = ["mean", "AVG", "", None, 1, True, ("avg",), "average"]
TERMS = {"c": (1e3, 0.0, 0.0), "s": (0.0, 4e5, 0.0), "tv": (0.0, 0.0, 1e2)}


def avg_vgg19_features(x, weights, decisions=None, record=None, *, use_relu=True):
    """cpu_ref.vgg19_features with F.avg_pool2d(2, 2) for the four pools (ReLU masks from `decisions.relu` when given; the
    average has no decisions of its own).  use_relu=False: map 5 is conv5_1 before its ReLU, as the reference's
    Vgg19(use_relu=False) leaves it."""
    outs = []
    last = len(cpu_ref.VGG19_CONVS) - 1
    for li, ((name, _, _), (w, b)) in enumerate(zip(cpu_ref.VGG19_CONVS, weights)):
        pre = F.conv2d(x, w, b, stride=1, padding=1)
        if record is not None:
            record.append(pre.detach())
        x = F.relu(pre) if decisions is None else pre * decisions.relu[li].to(pre.dtype)
        if name in cpu_ref.TAPS:
            outs.append(pre if (li == last and not use_relu) else x)
        if name in cpu_ref.POOL_AFTER:
            x = F.avg_pool2d(x, kernel_size=2, stride=2)
    return outs


@pytest.mark.parametrize("bad", BAD)
def test_pooling_is_validated_before_any_gpu_work(bad, monkeypatch):
    import neural_style_transfer as nst
    from artstyletransfer_amd import config, engine, neural_nets

    def no_engine(*a, **k):
        raise AssertionError("an engine was created before the pooling value was validated")

    monkeypatch.setattr(engine.StyleEngine, "__init__", no_engine)
    monkeypatch.setattr(neural_nets, "_weights_cache", [])

    async def run():
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (),
                                                  pooling=bad):
            pass

    with pytest.raises(ValueError):
        asyncio.run(run())
    with pytest.raises(ValueError):
        config.Config(pooling=bad)
    with pytest.raises(ValueError):
        nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam").set_pooling(bad)
    with pytest.raises(ValueError):
        neural_nets.Vgg19(pooling=bad)

    class Net:
        use_relu = True
        pooling = bad

    with pytest.raises(ValueError):
        nst.LossBuilder(4, [0], None, None, Net(), 1e3, 4e5, 1e2)
    # the engine's own setter validates before it touches the context
    eng = object.__new__(engine.StyleEngine)
    with pytest.raises(ValueError):
        eng.set_pooling(bad)


def test_pooling_is_keyword_only_in_the_job_driver():
    import inspect
    import neural_style_transfer as nst
    from artstyletransfer_amd import neural_nets
    par = inspect.signature(nst.neural_style_transfer).parameters["pooling"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == "max"
    # the network mirror takes it at the class call (Vgg19.__init__ keeps the reference's parameter list)
    par = inspect.signature(type(neural_nets.Vgg19).__call__).parameters["pooling"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default == "max"
    assert list(inspect.signature(neural_nets.Vgg19.__init__).parameters)[1:] == ["requires_grad", "show_progress", "use_relu"]


def test_vgg19_pooling_attribute(monkeypatch):
    from artstyletransfer_amd import neural_nets
    monkeypatch.setattr(neural_nets, "_weights_cache", [])
    assert neural_nets.Vgg19(pooling="avg").pooling == "avg"
    assert neural_nets.Vgg19().pooling == "max"
    net = neural_nets.Vgg19(use_relu=False, pooling="avg")
    assert net.pooling == "avg" and net.use_relu is False and net.layer_names[5] == "conv5_1"


def test_config_pooling_field():
    from artstyletransfer_amd import config
    before = repr(config.Config())
    c = config.Config(pooling="avg")
    assert c.pooling == "avg" and config.Config().pooling == "max"
    assert repr(c) == before and "pooling" not in before
    assert config.Config(*range(13)).pooling == "max"
    with pytest.raises(TypeError):
        config.Config(*range(14))


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"pooling": "max"}, {"device"}),
    ({"pooling": "avg"}, {"device", "pooling"}),
    ({"pooling": "avg", "preserve_color": "luminance", "content_layer": 2}, {"device", "pooling", "preserve_color", "content_layer"}),
])
def test_task_passes_pooling_through(monkeypatch, fields, expected):
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
        assert seen[0][k] == fields[k]


@pytest.mark.parametrize("mode,expected", [("max", {}), ("avg", {"pooling": "avg"})])
def test_process_hands_pooling_to_the_job(monkeypatch, mode, expected):
    """NeuralStyleTransfer.set_pooling reaches the device job (a fake in its place); "max" passes nothing: the default job."""
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
    job = nst.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", [], "adam")
    job.set_pooling(mode)

    async def run():
        async for _ in job.process([], None, 10.0, 0, 1e3, 4e5, 1e2, "x"):
            pass

    asyncio.run(run())
    assert seen == [expected]


def test_pooling_bindings_match_header_and_library():
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert "#define NST_POOL_MAX 0" in hdr and "#define NST_POOL_AVG 1" in hdr
    assert (_lib.NST_POOL_MAX, _lib.NST_POOL_AVG) == (0, 1)
    assert re.search(r"int nst_job_set_pooling\(nst_ctx\* ctx, int mode\);", hdr)
    assert re.search(r"int nst_job_pooling\(const nst_ctx\* ctx\);", hdr)
    assert _lib.SYMBOLS["nst_job_set_pooling"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.SYMBOLS["nst_job_pooling"] == (C.c_int, [C.c_void_p])
    lib = C.CDLL(_lib.LIB_PATH)                      # the built library exports both
    for name in ("nst_job_set_pooling", "nst_job_pooling"):
        assert hasattr(lib, name), name
    # without a context: an error code, no crash (bind() refuses a null context)
    lib.nst_job_set_pooling.restype = C.c_int
    lib.nst_job_set_pooling.argtypes = [C.c_void_p, C.c_int]
    lib.nst_job_pooling.restype = C.c_int
    lib.nst_job_pooling.argtypes = [C.c_void_p]
    assert lib.nst_job_set_pooling(None, 1) < 0 and lib.nst_job_pooling(None) == -1


# ---- the fixtures are what the header's definition says ---------------------------------------------------------------
CLOSURE_FIXTURES = ("pool_avg_64x96_L1", "pool_avg_shallow_64x96_L1", "pool_avg_prerelu_64x96_L1", "pool_avg_50x76_L0")


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", CLOSURE_FIXTURES)
def test_fixture_is_the_oracle_on_the_average_pool_network(golden, vgg_weights, monkeypatch, name):
    """Losses and the gradients of the sum and of every term alone to 1e-6 (tests/test_oracle_vs_golden.py's bounds for the
    max-pool fixtures), the oracle's network being the test-local average-pool one."""
    fx = golden(name)
    use_relu = bool(fx["use_relu"])
    monkeypatch.setattr(cpu_ref, "vgg19_features",
                        lambda x, w, decisions=None, record=None: avg_vgg19_features(x, w, decisions, record, use_relu=use_relu))
    monkeypatch.setattr(cpu_ref, "CONTENT_INDEX", int(fx["content_index"]))
    monkeypatch.setattr(cpu_ref, "STYLE_INDICES", tuple(int(i) for i in fx["style_indices"]))
    nlev = int(fx["levels"])
    tg = [cpu_ref.LevelTargets(cpu_ref.prepare_img(fx[f"content{i}"]), cpu_ref.prepare_img(fx[f"style{i}"]), vgg_weights)
          for i in range(nlev)]
    x = cpu_ref.prepare_img(fx["x_img"])
    total, grad, rows = cpu_ref.closure_eval(x, tg, vgg_weights, 1e3, 4e5, 1e2)
    print(f"{name}: total rel {abs(float(total) - float(fx['total'])) / float(fx['total']):.2e}, grad rel-L2 {_rel_l2(grad.numpy(), fx['grad']):.2e}")
    assert float(total) == pytest.approx(float(fx["total"]), rel=1e-6)
    np.testing.assert_allclose(np.array(rows), fx["rows"], rtol=1e-6)
    assert _rel_l2(grad.numpy(), fx["grad"]) < 1e-6
    for tag, wts in TERMS.items():
        t, g, _ = cpu_ref.closure_eval(x, tg, vgg_weights, *wts)
        print(f"{name} [{tag}]: total rel {abs(float(t) - float(fx[f'total_{tag}'])) / max(float(fx[f'total_{tag}']), 1e-30):.2e}, "
              f"grad rel-L2 {_rel_l2(g.numpy(), fx[f'grad_{tag}']):.2e}")
        assert float(t) == pytest.approx(float(fx[f"total_{tag}"]), rel=1e-6)
        assert _rel_l2(g.numpy(), fx[f"grad_{tag}"]) < 1e-6, tag


def test_vgg_fixture_is_the_average_pool_network(golden, vgg_weights):
    fx = golden("pool_avg_vgg_48x80")
    with torch.no_grad():
        outs = avg_vgg19_features(cpu_ref.prepare_img(fx["img"]), vgg_weights)
    for i, o in enumerate(outs):
        assert list(o.shape) == list(fx[f"out{i}.shape"])
        flat = o.reshape(-1)
        np.testing.assert_allclose(flat[torch.from_numpy(fx[f"out{i}.idx"])].numpy(), fx[f"out{i}.val"], rtol=1e-6, atol=1e-6)
        assert float(flat.double().sum()) == pytest.approx(float(fx[f"out{i}.sum"]), rel=1e-6)
    assert _rel_l2(outs[5].numpy(), fx["out5_full"]) < 1e-6 and _rel_l2(outs[4].numpy(), fx["out4_full"]) < 1e-6


def test_average_is_not_maximum(golden, vgg_weights):
    """The avg fixture's losses differ from the max fixture's on the same inputs (closure_64x96_L1)."""
    a, m = golden("pool_avg_64x96_L1"), golden("closure_64x96_L1")
    assert np.array_equal(a["x_img"], m["x_img"]) and np.array_equal(a["content0"], m["content0"])
    assert abs(float(a["total"]) - float(m["total"])) > 1e-2 * abs(float(m["total"]))
