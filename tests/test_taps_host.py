"""CPU: the feature-map options (taps) of the host layers - validation, Vgg19(use_relu=False) attributes, the Config
fields, their way through Task, and the binding of nst_job_set_taps.  No GPU."""
import asyncio
import ctypes as C
import re

import pytest

from artstyletransfer_amd import _lib
from artstyletransfer_amd.taps import normalize_taps, style_mask


def test_normalize_taps_accepts_indices_and_names():
    assert normalize_taps() == (4, (0, 1, 2, 3, 5))
    assert normalize_taps(2, [3, 2, 2]) == (2, (2, 3))                 # order and repeats do not matter
    assert normalize_taps("relu2_1", ["relu1_1", 1]) == (1, (0, 1))
    assert normalize_taps("conv4_2", "conv5_1", use_relu=False) == (4, (5,))
    assert normalize_taps(0, 3) == (0, (3,))                            # a single style index, as build_style takes it
    assert style_mask((0, 1, 2, 3, 5)) == 0x2F


@pytest.mark.parametrize("content,style,use_relu", [
    (4, [], True),                       # empty set: the reference divides by zero
    (4, [0, 6], True),                   # out of range: the reference silently drops it
    (-1, [0], True),
    ([4], [0], True),                    # content as a list
    (4.0, [0], True),
    (True, [0], True),
    ("conv1_1", [0], True),              # a name of the other flavour
    (4, ["relu1_1"], False),
    (4, [0], 1),                         # use_relu must be a bool
])
def test_normalize_taps_rejects(content, style, use_relu):
    with pytest.raises(ValueError):
        normalize_taps(content, style, use_relu)


def test_vgg19_prerelu_attributes(monkeypatch):
    from artstyletransfer_amd import neural_nets
    monkeypatch.setattr(neural_nets, "_weights_cache", [])
    net = neural_nets.Vgg19(use_relu=False)
    assert net.layer_names == ["conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv4_2", "conv5_1"]
    assert net.offset == 0 and net.use_relu is False
    assert net.content_feature_maps_index == 4 and net.style_feature_maps_indices == [0, 1, 2, 3, 5]
    d = neural_nets.Vgg19()
    assert d.layer_names[5] == "relu5_1" and d.offset == 1 and d.use_relu is True


def test_loss_builder_validates_before_any_gpu_work():
    import neural_style_transfer as nst

    class Net:
        use_relu = True

    with pytest.raises(ValueError):
        nst.LossBuilder(4, [], None, None, Net(), 1e3, 4e5, 1e2)
    with pytest.raises(ValueError):
        nst.LossBuilder([4], [0], None, None, Net(), 1e3, 4e5, 1e2)


def test_set_feature_maps_validates():
    import neural_style_transfer as nst
    job = nst.NeuralStyleTransfer("cpu", "vgg19", [], "adam")
    job.set_feature_maps("relu3_1", [2, 3])
    with pytest.raises(ValueError):
        job.set_feature_maps(4, [7])


def test_job_driver_validates_taps_first():
    import neural_style_transfer as nst

    async def run():
        async for _ in nst.neural_style_transfer(None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 1, 0.0, (), (), (), (),
                                                  style_layers=[]):
            pass

    with pytest.raises(ValueError):
        asyncio.run(run())


def test_config_keyword_only_fields():
    from artstyletransfer_amd import config
    c = config.Config()
    assert (c.content_layer, c.style_layers, c.use_relu) == (None, None, True)
    c = config.Config(content_layer=2, style_layers=[2, 3], use_relu=False)
    assert (c.content_layer, c.style_layers, c.use_relu) == (2, [2, 3], False)
    assert "content_layer" not in repr(c)
    with pytest.raises(TypeError):
        config.Config(*range(14))
    assert config.Config(*range(13)).noise_levels_dispersion == 12


@pytest.mark.parametrize("fields,expected", [
    ({}, {"device"}),
    ({"content_layer": "relu2_1", "style_layers": [0, 1], "use_relu": False},
     {"device", "content_layer", "style_layers", "use_relu"}),
])
def test_task_passes_taps_through(monkeypatch, fields, expected):
    from artstyletransfer_amd import config, task_executor as te
    seen = []

    async def fake_nst(pair, *args, **kw):
        seen.append(kw)
        yield 100.0, __import__("numpy").zeros((2, 2, 3), "float32")

    monkeypatch.setattr(te, "neural_style_transfer", fake_nst)

    async def main():
        ex = te.Executor(config.Config(iters_num=1, **fields), gpu_slots=te.GpuSlots(per_gpu=1, n_gpus=1))
        await ex.add_task("t", None)
        await ex.wait_all()

    asyncio.run(main())
    assert len(seen) == 1 and set(seen[0]) == expected
    for k, v in fields.items():
        assert seen[0][k] == v


def test_set_taps_binding_matches_header():
    import os
    res, args = _lib.SYMBOLS["nst_job_set_taps"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_uint, C.c_int]
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "nst_hip.h")).read()
    assert re.search(r"int nst_job_set_taps\(nst_ctx\* ctx, int content_index, unsigned style_mask, int use_relu\);", hdr)
