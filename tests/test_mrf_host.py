"""CPU: the MRF style term on the host layers - the one normaliser (artstyletransfer_amd/mrf_modes.py) with every accepted
form and every refusal, validation before any GPU work, the signature of neural_style_transfer_mrf(), its delegation to
neural_style_transfer() when the term is off and its way down to the device job (fakes in their places), and the bindings
against the header.  No GPU."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest

from artstyletransfer_amd import _lib
from artstyletransfer_amd import mrf_modes as mrf

Z = 0.0
ZEROS = (Z,) * 6
EPS = mrf.DEFAULT_EPSILON
LW = (Z, Z, 5.0, 5.0, Z, Z)                    # a number: that weight on relu3_1 and relu4_1


# ---- the normaliser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [None, 0, 0.0, [0] * 6, (0.0,) * 6, {}, {2: 0}, np.zeros(6), np.float32(0)])
def test_normaliser_off(value):
    assert mrf.normalize_mrf(value) is None
    assert mrf.normalize_weights(value) == ZEROS


@pytest.mark.parametrize("value,expected", [
    (5.0, LW), (5, LW), (np.float64(5), LW), ([0, 0, 5, 5, 0, 0], LW), (np.array(LW), LW), ({2: 5, 3: 5.0}, LW),
    ({"relu3_1": 5, "relu4_1": 5}, LW), ({"conv3_1": 5, 3: 5}, LW), ({np.int64(5): 0.25}, (Z, Z, Z, Z, Z, 0.25)),
    ([1, 2, 3, 4, 0, 6], (1.0, 2.0, 3.0, 4.0, Z, 6.0)),
])
def test_normaliser_accepts(value, expected):
    assert mrf.normalize_weights(value) == expected
    assert mrf.normalize_mrf(value) == (expected, 1, EPS, None)
    assert mrf.normalize_mrf(value, 2, 1e-3, [1, 0, 1]) == (expected, 2, 1e-3, (0, 1))
    assert mrf.normalize_mrf(value, np.int64(8), mrf_levels=(2,), levels_num=3) == (expected, 8, EPS, (2,))


def test_a_number_goes_on_the_li_wand_maps_that_are_style_maps():
    assert mrf.normalize_weights(2.0, style_indices=(0, 1, 2)) == (Z, Z, 2.0, Z, Z, Z)
    assert mrf.normalize_weights(2.0, style_indices=range(6)) == (Z, Z, 2.0, 2.0, Z, Z)
    with pytest.raises(ValueError, match="neither relu3_1 nor relu4_1"):
        mrf.normalize_weights(2.0, style_indices=(0, 1, 5))
    assert mrf.normalize_weights(0.0, style_indices=(0, 1, 5)) == ZEROS           # off names no map
    # six numbers and a dict are by map index: a positive weight outside the style set is refused where the set is known
    for bad in ([0, 0, 1, 0, 0, 0], {4: 1.0}, {"conv4_2": 1.0}):
        with pytest.raises(ValueError, match="not a style map"):
            mrf.normalize_weights(bad, style_indices=(0, 1))
        assert mrf.normalize_weights(bad) is not None                             # (not checked while the set is not known)
    assert mrf.normalize_weights({4: 0.0}, style_indices=(0, 1)) == ZEROS
    with pytest.raises(ValueError, match="not one of the feature maps"):
        mrf.normalize_weights({"relu3_1": 1.0}, style_indices=(2,), use_relu=False)


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), "5", True, [1, 2, 3], [0] * 7, [0, 0, -1, 0, 0, 0], {6: 1.0},
                                 {"relu9_9": 1.0}, {2: "x"}, {2.5: 1.0}, {1, 2}, object()])
def test_normaliser_refuses_weights(bad):
    with pytest.raises(ValueError, match="mrf_weight"):
        mrf.normalize_mrf(bad)


@pytest.mark.parametrize("stride", [0, 9, -1, 1.0, 2.5, "2", None, True])
def test_normaliser_refuses_strides(stride):
    with pytest.raises(ValueError, match="mrf_stride"):
        mrf.normalize_mrf(1.0, stride)
    with pytest.raises(ValueError, match="mrf_stride"):
        mrf.normalize_mrf(None, stride)                    # the off setting is validated too


@pytest.mark.parametrize("eps", [0, 0.0, -1e-5, float("nan"), float("inf"), "1e-5", None, True])
def test_normaliser_refuses_epsilons(eps):
    with pytest.raises(ValueError, match="mrf_epsilon"):
        mrf.normalize_mrf(1.0, 1, eps)


@pytest.mark.parametrize("levels", [[], 1, "01", [0.5], [-1], [8], [True], {0: 1}, [0, "1"]])
def test_normaliser_refuses_levels(levels):
    with pytest.raises(ValueError, match="mrf_levels"):
        mrf.normalize_mrf(1.0, mrf_levels=levels)


def test_levels_against_the_job():
    assert mrf.normalize_levels([2, 0], levels_num=3) == (0, 2)
    with pytest.raises(ValueError, match="mrf_levels"):
        mrf.normalize_levels([3], levels_num=3)
    assert mrf.normalize_levels({1}) == (1,) and mrf.normalize_levels(range(2)) == (0, 1) and mrf.normalize_levels(None) is None


def test_exclusive_and_sizes():
    on = mrf.normalize_mrf(1.0)
    mrf.check_exclusive(None, regions=object(), stripes=True, extra_styles=[1])
    mrf.check_exclusive(on)
    mrf.check_exclusive(on, extra_styles=[])
    with pytest.raises(ValueError, match="extra_styles"):
        mrf.check_exclusive(on, extra_styles=[object()])
    with pytest.raises(ValueError, match="content_regions"):
        mrf.check_exclusive(on, regions=object())
    with pytest.raises(ValueError, match="stripe sharding"):
        mrf.check_exclusive(on, stripes=True)
    # relu4_1 of a 16x24 level is 2x3: no patch - on the image or on the style image, on a chosen level only
    shapes, small = [(64, 96), (32, 48)], [(64, 96), (16, 24)]
    mrf.check_sizes(on, shapes, shapes)
    mrf.check_sizes(None, small, small)
    for c, s, what in ((small, shapes, "of the image"), (shapes, small, "of the style image")):
        with pytest.raises(ValueError, match=f"map 3 {what} of level 1"):
            mrf.check_sizes(on, c, s)
        mrf.check_sizes(mrf.normalize_mrf(1.0, mrf_levels=[0]), c, s)
    mrf.check_sizes(mrf.normalize_mrf({2: 1.0}), small, small)              # relu3_1 of 16x24 is 4x6
    with pytest.raises(ValueError, match="outside the job"):
        mrf.check_sizes(mrf.normalize_mrf(1.0, mrf_levels=[2]), shapes, shapes)


def test_module_is_free_of_torch():
    src = open(mrf.__file__).read()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)


# ---- the job function -------------------------------------------------------------------------------------------------------
def test_signature_is_neural_style_transfers_plus_four_keywords():
    from artstyletransfer_amd.neural_style_transfer import neural_style_transfer
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf
    base = list(inspect.signature(neural_style_transfer).parameters.values())
    ours = list(inspect.signature(neural_style_transfer_mrf).parameters.values())
    assert [(p.name, p.kind, p.default) for p in ours[:len(base)]] == [(p.name, p.kind, p.default) for p in base]
    extra = ours[len(base):]
    assert [(p.name, p.default) for p in extra] == [("mrf_weight", None), ("mrf_stride", 1), ("mrf_epsilon", 1e-5), ("mrf_levels", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in extra)
    assert inspect.isasyncgenfunction(neural_style_transfer_mrf)


ARGS = (None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 2, 0.0, (), (), (), ())


def _collect(gen):
    async def run():
        return [item async for item in gen]
    return asyncio.run(run())


def test_off_delegates_and_on_goes_through_transfer_from(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf
    calls = []

    async def fake_plain(*a, **kw):
        calls.append(("plain", a, kw))
        yield 100, "plain image"

    def fake_from(*a, device=None, start=None, patches=None, **kw):
        calls.append(("from", a, dict(kw, device=device, start=start, patches=patches)))

        async def gen():
            yield 100, "mrf image"
        return gen()

    monkeypatch.setattr(impl, "neural_style_transfer", fake_plain)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    for off in (None, 0, 0.0, [0] * 6, {}):
        calls.clear()
        assert _collect(neural_style_transfer_mrf(*ARGS, "dev", pooling="avg", mrf_weight=off, mrf_stride=2)) == [(100, "plain image")]
        (kind, a, kw), = calls
        assert kind == "plain" and a == ARGS + ("dev",) and kw["pooling"] == "avg" and not any(k.startswith("mrf_") for k in kw)
    calls.clear()
    out = _collect(neural_style_transfer_mrf(*ARGS, "dev", moment_weight=3.0, mrf_weight={3: 2.0}, mrf_stride=2, mrf_levels=[1]))
    assert out == [(100, "mrf image")]
    (kind, a, kw), = calls
    assert kind == "from" and a == ARGS and kw["device"] == "dev" and kw["start"] is None and kw["moment_weight"] == 3.0
    assert kw["patches"] == ({3: 2.0}, 2, 1e-5, [1])
    # a malformed setting never reaches either
    calls.clear()
    for bad in (dict(mrf_weight=-1.0), dict(mrf_weight=1.0, mrf_stride=9), dict(mrf_weight=None, mrf_epsilon=0.0),
                dict(mrf_weight=1.0, mrf_levels=[])):
        with pytest.raises(ValueError, match="mrf_"):
            _collect(neural_style_transfer_mrf(*ARGS, **bad))
    assert calls == []


def _pair(h=64, w=96, hs=70, ws=110):
    from artstyletransfer_amd import neural_style_transfer as impl
    return impl.ContentStylePair(("c", np.zeros((h, w, 3), np.float32)), ("s", np.zeros((hs, ws, 3), np.float32)))


def test_refusals_before_any_gpu_work(monkeypatch):
    """With the job's style set and level sizes: everything is refused in _transfer_from, before _transfer is even created."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf

    def reached(*a, **kw):
        raise AssertionError("the job was started")

    monkeypatch.setattr(impl, "_transfer", reached)
    monkeypatch.setattr(impl, "shared_engine", reached)
    args = (_pair(),) + ARGS[1:]
    cases = [
        (dict(mrf_weight=1.0, extra_styles=[np.zeros((32, 32, 3), np.float32)]), "extra_styles"),
        (dict(mrf_weight=1.0, content_regions=np.zeros((64, 96), np.int64), style_regions=np.zeros((70, 110), np.int64)), "content_regions"),
        (dict(mrf_weight={4: 1.0}), "not a style map"),
        (dict(mrf_weight=1.0, style_layers=[0, 1, 5]), "neither relu3_1 nor relu4_1"),
        (dict(mrf_weight=1.0, mrf_levels=[2]), "mrf_levels"),
    ]
    # (a level of this driver has a short edge of 256 or more, so no map of it pools below 3x3: mrf_modes.check_sizes is
    # held above and through NeuralStyleTransfer.process below)
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            _collect(neural_style_transfer_mrf(*args, **kw))


def test_set_patch_match_reaches_the_device_job(monkeypatch):
    """NeuralStyleTransfer.set_patch_match is data of the next process: handed to the device job once it exists, after the
    settings, with the checked weights; a job without it never calls the hook."""
    import torch
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def __init__(self, *a, **kw):
            seen.append(("made", sorted(kw)))

        def set_patch_match(self, *a):
            seen.append(("patches", a))

        def close(self):
            seen.append(("closed",))

    monkeypatch.setattr(impl, "_make_job", lambda *a, **kw: FakeJob(*a, **kw))
    monkeypatch.setattr(impl.math_utils, "prepare_model", lambda *a: None)
    content = [np.zeros((64, 96, 3), np.float32), np.zeros((32, 48, 3), np.float32)]
    style = [np.zeros((70, 110, 3), np.float32), np.zeros((35, 55, 3), np.float32)]

    def run(nst):
        async def go():
            return [x async for x in nst.process(content, content[0], 10.0, 0, 1e3, 4e5, 1e2, "c")]
        return asyncio.run(go())

    nst = impl.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", style, "adam")
    nst.set_patch_match(2.0, stride=2, levels=[1])
    assert run(nst) == []
    assert seen == [("made", []), ("patches", ((Z, Z, 2.0, 2.0, Z, Z), 2, 1e-5, (1,))), ("closed",)]
    seen.clear()
    nst.set_patch_match(None)
    assert run(nst) == [] and seen == [("made", []), ("closed",)]
    # refusals of process(), where the style set and the level sizes are known: before the job exists
    seen.clear()
    nst.set_patch_match({5: 1.0})                                  # relu5_1 of the 32x48 level is 2x3
    with pytest.raises(ValueError, match="pools below 3x3"):
        run(nst)
    nst.set_patch_match(1.0)
    nst.set_feature_maps(4, [0, 1, 5])
    with pytest.raises(ValueError, match="neither relu3_1 nor relu4_1"):
        run(nst)
    assert seen == []
    with pytest.raises(ValueError, match="mrf_stride"):
        nst.set_patch_match(1.0, stride=0)


# ---- the bindings -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nst_hip.h")).read()
    for name, nargs in (("nst_level_set_patches", 9), ("nst_level_patches", 5), ("nst_job_patch_losses", 3),
                        ("nst_level_patch_matches", 5), ("nst_patch_match", 13), ("nst_patch_term", 14)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name


def test_job_settings_tables_are_untouched():
    """The term is data of a job: no SETTINGS row, no _JOB_SETTINGS row, no keyword of neural_style_transfer()."""
    from artstyletransfer_amd import job_settings
    from artstyletransfer_amd.neural_style_transfer import neural_style_transfer
    assert not any("mrf" in str(row).lower() or "patch" in str(row).lower() for row in job_settings.SETTINGS)
    assert not any(p.startswith("mrf") for p in inspect.signature(neural_style_transfer).parameters)
