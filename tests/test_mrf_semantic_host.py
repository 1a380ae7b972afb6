"""CPU: the semantic maps of the MRF term (neural-doodle) on the host layers - the normaliser (mrf_modes.normalize_semantic)
with every accepted form and every refusal, the signature of neural_style_transfer_mrf_semantic(), its delegation to
neural_style_transfer_mrf() when no map is given, validation before any GPU work, the way down to
_DeviceJob.set_patch_semantics (fakes in their places), and the bindings against the header.  No GPU."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest

from artstyletransfer_amd import _lib
from artstyletransfer_amd import mrf_modes as mrf
from artstyletransfer_amd import regions as rg

LABELS = (np.arange(96)[None, :] * 2 // 96).repeat(64, 0)                 # (64,96), two vertical bands
STYLE_LABELS = (np.arange(110)[None, :] * 2 // 110).repeat(70, 0)


# ---- the normaliser -------------------------------------------------------------------------------------------------------
def test_normaliser_off():
    assert mrf.normalize_semantic() is None
    assert mrf.normalize_semantic(None, None, 3.0) is None
    assert mrf.normalize_semantic(LABELS, STYLE_LABELS, 0) is None          # a weight of 0 is off, the maps still checked
    assert mrf.normalize_semantic(LABELS, STYLE_LABELS, 0.0) is None
    assert mrf.DEFAULT_SEMANTIC_WEIGHT == 1.0


def test_normaliser_forms():
    c, s, w = mrf.normalize_semantic(LABELS, STYLE_LABELS)
    assert w == 1.0 and c.shape == (2, 64, 96) and s.shape == (2, 70, 110) and c.dtype == s.dtype == np.float32
    assert np.array_equal(c, rg.normalize_regions(LABELS)) and np.array_equal(c.sum(axis=0), np.ones((64, 96), np.float32))
    # a float stack on one side, a label map on the other; the resolutions are each side's own
    stack = np.random.default_rng(0).random((2, 9, 7)).astype(np.float64)
    c2, s2, w2 = mrf.normalize_semantic(stack, STYLE_LABELS.astype(np.uint8), np.float32(0.25))
    assert w2 == 0.25 and c2.dtype == np.float32 and np.array_equal(c2, stack.astype(np.float32)) and s2.shape == (2, 70, 110)
    # R = 1 and R = 4
    assert mrf.normalize_semantic(np.zeros((5, 5), np.int64), np.ones((1, 4, 4), np.float32), 2)[2] == 2.0
    four = np.arange(16).reshape(4, 4) % 4
    assert mrf.normalize_semantic(four, four)[0].shape == (4, 4, 4)


@pytest.mark.parametrize("c,s,text", [
    (LABELS, None, "go together"), (None, STYLE_LABELS, "go together"),
    (LABELS, np.zeros((70, 110), np.int64), "semantic_content has 2 regions, semantic_style 1"),
    (np.zeros((3, 4, 4), np.float32), STYLE_LABELS, "semantic_content has 3 regions"),
    (LABELS + 3, STYLE_LABELS, "semantic_content"), (LABELS, -STYLE_LABELS, "semantic_style"),
    (LABELS * 2, STYLE_LABELS, "without gaps"), (LABELS.astype(np.float32), STYLE_LABELS, r"\(R,H,W\)"),
    (np.full((2, 4, 4), 1.5, np.float32), STYLE_LABELS, r"\[0,1\]"), (np.full((2, 4, 4), np.nan, np.float32), STYLE_LABELS, r"\[0,1\]"),
    (np.zeros((5, 4, 4), np.float32), np.zeros((5, 4, 4), np.float32), "regions"), ("sky", STYLE_LABELS, "semantic_content"),
])
def test_normaliser_refuses_maps(c, s, text):
    with pytest.raises(ValueError, match=text):
        mrf.normalize_semantic(c, s)


@pytest.mark.parametrize("weight", [-1.0, float("nan"), float("inf"), "1", None, True, [1.0]])
def test_normaliser_refuses_weights(weight):
    with pytest.raises(ValueError, match="semantic_weight"):
        mrf.normalize_semantic(LABELS, STYLE_LABELS, weight)
    with pytest.raises(ValueError, match="semantic_weight"):
        mrf.normalize_semantic(None, None, weight)                            # the off setting is validated too


def test_level_planes_follow_the_levels_of_the_term():
    setting = mrf.normalize_semantic(LABELS, STYLE_LABELS, 2.0)
    shapes, sshapes = [(64, 96), (32, 48)], [(70, 110), (35, 55)]
    planes = mrf.semantic_level_planes(setting, shapes, sshapes)
    assert [(p[0].shape, p[1].shape) for p in planes] == [((2, 64, 96), (2, 70, 110)), ((2, 32, 48), (2, 35, 55))]
    assert np.array_equal(planes[1][0], rg.resize_nearest(setting[0], 32, 48))
    assert np.array_equal(planes[1][1], rg.resize_nearest(setting[1], 35, 55))
    only = mrf.semantic_level_planes(setting, shapes, sshapes, levels=(1,))
    assert only[0] is None and np.array_equal(only[1][0], planes[1][0])


def test_module_is_still_free_of_torch():
    src = open(mrf.__file__).read()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)


# ---- the job function -------------------------------------------------------------------------------------------------------
def test_signature_is_the_mrf_functions_plus_three_keywords():
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf, neural_style_transfer_mrf_semantic
    base = list(inspect.signature(neural_style_transfer_mrf).parameters.values())
    ours = list(inspect.signature(neural_style_transfer_mrf_semantic).parameters.values())
    assert [(p.name, p.kind, p.default) for p in ours[:len(base)]] == [(p.name, p.kind, p.default) for p in base]
    extra = ours[len(base):]
    assert [(p.name, p.default) for p in extra] == [("semantic_content", None), ("semantic_style", None), ("semantic_weight", 1.0)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in extra)
    assert inspect.isasyncgenfunction(neural_style_transfer_mrf_semantic)


ARGS = (None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 2, 0.0, (), (), (), ())


def _collect(gen):
    async def run():
        return [item async for item in gen]
    return asyncio.run(run())


def test_off_delegates_and_on_goes_through_transfer_from(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd import patch_match as pm
    calls = []

    async def fake_mrf(*a, **kw):
        calls.append(("mrf", a, kw))
        yield 100, "mrf image"

    def fake_from(*a, device=None, start=None, patches=None, semantics=None, **kw):
        calls.append(("from", a, dict(kw, device=device, start=start, patches=patches, semantics=semantics)))

        async def gen():
            yield 100, "semantic image"
        return gen()

    monkeypatch.setattr(pm, "neural_style_transfer_mrf", fake_mrf)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    # no map: neural_style_transfer_mrf with its own keywords, whatever the weight
    for weight in (1.0, 0, 5.0):
        calls.clear()
        out = _collect(pm.neural_style_transfer_mrf_semantic(*ARGS, "dev", pooling="avg", mrf_weight=2.0, mrf_stride=2, semantic_weight=weight))
        assert out == [(100, "mrf image")]
        (kind, a, kw), = calls
        assert kind == "mrf" and a == ARGS + ("dev",) and kw["pooling"] == "avg"
        assert (kw["mrf_weight"], kw["mrf_stride"], kw["mrf_epsilon"], kw["mrf_levels"]) == (2.0, 2, 1e-5, None)
        assert not any(k.startswith("semantic") for k in kw)
    # maps: _transfer_from with the patches and the maps as they were given
    calls.clear()
    out = _collect(pm.neural_style_transfer_mrf_semantic(*ARGS, "dev", moment_weight=3.0, mrf_weight={3: 2.0}, mrf_levels=[1],
                                                          semantic_content=LABELS, semantic_style=STYLE_LABELS, semantic_weight=2))
    assert out == [(100, "semantic image")]
    (kind, a, kw), = calls
    assert kind == "from" and a == ARGS and kw["device"] == "dev" and kw["start"] is None and kw["moment_weight"] == 3.0
    assert kw["patches"] == ({3: 2.0}, 1, 1e-5, [1])
    assert kw["semantics"][0] is LABELS and kw["semantics"][1] is STYLE_LABELS and kw["semantics"][2] == 2
    # maps under a weight of 0: the plain MRF job
    calls.clear()
    _collect(pm.neural_style_transfer_mrf_semantic(*ARGS, mrf_weight=1.0, semantic_content=LABELS, semantic_style=STYLE_LABELS, semantic_weight=0))
    (kind, a, kw), = calls
    assert kind == "from" and kw["semantics"] is None and kw["patches"] == (1.0, 1, 1e-5, None)
    # refusals never reach either
    calls.clear()
    for bad, text in ((dict(mrf_weight=1.0, semantic_content=LABELS), "go together"),
                      (dict(mrf_weight=1.0, semantic_content=LABELS, semantic_style=np.zeros((70, 110), np.int64)), "regions"),
                      (dict(mrf_weight=1.0, semantic_content=LABELS, semantic_style=STYLE_LABELS, semantic_weight=-1.0), "semantic_weight"),
                      (dict(mrf_weight=1.0, semantic_weight=float("nan")), "semantic_weight"),
                      (dict(semantic_content=LABELS, semantic_style=STYLE_LABELS), "mrf_weight is off"),
                      (dict(mrf_weight=0.0, semantic_content=LABELS, semantic_style=STYLE_LABELS), "mrf_weight is off"),
                      (dict(mrf_weight=1.0, mrf_stride=9, semantic_content=LABELS, semantic_style=STYLE_LABELS), "mrf_stride")):
        with pytest.raises(ValueError, match=text):
            _collect(pm.neural_style_transfer_mrf_semantic(*ARGS, **bad))
    assert calls == []


def _pair(h=64, w=96, hs=70, ws=110):
    from artstyletransfer_amd import neural_style_transfer as impl
    return impl.ContentStylePair(("c", np.zeros((h, w, 3), np.float32)), ("s", np.zeros((hs, ws, 3), np.float32)))


def test_refusals_before_any_gpu_work(monkeypatch):
    """With the job's own settings: what the MRF term refuses stays refused under semantic maps, in _transfer_from, before
    _transfer is even created."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf_semantic

    def reached(*a, **kw):
        raise AssertionError("the job was started")

    monkeypatch.setattr(impl, "_transfer", reached)
    monkeypatch.setattr(impl, "shared_engine", reached)
    args = (_pair(),) + ARGS[1:]
    sem = dict(semantic_content=LABELS, semantic_style=STYLE_LABELS)
    cases = [
        (dict(mrf_weight=1.0, extra_styles=[np.zeros((32, 32, 3), np.float32)], **sem), "extra_styles"),
        (dict(mrf_weight=1.0, content_regions=np.zeros((64, 96), np.int64), style_regions=np.zeros((70, 110), np.int64), **sem),
         "content_regions"),
        (dict(mrf_weight={4: 1.0}, **sem), "not a style map"),
        (dict(mrf_weight=1.0, mrf_levels=[2], **sem), "mrf_levels"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            _collect(neural_style_transfer_mrf_semantic(*args, **kw))
    # _transfer_from itself holds the rule too (video.py and other drivers call it)
    with pytest.raises(ValueError, match="mrf_weight is off"):
        impl._transfer_from(*args, patches=None, semantics=(LABELS, STYLE_LABELS, 1.0))


def test_set_patch_semantics_reaches_the_device_job(monkeypatch):
    """NeuralStyleTransfer.set_patch_semantics is data of the next process: resized to the levels that carry the term and
    handed to the device job after set_patch_match; a job without it never calls the hook."""
    import torch
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def __init__(self, *a, **kw):
            seen.append(("made", sorted(kw)))

        def set_patch_match(self, *a):
            seen.append(("patches", a))

        def set_patch_semantics(self, planes, weight):
            seen.append(("semantics", planes, weight))

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
    nst.set_patch_match(2.0)
    nst.set_patch_semantics(LABELS, STYLE_LABELS, 2.0)
    assert run(nst) == []
    assert [s[0] for s in seen] == ["made", "patches", "semantics", "closed"]
    planes, weight = seen[2][1:]
    want_c, want_s = rg.normalize_regions(LABELS), rg.normalize_regions(STYLE_LABELS)
    assert weight == 2.0 and len(planes) == 2
    for lv, ((h, w), (hs, ws)) in enumerate(zip([(64, 96), (32, 48)], [(70, 110), (35, 55)])):
        assert np.array_equal(planes[lv][0], rg.resize_nearest(want_c, h, w))
        assert np.array_equal(planes[lv][1], rg.resize_nearest(want_s, hs, ws))
    # only the levels of the term
    seen.clear()
    nst.set_patch_match(2.0, levels=[1])
    assert run(nst) == []
    assert seen[2][0] == "semantics" and seen[2][1][0] is None and seen[2][1][1][0].shape == (2, 32, 48)
    # off again: the hook is not called
    seen.clear()
    nst.set_patch_semantics(None, None)
    assert run(nst) == [] and [s[0] for s in seen] == ["made", "patches", "closed"]
    seen.clear()
    nst.set_patch_semantics(LABELS, STYLE_LABELS, 0)
    assert run(nst) == [] and [s[0] for s in seen] == ["made", "patches", "closed"]
    # semantic maps without the term: refused in process, before the job exists
    seen.clear()
    nst.set_patch_semantics(LABELS, STYLE_LABELS)
    nst.set_patch_match(None)
    with pytest.raises(ValueError, match="mrf_weight is off"):
        run(nst)
    assert seen == []
    for bad in ((LABELS, None), (LABELS, np.zeros((70, 110), np.int64))):
        with pytest.raises(ValueError, match="semantic_"):
            nst.set_patch_semantics(*bad)
    with pytest.raises(ValueError, match="semantic_weight"):
        nst.set_patch_semantics(LABELS, STYLE_LABELS, -2.0)


def test_a_failing_hook_closes_the_job(monkeypatch):
    import torch
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def __init__(self, *a, **kw):
            pass

        def set_patch_match(self, *a):
            seen.append("patches")

        def set_patch_semantics(self, planes, weight):
            raise RuntimeError("refused on the device")

        def close(self):
            seen.append("closed")

    monkeypatch.setattr(impl, "_make_job", lambda *a, **kw: FakeJob())
    monkeypatch.setattr(impl.math_utils, "prepare_model", lambda *a: None)
    content, style = [np.zeros((64, 96, 3), np.float32)], [np.zeros((70, 110, 3), np.float32)]
    nst = impl.NeuralStyleTransfer(torch.device("cuda", 0), "vgg19", style, "adam")
    nst.set_patch_match(1.0)
    nst.set_patch_semantics(LABELS, STYLE_LABELS)

    async def go():
        return [x async for x in nst.process(content, content[0], 10.0, 0, 1e3, 4e5, 1e2, "c")]
    with pytest.raises(RuntimeError, match="refused on the device"):
        asyncio.run(go())
    assert seen == ["patches", "closed"]


# ---- the bindings -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nst_hip.h")).read()
    for name, nargs in (("nst_level_set_patch_guidance", 7), ("nst_level_patch_guidance", 6), ("nst_patch_descriptors", 9),
                        ("nst_patch_match_guided", 17)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    # the definition stands above the entry points, as the other terms have it
    at = header.index("int nst_level_set_patch_guidance(")
    for text in ("T(i,j) = cos(i,j) + gamma <d_i, e_j>", "rp_i = (float)(1 / sqrt(|P_i|^2 + epsilon))",
                 "sc   = feat + gamma * sem + 0.f", "entries r >= R zero"):
        assert text in header[:at], text


def test_job_settings_tables_are_untouched():
    """The maps are data of a job: no SETTINGS row, and the parameter lists of the two older job functions stay."""
    from artstyletransfer_amd import job_settings
    from artstyletransfer_amd.neural_style_transfer import neural_style_transfer
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf
    assert not any("semantic" in str(row).lower() for row in job_settings.SETTINGS)
    for fn in (neural_style_transfer, neural_style_transfer_mrf):
        assert not any(p.startswith("semantic") for p in inspect.signature(fn).parameters)
