"""CPU: the relaxed EMD term's host side - the normaliser (remd_modes.py), the stride rule, the job function's parameter list
and its delegation, the refusals before any GPU work, the hooks of NeuralStyleTransfer and the device job, the bindings, and
the reference's gradient (tests/remd_ref.py) against finite differences in fp64."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest
import torch

import remd_ref
from artstyletransfer_amd import _lib, remd_modes as remd

Z = 0.0


# ---- the normaliser -----------------------------------------------------------------------------------------------------------
def test_normalize_every_form():
    assert remd.normalize_remd() is None and remd.normalize_remd(0) is None and remd.normalize_remd([0] * 6) is None
    assert remd.normalize_remd({}) is None and remd.normalize_remd(0.0, 16, 1e-3, [0]) is None
    assert remd.normalize_remd(2.0) == ((Z, 2.0, 2.0, 2.0, Z, Z), 4096, 1e-5, None)
    # a number weighs those of relu2_1, relu3_1, relu4_1 that are style maps of the job
    assert remd.normalize_remd(2.0, style_indices=[0, 2, 5])[0] == (Z, Z, 2.0, Z, Z, Z)
    assert remd.normalize_remd([1, 0, 0, 0, 0, 3], 7, 0.5, (1, 0, 1)) == ((1.0, Z, Z, Z, Z, 3.0), 7, 0.5, (0, 1))
    assert remd.normalize_remd({"relu3_1": 4, 0: 1.5}, use_relu=True)[0] == (1.5, Z, 4.0, Z, Z, Z)
    assert remd.normalize_remd({4: 1.0}, style_indices=[0, 4])[0] == (Z, Z, Z, Z, 1.0, Z)
    assert remd.check_strides(3) == (3,) * 6 and remd.check_strides([1, 2, 3, 4, 5, 256]) == (1, 2, 3, 4, 5, 256)


def test_normalize_every_refusal():
    for bad in (-1.0, float("nan"), float("inf"), "1", True, [1] * 5, [1] * 7, [0, 0, -1, 0, 0, 0], {"relu9_9": 1.0}, {6: 1.0}, {1, 2}):
        with pytest.raises(ValueError, match="remd_weight"):
            remd.normalize_remd(bad)
    for bad in (0, -1, 1.5, "4096", True, None):
        with pytest.raises(ValueError, match="remd_samples"):
            remd.normalize_remd(1.0, bad)
        with pytest.raises(ValueError, match="remd_samples"):
            remd.normalize_remd(None, bad)                   # (the off setting is validated too)
    for bad in (0.0, -1e-5, float("nan"), float("inf"), "1e-5", True, None):
        with pytest.raises(ValueError, match="remd_epsilon"):
            remd.normalize_remd(1.0, 4096, bad)
    for bad in ([], 1, "0", [0, 8], [-1], [0.5], {0: 1}):
        with pytest.raises(ValueError, match="remd_levels"):
            remd.normalize_remd(1.0, 4096, 1e-5, bad)
    with pytest.raises(ValueError, match="remd_levels"):
        remd.normalize_remd(1.0, remd_levels=[2], levels_num=2)
    with pytest.raises(ValueError, match="not a style map"):
        remd.normalize_remd({4: 1.0}, style_indices=[0, 1, 2, 3, 5])
    with pytest.raises(ValueError, match="none of relu2_1, relu3_1, relu4_1"):
        remd.normalize_remd(1.0, style_indices=[0, 5])
    for bad in (0, 257, 1.0, True, [1] * 5, [1, 1, 1, 1, 1, 0], "1"):
        with pytest.raises(ValueError, match="strides"):
            remd.check_strides(bad, "strides")
    on = remd.normalize_remd(1.0)
    remd.check_exclusive(None, regions=object(), stripes=True, extra_styles=[1])
    remd.check_exclusive(on)
    for kw in (dict(regions=object()), dict(stripes=True), dict(extra_styles=[1])):
        with pytest.raises(ValueError, match="remd_weight cannot be combined"):
            remd.check_exclusive(on, **kw)


def test_module_is_free_of_torch():
    src = open(remd.__file__).read()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)


# ---- the stride rule --------------------------------------------------------------------------------------------------------------
STRIDES = [  # (hm, wm, samples, stride): the smallest s with ((hm-1)//s + 1) ((wm-1)//s + 1) <= samples
    (1, 1, 1, 1), (64, 64, 4096, 1), (64, 65, 4096, 2), (128, 192, 4096, 3), (512, 768, 4096, 10), (1024, 1536, 4096, 20),
    (256, 384, 4096, 5), (7, 33, 100, 2), (7, 33, 231, 1), (7, 33, 1, 33), (1, 300, 2, 150), (4096, 4096, 16384, 32),
    (100, 100, 1, 100), (257, 257, 4, 129), (512, 1, 2, 256),
]


@pytest.mark.parametrize("hm,wm,samples,stride", STRIDES)
def test_stride_rule(hm, wm, samples, stride):
    s = remd.stride_for(hm, wm, samples)
    assert s == stride
    assert remd.samples_of(hm, wm, s) <= samples
    assert s == 1 or remd.samples_of(hm, wm, s - 1) > samples
    # the count is the reference's
    assert remd.samples_of(hm, wm, s) == remd_ref.counts(hm, wm, s) == remd_ref.samples(torch.zeros((1, 2, hm, wm)), s).shape[0]


def test_stride_rule_refuses_a_map_that_needs_more_than_256():
    with pytest.raises(ValueError, match="needs a stride above 256"):
        remd.stride_for(257, 257, 1)
    with pytest.raises(ValueError, match="needs a stride above 256"):
        remd.stride_for(1, 1000, 3)
    with pytest.raises(ValueError, match="needs a stride above 256"):
        remd.stride_for(513, 1, 2)
    # per level and map: MAP_SCALE halves the image size; unweighted maps get 1; levels outside remd_levels get None
    st = remd.normalize_remd({1: 1.0, 3: 1.0}, 100, 1e-5, [0])
    out = remd.level_strides(st, [(64, 96), (32, 48)], [(70, 110), (35, 55)])
    assert out == [((1, 4, 1, 1, 1, 1), (1, 5, 1, 2, 1, 1)), None]
    assert remd.level_strides(None, [(64, 96)], [(64, 96)]) == [None]
    with pytest.raises(ValueError, match="needs a stride above 256"):
        remd.level_strides(remd.normalize_remd({0: 1.0}, 1), [(1024, 1024)], [(64, 64)])
    with pytest.raises(ValueError, match="pools to nothing"):
        remd.level_strides(remd.normalize_remd({5: 1.0}), [(64, 64)], [(8, 8)])
    with pytest.raises(ValueError, match="remd_levels"):
        remd.level_strides(remd.normalize_remd(1.0, remd_levels=[3]), [(64, 64)], [(64, 64)])


# ---- the job function -------------------------------------------------------------------------------------------------------
def test_signature_is_the_histogram_jobs_plus_four_keywords():
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist
    from artstyletransfer_amd.remd_loss import neural_style_transfer_remd
    base = list(inspect.signature(neural_style_transfer_hist).parameters.values())
    ours = list(inspect.signature(neural_style_transfer_remd).parameters.values())
    assert [(p.name, p.kind, p.default) for p in ours[:len(base)]] == [(p.name, p.kind, p.default) for p in base]
    extra = ours[len(base):]
    assert [(p.name, p.default) for p in extra] == [("remd_weight", None), ("remd_samples", 4096), ("remd_epsilon", 1e-5), ("remd_levels", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in extra)
    assert inspect.isasyncgenfunction(neural_style_transfer_remd)


ARGS = (None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 2, 0.0, (), (), (), ())


def _collect(gen):
    async def run():
        return [item async for item in gen]
    return asyncio.run(run())


def test_off_delegates_and_on_goes_through_transfer_from(monkeypatch):
    from artstyletransfer_amd import histogram_loss, neural_style_transfer as impl
    from artstyletransfer_amd.remd_loss import neural_style_transfer_remd
    calls = []

    async def fake_hist(*a, **kw):
        calls.append(("hist", a, kw))
        yield 100, "plain image"

    def fake_from(*a, **kw):
        calls.append(("from", a, kw))

        async def gen():
            yield 100, "remd image"
        return gen()

    monkeypatch.setattr(histogram_loss, "neural_style_transfer_hist", fake_hist)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    for off in (None, 0, 0.0, [0] * 6, {}):
        calls.clear()
        out = _collect(neural_style_transfer_remd(*ARGS, "dev", pooling="avg", mrf_weight=2.0, hist_weight=3.0, hist_bins=16, remd_weight=off,
                                                  remd_samples=64))
        assert out == [(100, "plain image")]
        (kind, a, kw), = calls
        assert kind == "hist" and a == ARGS + ("dev",) and kw["pooling"] == "avg" and kw["mrf_weight"] == 2.0
        assert kw["hist_weight"] == 3.0 and kw["hist_bins"] == 16 and not any(k.startswith("remd_") for k in kw)
    calls.clear()
    out = _collect(neural_style_transfer_remd(*ARGS, "dev", moment_weight=3.0, remd_weight={3: 2.0}, remd_samples=64, remd_epsilon=1e-3,
                                              remd_levels=[1]))
    assert out == [(100, "remd image")]
    (kind, a, kw), = calls
    assert kind == "from" and a == ARGS and kw["device"] == "dev" and kw["start"] is None and kw["moment_weight"] == 3.0
    assert kw["remd"] == ({3: 2.0}, 64, 1e-3, [1]) and kw["patches"] is None and kw["semantics"] is None and kw["histograms"] is None
    # beside the MRF term, its semantic maps and the histogram loss
    calls.clear()
    sem = np.zeros((8, 8), np.int64)
    _collect(neural_style_transfer_remd(*ARGS, mrf_weight=1.0, mrf_stride=2, semantic_content=sem, semantic_style=sem, hist_weight=1.0,
                                        remd_weight=1.0))
    (kind, a, kw), = calls
    assert kw["patches"] == (1.0, 2, 1e-5, None) and kw["semantics"][0] is sem and kw["semantics"][2] == 1.0
    assert kw["histograms"] == (1.0, 256, None) and kw["remd"] == (1.0, 4096, 1e-5, None)
    # a malformed setting never reaches either
    calls.clear()
    for bad in (dict(remd_weight=-1.0), dict(remd_weight=1.0, remd_samples=0), dict(remd_weight=None, remd_samples=-3),
                dict(remd_weight=1.0, remd_epsilon=0.0), dict(remd_weight=1.0, remd_levels=[])):
        with pytest.raises(ValueError, match="remd_"):
            _collect(neural_style_transfer_remd(*ARGS, **bad))
    with pytest.raises(ValueError, match="mrf_weight is off"):
        _collect(neural_style_transfer_remd(*ARGS, semantic_content=sem, semantic_style=sem, remd_weight=1.0))
    assert calls == []


def _pair(h=64, w=96, hs=70, ws=110):
    from artstyletransfer_amd import neural_style_transfer as impl
    return impl.ContentStylePair(("c", np.zeros((h, w, 3), np.float32)), ("s", np.zeros((hs, ws, 3), np.float32)))


def test_refusals_before_any_gpu_work(monkeypatch):
    """With the job's style set and sizes: everything is refused in _transfer_from, before _transfer is even created."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.remd_loss import neural_style_transfer_remd

    def reached(*a, **kw):
        raise AssertionError("the job was started")

    monkeypatch.setattr(impl, "_transfer", reached)
    monkeypatch.setattr(impl, "shared_engine", reached)
    args = (_pair(),) + ARGS[1:]
    cases = [
        (dict(remd_weight=1.0, extra_styles=[np.zeros((32, 32, 3), np.float32)]), "extra_styles"),
        (dict(remd_weight=1.0, content_regions=np.zeros((64, 96), np.int64), style_regions=np.zeros((70, 110), np.int64)), "content_regions"),
        (dict(remd_weight={4: 1.0}), "not a style map"),
        (dict(remd_weight=1.0, style_layers=[0, 5]), "none of relu2_1, relu3_1, relu4_1"),
        (dict(remd_weight=1.0, remd_levels=[2]), "remd_levels"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            _collect(neural_style_transfer_remd(*args, **kw))
    # a map that needs a stride above 256: relu1_1 of a 600 x 600 level under one sample
    big = (_pair(600, 600, 70, 110),) + ARGS[1:8] + (1,) + ARGS[9:]
    with pytest.raises(ValueError, match="needs a stride above 256"):
        _collect(neural_style_transfer_remd(*big, remd_weight={0: 1.0}, remd_samples=1))


def test_stripe_sharding_refuses_the_term():
    with pytest.raises(ValueError, match="remd_weight cannot be combined with stripe sharding"):
        remd.check_exclusive(((Z, 1.0, Z, Z, Z, Z), (1,) * 6, (1,) * 6, 1e-5, (64, 96)), stripes=True)
    src = open(os.path.join(os.path.dirname(remd.__file__), "engine.py")).read()
    assert "_remd.check_exclusive(" in src[src.index("def shard_stripes"):]


def test_set_relaxed_emd_reaches_the_device_job_after_the_other_hooks(monkeypatch):
    """NeuralStyleTransfer.set_relaxed_emd is data of the next process: handed to the device job once it exists, after
    set_patch_match and set_histogram_loss, with the checked weights and the strides of every level; a job without it never
    calls the hook."""
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def __init__(self, *a, **kw):
            seen.append(("made", sorted(kw)))

        def set_patch_match(self, *a):
            seen.append(("patches", a))

        def set_histogram_loss(self, *a):
            seen.append(("histograms", a))

        def set_relaxed_emd(self, *a):
            seen.append(("remd", a))

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
    nst.set_relaxed_emd(2.0, samples=100, epsilon=1e-3, levels=[1])
    assert run(nst) == []
    w = (Z, 2.0, 2.0, 2.0, Z, Z)
    # level 1: maps of 16x24 / 8x12 / 4x6 and of 17x27 / 8x13 / 4x6
    assert seen == [("made", []), ("remd", (w, [None, ((1, 2, 1, 1, 1, 1), (1, 3, 2, 1, 1, 1))], 1e-3)), ("closed",)]
    seen.clear()
    nst.set_patch_match({2: 1.0}, levels=[0])
    nst.set_histogram_loss(1.0)
    assert run(nst) == []
    assert [s[0] for s in seen] == ["made", "patches", "histograms", "remd", "closed"]
    seen.clear()
    nst.set_patch_match(None)
    nst.set_histogram_loss(None)
    nst.set_relaxed_emd(None)
    assert run(nst) == [] and seen == [("made", []), ("closed",)]
    nst.set_relaxed_emd(0)
    assert run(nst) == [] and seen == [("made", []), ("closed",)] * 2
    # refusals of process(), where the style set is known: before the job exists
    seen.clear()
    nst.set_relaxed_emd({4: 1.0})
    with pytest.raises(ValueError, match="not a style map"):
        run(nst)
    nst.set_relaxed_emd(1.0)
    nst.set_feature_maps(4, [0, 5])
    with pytest.raises(ValueError, match="none of relu2_1, relu3_1, relu4_1"):
        run(nst)
    assert seen == []
    with pytest.raises(ValueError, match="remd_samples"):
        nst.set_relaxed_emd(1.0, samples=0)


def test_device_job_hook_gives_each_level_its_style_image():
    import contextlib
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class Engine:
        def set_remd(self, level, style, weights, si, ss, eps):
            seen.append((level, style, weights, si, ss, eps))

    job = object.__new__(impl._DeviceJob)
    job.engine, job.dev, job.job_stream = Engine(), None, None
    job.style_levels = [lambda: "s0", lambda: "s1", lambda: "s2"]
    null = lambda *a, **kw: contextlib.nullcontext()                   # noqa: E731
    orig = torch.cuda.device, torch.cuda.stream
    torch.cuda.device, torch.cuda.stream = null, null
    try:
        job.set_relaxed_emd((1.0,) * 6, [("a0", "b0"), None, ("a2", "b2")], 1e-4)
    finally:
        torch.cuda.device, torch.cuda.stream = orig
    assert seen == [(0, "s0", (1.0,) * 6, "a0", "b0", 1e-4), (2, "s2", (1.0,) * 6, "a2", "b2", 1e-4)]


# ---- the bindings -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_in_the_header_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nst_hip.h")).read()
    for name, nargs in (("nst_level_set_remd", 10), ("nst_level_remd", 8), ("nst_job_remd_losses", 3), ("nst_level_remd_matches", 7),
                        ("nst_remd_match", 14), ("nst_remd_term", 19)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    lib_path = os.path.join(root, "artstyletransfer_amd", "libnst_hip.so")
    if os.path.exists(lib_path):                     # (the built library exports them: no GPU needed to look)
        import ctypes
        lib = ctypes.CDLL(lib_path)
        for name in _lib.SYMBOLS:
            if "remd" in name:
                assert hasattr(lib, name), name
    from artstyletransfer_amd.engine import StyleEngine
    for method in ("set_remd", "clear_remd", "remd_setting", "remd_losses", "remd_matches", "remd_match", "remd_term"):
        assert callable(getattr(StyleEngine, method)), method


def test_job_settings_tables_are_untouched():
    """The term is data of a job: no SETTINGS row, no keyword of the existing job functions, no Config field."""
    from artstyletransfer_amd import config, job_settings
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist
    from artstyletransfer_amd.neural_style_transfer import neural_style_transfer
    assert not any("remd" in str(row).lower() for row in job_settings.SETTINGS)
    for fn in (neural_style_transfer, neural_style_transfer_hist):
        assert not any(p.startswith("remd") for p in inspect.signature(fn).parameters)
    assert "remd" not in open(config.__file__).read().lower()


# ---- the reference's gradient against finite differences, fp64 -------------------------------------------------------------------
def _fd_case(seed, c, h, w, hs, ws, si, ss):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((1, c, h, w), generator=g, dtype=torch.float64)
    fs = torch.randn((1, c, hs, ws), generator=g, dtype=torch.float64)
    return f, fs


@pytest.mark.parametrize("side", [0, 1])
def test_reference_gradient_vs_finite_differences(side):
    """Central differences of the reference's value at FIXED matches, every element of a small map, fp64: side A, and side B
    with matches chosen so that several style samples share one image sample and some image samples have none.  Also the
    closed form of the definition, d(i,j) = rp_i ((cos rp_i) X_i - rq_j Y_j), against autograd."""
    c, h, w, hs, ws, si, ss = 6, 3, 5, 4, 3, 2, 1
    f, fs = _fd_case(5, c, h, w, hs, ws, si, ss)
    n, m = remd_ref.counts(h, w, si), remd_ref.counts(hs, ws, ss)
    assert (n, m) == (6, 12)
    nnA = torch.tensor([3, 0, 11, 3, 7, 5])
    nnB = torch.tensor([0, 2, 2, 5, 2, 0, 1, 2, 5, 5, 0, 2])          # image sample 2 five times, 3 and 4 never
    x = f.clone().requires_grad_(True)
    v, sd, rA, rB = remd_ref.value(x, fs, nnA, nnB, si, ss, side=side)
    assert sd == side
    v.backward()
    grad = x.grad.clone()
    step = 1e-6
    fd = torch.zeros_like(f)
    flat, out = f.reshape(-1), fd.reshape(-1)
    for k in range(flat.numel()):
        keep = float(flat[k])
        flat[k] = keep + step
        up = float(remd_ref.value(f, fs, nnA, nnB, si, ss, side=side)[0])
        flat[k] = keep - step
        dn = float(remd_ref.value(f, fs, nnA, nnB, si, ss, side=side)[0])
        flat[k] = keep
        out[k] = (up - dn) / (2 * step)
    err = float((grad - fd).norm() / fd.norm())
    assert err < 1e-8, err
    # zero off the sample grid
    off = torch.ones((h, w), dtype=torch.bool)
    off[::si, ::si] = False
    assert not grad[0][:, off].any() and grad[0][:, ~off].any()
    # the closed form
    xs, ys = remd_ref.samples(f, si), remd_ref.samples(fs, ss)
    rp, rq = remd_ref.rnorm(xs), remd_ref.rnorm(ys)
    closed = torch.zeros_like(xs)
    if side == 0:
        for i in range(n):
            j = int(nnA[i])
            cos = float((xs[i] * ys[j]).sum() * rp[i] * rq[j])
            closed[i] = rp[i] * ((cos * rp[i]) * xs[i] - rq[j] * ys[j]) / n
    else:
        for j in range(m):
            i = int(nnB[j])
            cos = float((xs[i] * ys[j]).sum() * rp[i] * rq[j])
            closed[i] += rp[i] * ((cos * rp[i]) * xs[i] - rq[j] * ys[j]) / m
    got = remd_ref.samples(grad, si)
    assert float((got - closed).norm() / closed.norm()) < 1e-12
    if side == 1:
        assert not got[3].any() and not got[4].any() and got[2].any()


def test_reference_matches_and_side():
    """The reference's arg-max takes the lowest index of equal maxima in both directions, and the decided side is A when
    rA >= rB - on a 1x1 pair rA = rB exactly."""
    cos = torch.tensor([[0.5, 0.9, 0.9], [0.9, 0.1, 0.9], [0.9, 0.9, 0.2]])
    a, b = remd_ref.matches(cos)
    assert a.tolist() == [1, 0, 0] and b.tolist() == [1, 0, 0]
    f, fs = _fd_case(1, 4, 1, 1, 1, 1, 1, 1)
    z = torch.zeros(1, dtype=torch.long)
    v, side, rA, rB = remd_ref.value(f, fs, z, z)
    assert float(rA) == float(rB) and side == 0 and float(v) == float(rA)
