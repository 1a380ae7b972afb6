"""CPU: the self-similarity content term (nst_level_set_selfsim) - the reference of tests/selfsim_ref.py against finite
differences, its value's range, the Python setting parser (selfsim_modes) with the stride rule, the defaults and every refusal,
and the job function's plumbing.  No GPU."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest
import torch

import selfsim_ref
from artstyletransfer_amd import _lib, selfsim_modes as selfsim

Z = 0.0


def _map(c, h, w, seed, base=None, scale=1.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((1, c, h, w), generator=g, dtype=dtype)
    return torch.relu(z if base is None else base + scale * z)


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 4, 5, 1, "free"), (16, 6, 7, 2, "near"), (4, 3, 1, 1, "free"), (32, 5, 5, 1, "near")])
def test_reference_gradient_vs_central_differences(shape):
    """fp64: autograd of the value under its own signs against central differences of the value itself (the signs are locally
    constant away from ties: the step is 1e-6 and the smallest |N - M| off the diagonal is checked to be far above what that
    step moves), and of value_under at fixed signs."""
    c, h, w, st, kind = shape
    fc = _map(c, h, w, 1)
    f = _map(c, h, w, 2) if kind == "free" else _map(c, h, w, 2, base=fc, scale=0.3)
    f = f + 0.05                                               # (off the ReLU's corner: the map is a free variable here)
    sg, d = selfsim_ref.signs(f, fc, st)
    n = d.shape[0]
    off = ~torch.eye(n, dtype=torch.bool)
    assert float(d[off].abs().min()) > 1e-7
    x = f.clone().requires_grad_(True)
    v = selfsim_ref.value_under(x, fc, sg, st)
    v.backward()
    g = x.grad.clone()
    assert float(v.detach()) == pytest.approx(float(selfsim_ref.value(f, fc, st)), rel=1e-12)
    x2 = f.clone().requires_grad_(True)
    selfsim_ref.value(x2, fc, st).backward()
    assert torch.allclose(x2.grad, g, rtol=1e-10, atol=1e-14)
    rng = np.random.default_rng(0)
    step = 1e-6
    flat = f.reshape(-1)
    for k in rng.choice(flat.numel(), size=min(40, flat.numel()), replace=False):
        e = torch.zeros_like(flat)
        e[k] = step
        up, dn = (flat + e).reshape(f.shape), (flat - e).reshape(f.shape)
        fd = (float(selfsim_ref.value(up, fc, st)) - float(selfsim_ref.value(dn, fc, st))) / (2 * step)
        fd_fixed = (float(selfsim_ref.value_under(up, fc, sg, st)) - float(selfsim_ref.value_under(dn, fc, sg, st))) / (2 * step)
        got = float(g.reshape(-1)[k])
        assert fd == pytest.approx(got, rel=2e-5, abs=1e-9), (k, fd, got)
        assert fd_fixed == pytest.approx(got, rel=2e-5, abs=1e-9), (k, fd_fixed, got)
    # the gradient reaches sampled pixels only
    mask = torch.ones((h, w), dtype=torch.bool)
    mask[::st, ::st] = False
    assert not g[0][:, mask].any()


def test_reference_value_is_zero_at_the_content_and_lies_in_0_2():
    for c, h, w, st in ((8, 4, 5, 1), (16, 9, 7, 2), (4, 1, 1, 1), (64, 6, 6, 3)):
        fc = _map(c, h, w, 3)
        assert float(selfsim_ref.value(fc.clone(), fc, st)) == 0.0
        sg, d = selfsim_ref.signs(fc.clone(), fc, st)
        assert not sg.any()
        for seed in range(4):
            v = float(selfsim_ref.value(_map(c, h, w, 10 + seed) * 10.0 ** seed, fc, st))
            assert 0.0 <= v <= 2.0
        n = selfsim_ref.counts(h, w, st)
        d, s, nm = selfsim_ref.matrices(fc, st)
        assert tuple(d.shape) == (n, n) and not d.diagonal().any() and float(d.min()) >= 0.0
        if n > 1:
            assert torch.allclose(nm.sum(dim=0), torch.ones(n, dtype=nm.dtype), atol=1e-3)      # (columns are distributions up to eps)
    # the extremes: a content whose samples are all alike against an image with one outlier stays inside [0, 2]
    one = torch.ones((1, 8, 3, 3), dtype=torch.float64)
    spike = one.clone()
    spike[0, :, 1, 1] = torch.tensor([5.0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float64)
    assert 0.0 <= float(selfsim_ref.value(spike, one)) <= 2.0
    assert float(selfsim_ref.value(one, one.clone())) == 0.0
    assert selfsim_ref.clamped(_map(8, 4, 5, 5)) == 0


# ---- the setting parser ---------------------------------------------------------------------------------------------------------
def test_normalize_every_form():
    assert selfsim.normalize_selfsim() is None and selfsim.normalize_selfsim(0) is None and selfsim.normalize_selfsim([0] * 6) is None
    assert selfsim.normalize_selfsim({}) is None
    # a bare number weighs the job's content map, whichever it is
    assert selfsim.normalize_selfsim(3.0) == ((Z, Z, Z, Z, 3.0, Z), 1024, 1e-5, None)
    assert selfsim.normalize_selfsim(3, content_index=5, style_indices=(0, 1))[0] == (Z, Z, Z, Z, Z, 3.0)
    assert selfsim.normalize_selfsim(2.0, 64, 1e-3, [1, 0, 1]) == ((Z, Z, Z, Z, 2.0, Z), 64, 1e-3, (0, 1))
    # any map the job uses: its content map or a style map
    assert selfsim.normalize_selfsim({3: 1.0, 4: 2.0}, content_index=4, style_indices=(0, 1, 2, 3, 5))[0] == (Z, Z, Z, 1.0, 2.0, Z)
    assert selfsim.normalize_selfsim({"relu4_1": 1.0, "conv4_2": 2.0})[0] == (Z, Z, Z, 1.0, 2.0, Z)
    assert selfsim.normalize_selfsim([1, 0, 0, 0, 0, 0.5])[0] == (1.0, Z, Z, Z, Z, 0.5)
    assert selfsim.DEFAULT_SAMPLES == 1024 and selfsim.MAX_SAMPLES == 4096 and selfsim.DEFAULT_EPSILON == 1e-5
    assert selfsim.used_maps() is None and selfsim.used_maps(5, (0, 1)) == (0, 1, 5) and selfsim.used_maps(None, (0, 4)) == (0, 4)


def test_normalize_every_refusal():
    for bad in (-1.0, float("nan"), float("inf"), True, "1", [1.0] * 5, {9: 1.0}, {"relu9_9": 1.0}, {3: -1.0}, {1, 2}):
        with pytest.raises(ValueError, match="selfsim_weight"):
            selfsim.normalize_selfsim(bad)
    for bad in (0, -1, 4097, 1.5, True, "64", None):
        with pytest.raises(ValueError, match="selfsim_samples must be an integer 1..4096"):
            selfsim.normalize_selfsim(1.0, bad)
    assert selfsim.normalize_selfsim(1.0, 4096)[1] == 4096 and selfsim.normalize_selfsim(1.0, 1)[1] == 1
    for bad in (0.0, -1e-5, float("nan"), float("inf"), True, "x", None):
        with pytest.raises(ValueError, match="selfsim_epsilon"):
            selfsim.normalize_selfsim(1.0, 64, bad)
    for bad in ([], 1, "0", {0: 1}, [0.5], [-1], [8], [True]):
        with pytest.raises(ValueError, match="selfsim_levels"):
            selfsim.normalize_selfsim(1.0, 64, 1e-5, bad)
    with pytest.raises(ValueError, match="selfsim_levels"):
        selfsim.normalize_selfsim(1.0, 64, 1e-5, [2], levels_num=2)
    # the off setting is validated too
    with pytest.raises(ValueError, match="selfsim_samples"):
        selfsim.normalize_selfsim(None, 0)
    # a positive weight on a map the job does not use
    with pytest.raises(ValueError, match="map 4 has a positive weight but is not a map of the job"):
        selfsim.normalize_selfsim({4: 1.0}, content_index=5, style_indices=(0, 1, 2, 3))
    with pytest.raises(ValueError, match="map 5 has a positive weight but is not a map of the job"):
        selfsim.normalize_selfsim([0, 0, 0, 0, 1, 1], content_index=4, style_indices=(0, 1))
    on = selfsim.normalize_selfsim(1.0)
    for kw in (dict(extra_styles=[object()]), dict(regions=object()), dict(stripes=True)):
        with pytest.raises(ValueError, match="selfsim_weight cannot be combined"):
            selfsim.check_exclusive(on, **kw)
        selfsim.check_exclusive(None, **kw)


def test_module_is_free_of_torch():
    src = open(selfsim.__file__).read()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)


STRIDES = [  # (hm, wm, samples, stride): the smallest s with ((hm-1)//s + 1) ((wm-1)//s + 1) <= samples
    (1, 1, 1, 1), (32, 32, 1024, 1), (32, 33, 1024, 2), (128, 192, 1024, 5), (128, 192, 4096, 3), (64, 96, 1024, 3), (7, 33, 231, 1),
    (7, 33, 1, 33), (1, 300, 2, 150), (100, 100, 1, 100), (257, 257, 4, 129), (512, 1, 2, 256), (1024, 1536, 4096, 20),
]


@pytest.mark.parametrize("hm,wm,samples,stride", STRIDES)
def test_stride_rule(hm, wm, samples, stride):
    s = selfsim.stride_for(hm, wm, samples)
    assert s == stride
    assert selfsim.samples_of(hm, wm, s) <= samples
    assert s == 1 or selfsim.samples_of(hm, wm, s - 1) > samples
    assert selfsim.samples_of(hm, wm, s) == selfsim_ref.counts(hm, wm, s) == selfsim_ref.samples(torch.zeros((1, 2, hm, wm)), s).shape[0]


def test_stride_rule_per_level_and_its_refusals():
    with pytest.raises(ValueError, match="needs a stride above 256"):
        selfsim.stride_for(257, 257, 1)
    with pytest.raises(ValueError, match="selfsim_samples"):
        selfsim.stride_for(64, 64, 5000)
    # per level and map: MAP_SCALE halves the image size; unweighted maps get 1; levels outside selfsim_levels get None
    st = selfsim.normalize_selfsim({1: 1.0, 4: 1.0}, 100, 1e-5, [0])
    assert selfsim.level_strides(st, [(64, 96), (32, 48)]) == [(1, 4, 1, 1, 1, 1), None]
    assert selfsim.level_strides(selfsim.normalize_selfsim(1.0), [(1024, 1536), (512, 768)]) == [(1, 1, 1, 1, 5, 1), (1, 1, 1, 1, 3, 1)]
    assert selfsim.level_strides(None, [(64, 96)]) == [None]
    with pytest.raises(ValueError, match="needs a stride above 256"):
        selfsim.level_strides(selfsim.normalize_selfsim({0: 1.0}, 1), [(1024, 1024)])
    with pytest.raises(ValueError, match="pools to nothing"):
        selfsim.level_strides(selfsim.normalize_selfsim({5: 1.0}), [(8, 8)])
    with pytest.raises(ValueError, match="selfsim_levels"):
        selfsim.level_strides(selfsim.normalize_selfsim(1.0, selfsim_levels=[3]), [(64, 64)])
    assert selfsim.check_strides(2) == (2,) * 6 and selfsim.check_strides([1, 2, 3, 4, 5, 6]) == (1, 2, 3, 4, 5, 6)
    for bad in (0, 257, [1] * 5, "1", 1.5):
        with pytest.raises(ValueError):
            selfsim.check_strides(bad)


# ---- the job function -------------------------------------------------------------------------------------------------------
def test_signature_is_the_remd_jobs_plus_four_keywords():
    from artstyletransfer_amd.remd_loss import neural_style_transfer_remd
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim
    base = list(inspect.signature(neural_style_transfer_remd).parameters.values())
    ours = list(inspect.signature(neural_style_transfer_selfsim).parameters.values())
    assert [(p.name, p.kind, p.default) for p in ours[:len(base)]] == [(p.name, p.kind, p.default) for p in base]
    extra = ours[len(base):]
    assert [(p.name, p.default) for p in extra] == [("selfsim_weight", None), ("selfsim_samples", 1024), ("selfsim_epsilon", 1e-5),
                                                    ("selfsim_levels", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in extra)
    assert inspect.isasyncgenfunction(neural_style_transfer_selfsim)
    # the relaxed EMD job's own parameter list ends where it ended
    assert [p.name for p in base][-4:] == ["remd_weight", "remd_samples", "remd_epsilon", "remd_levels"]


ARGS = (None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 2, 0.0, (), (), (), ())


def _collect(gen):
    async def run():
        return [item async for item in gen]
    return asyncio.run(run())


def test_off_delegates_and_on_goes_through_transfer_from(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl, remd_loss
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim
    calls = []

    async def fake_remd(*a, **kw):
        calls.append(("remd", a, kw))
        yield 100, "plain image"

    def fake_from(*a, **kw):
        calls.append(("from", a, kw))

        async def gen():
            yield 100, "selfsim image"
        return gen()

    monkeypatch.setattr(remd_loss, "neural_style_transfer_remd", fake_remd)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    for off in (None, 0, 0.0, [0] * 6, {}):
        calls.clear()
        out = _collect(neural_style_transfer_selfsim(*ARGS, "dev", pooling="avg", mrf_weight=2.0, remd_weight=3.0, remd_samples=16,
                                                     selfsim_weight=off, selfsim_samples=64))
        assert out == [(100, "plain image")]
        (kind, a, kw), = calls
        assert kind == "remd" and a == ARGS + ("dev",) and kw["pooling"] == "avg" and kw["mrf_weight"] == 2.0
        assert kw["remd_weight"] == 3.0 and kw["remd_samples"] == 16 and not any(k.startswith("selfsim_") for k in kw)
    calls.clear()
    out = _collect(neural_style_transfer_selfsim(*ARGS, "dev", moment_weight=3.0, selfsim_weight={3: 2.0}, selfsim_samples=64,
                                                 selfsim_epsilon=1e-3, selfsim_levels=[1]))
    assert out == [(100, "selfsim image")]
    (kind, a, kw), = calls
    assert kind == "from" and a == ARGS and kw["device"] == "dev" and kw["start"] is None and kw["moment_weight"] == 3.0
    assert kw["selfsim"] == ({3: 2.0}, 64, 1e-3, [1])
    assert kw["patches"] is None and kw["semantics"] is None and kw["histograms"] is None and kw["remd"] is None
    # beside the other per-map terms
    calls.clear()
    _collect(neural_style_transfer_selfsim(*ARGS, mrf_weight=1.0, mrf_stride=2, hist_weight=1.0, remd_weight=2.0, selfsim_weight=1.0))
    (kind, a, kw), = calls
    assert kw["patches"] == (1.0, 2, 1e-5, None) and kw["histograms"] == (1.0, 256, None) and kw["remd"] == (2.0, 4096, 1e-5, None)
    assert kw["selfsim"] == (1.0, 1024, 1e-5, None)
    # a malformed setting never reaches either
    calls.clear()
    for bad in (dict(selfsim_weight=-1.0), dict(selfsim_weight=1.0, selfsim_samples=0), dict(selfsim_weight=None, selfsim_samples=5000),
                dict(selfsim_weight=1.0, selfsim_epsilon=0.0), dict(selfsim_weight=1.0, selfsim_levels=[])):
        with pytest.raises(ValueError, match="selfsim_"):
            _collect(neural_style_transfer_selfsim(*ARGS, **bad))
    assert calls == []


def _pair(h=64, w=96, hs=70, ws=110):
    from artstyletransfer_amd import neural_style_transfer as impl
    return impl.ContentStylePair(("c", np.zeros((h, w, 3), np.float32)), ("s", np.zeros((hs, ws, 3), np.float32)))


def test_refusals_before_any_gpu_work(monkeypatch):
    """With the job's taps and sizes: everything is refused in _transfer_from, before _transfer is even created."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim

    def reached(*a, **kw):
        raise AssertionError("the job was started")

    monkeypatch.setattr(impl, "_transfer", reached)
    monkeypatch.setattr(impl, "shared_engine", reached)
    args = (_pair(),) + ARGS[1:]
    cases = [
        (dict(selfsim_weight=1.0, extra_styles=[np.zeros((32, 32, 3), np.float32)]), "extra_styles"),
        (dict(selfsim_weight=1.0, content_regions=np.zeros((64, 96), np.int64), style_regions=np.zeros((70, 110), np.int64)), "content_regions"),
        (dict(selfsim_weight={4: 1.0}, content_layer=5, style_layers=[0, 1, 2, 3]), "not a map of the job"),
        (dict(selfsim_weight={2: 1.0}, style_layers=[0, 5]), "not a map of the job"),
        (dict(selfsim_weight=1.0, selfsim_levels=[2]), "selfsim_levels"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            _collect(neural_style_transfer_selfsim(*args, **kw))
    # a map that needs a stride above 256: relu1_1 of a 1:2 level (short edge 256) under one sample
    big = (_pair(600, 1200, 70, 110),) + ARGS[1:8] + (1,) + ARGS[9:]
    with pytest.raises(ValueError, match="needs a stride above 256"):
        _collect(neural_style_transfer_selfsim(*big, selfsim_weight={0: 1.0}, selfsim_samples=1))


def test_a_weight_on_the_content_map_and_on_a_style_map_reaches_the_job(monkeypatch):
    """What is allowed: the content map under its own taps (a bare number follows content_layer), and a style map."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim
    seen = []

    def fake_transfer(*a):
        seen.append(a[-1])

        async def gen():
            yield 100, "image"
        return gen()

    monkeypatch.setattr(impl, "_transfer", fake_transfer)
    args = (_pair(),) + ARGS[1:]
    for kw in (dict(selfsim_weight=1.0), dict(selfsim_weight=1.0, content_layer=5, style_layers=[0, 1, 2, 3]),
               dict(selfsim_weight={3: 1.0, 4: 2.0}), dict(selfsim_weight={"relu5_1": 1.0}, content_layer=5, style_layers=[0, 1])):
        assert _collect(neural_style_transfer_selfsim(*args, **kw)) == [(100, "image")]
    assert [s[0] for s in seen] == [1.0, 1.0, {3: 1.0, 4: 2.0}, {"relu5_1": 1.0}]


def test_stripe_sharding_refuses_the_term():
    with pytest.raises(ValueError, match="selfsim_weight cannot be combined with stripe sharding"):
        selfsim.check_exclusive(((Z, 1.0, Z, Z, Z, Z), (1,) * 6, 1e-5), stripes=True)
    src = open(os.path.join(os.path.dirname(selfsim.__file__), "engine.py")).read()
    assert "_selfsim.check_exclusive(" in src[src.index("def shard_stripes"):]


def test_set_self_similarity_keeps_the_setting_and_refuses_a_malformed_one():
    from artstyletransfer_amd.neural_style_transfer import NeuralStyleTransfer
    nst = NeuralStyleTransfer(torch.device("cpu"), "vgg19", [np.zeros((16, 16, 3), np.float32)], "lbfgs")
    nst.set_self_similarity(2.0, 256, 1e-4, [0])
    assert nst._NeuralStyleTransfer__selfsim == (2.0, 256, 1e-4, [0])
    nst.set_self_similarity(0)
    assert nst._NeuralStyleTransfer__selfsim is None
    nst.set_self_similarity()
    assert nst._NeuralStyleTransfer__selfsim is None
    for bad in (dict(weights=-1.0), dict(weights=1.0, samples=5000), dict(weights=1.0, epsilon=0.0), dict(weights=1.0, levels=[])):
        with pytest.raises(ValueError, match="selfsim_"):
            nst.set_self_similarity(**bad)
    assert [p.default for p in list(inspect.signature(nst.set_self_similarity).parameters.values())] == [None, 1024, 1e-5, None]


def test_symbols_are_declared_in_the_header_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nst_hip.h")).read()
    names = ("nst_level_set_selfsim", "nst_level_selfsim", "nst_job_selfsim_losses", "nst_level_selfsim_decisions", "nst_selfsim_matrix",
             "nst_selfsim_term")
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    src = open(os.path.join(root, "artstyletransfer_amd", "csrc", "nst_kernels.h")).read()
    assert "constexpr int NST_MAP_TERMS = 4;" in src
    assert "#define NST_LOSS_ROW 4" in header or "NST_LOSS_ROW" in header
    # the hot path is HIP: the kernels exist under their names
    hip = open(os.path.join(root, "artstyletransfer_amd", "csrc", "selfsim.hip")).read()
    for kernel in ("selfsim_matrix_kernel", "selfsim_colsum_kernel", "selfsim_value_kernel", "selfsim_w_kernel", "selfsim_grad_kernel"):
        assert "void " + kernel in hip, kernel
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16" in hip and "__builtin_amdgcn_mfma_f32_32x32x2f32" in hip
    assert "atomic" not in re.sub(r"//.*", "", hip)
