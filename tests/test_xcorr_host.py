"""CPU: the long-range style term, xcorr (nst_level_set_xcorr) - the reference of tests/xcorr_ref.py against a literal triple
loop, its flip symmetry, fp64 autograd against the header's closed-form gradient, the Python setting parser (xcorr_modes) with
every refusal, and the job function's plumbing.  No GPU."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest
import torch

import xcorr_ref
from artstyletransfer_amd import _lib, xcorr_modes as xcorr

Z = 0.0


def _map(c, h, w, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn((1, c, h, w), generator=g, dtype=dtype) + 0.3)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_vs_a_literal_triple_loop():
    """A 3 x 4 x 2 map (h x w x C), every shift it admits: G_d[c][e] = (1/Z_d) sum_{y < h-dy, x < w-dx} F(y+dy, x+dx)[c] F(y, x)[e],
    Z_d = C (h-dy)(w-dx), written out."""
    h, w, c = 3, 4, 2
    f = _map(c, h, w, 3)
    for dy in range(h):
        for dx in range(w):
            if (dx, dy) == (0, 0):
                continue
            want = torch.zeros((c, c), dtype=torch.float64)
            for y in range(h - dy):
                for x in range(w - dx):
                    for a in range(c):
                        for b in range(c):
                            want[a, b] += f[0, a, y + dy, x + dx] * f[0, b, y, x]
            want /= c * (h - dy) * (w - dx)
            got = xcorr_ref.matrix(f, (dx, dy))
            assert torch.allclose(got, want, rtol=1e-14, atol=0), (dx, dy)
    # the value: the mean over the shifts of the mean squared difference
    shifts = ((1, 0), (0, 2), (3, 1))
    gt = xcorr_ref.matrices(_map(c, 5, 6, 4), shifts)
    want = sum(float(((xcorr_ref.matrix(f, d) - gt[k]) ** 2).sum()) / (c * c) for k, d in enumerate(shifts)) / 3
    assert float(xcorr_ref.value(f, gt, shifts)) == pytest.approx(want, rel=1e-14)
    for bad in ((0, 0), (4, 0), (0, 3)):
        with pytest.raises(AssertionError):
            xcorr_ref.matrix(f, bad)


@pytest.mark.parametrize("shape", [(3, 5, 7), (8, 4, 4), (2, 1, 9)])
def test_a_map_flipped_in_x_and_y_gives_the_transpose(shape):
    """p -> p + d on the flipped map is p' + d -> p' on the original: G_d(flip F) = G_d(F)^T."""
    c, h, w = shape
    f = _map(c, h, w, 5)
    for dx, dy in ((1, 0), (0, h - 1), (w - 1, 0), (min(2, w - 1), min(1, h - 1))):
        if (dx, dy) == (0, 0):
            continue
        a = xcorr_ref.matrix(torch.flip(f, dims=(2, 3)), (dx, dy))
        b = xcorr_ref.matrix(f, (dx, dy))
        assert torch.allclose(a, b.t(), rtol=1e-13, atol=1e-300), (dx, dy)
        assert not torch.allclose(b, b.t(), rtol=1e-6)          # (the statistic is not symmetric: the check is not vacuous)


@pytest.mark.parametrize("shape,shifts", [((4, 5, 6), ((1, 0), (0, 2), (3, 1))), ((16, 7, 3), ((2, 0), (0, 6), (1, 1))),
                                          ((2, 3, 4), ((3, 0), (0, 2), (3, 2), (1, 0), (0, 1))), ((8, 1, 9), ((4, 0), (8, 0)))])
def test_autograd_vs_the_closed_form_gradient(shape, shifts):
    """fp64 autograd of weight x value against S_d = (2 w / (|D| C^2 Z_d)) (G_d - Gt_d),
    dF(q) = sum_d ([x >= dx, y >= dy] F(q - d) S_d^T + [x < w-dx, y < h-dy] F(q + d) S_d)."""
    c, h, w = shape
    f = _map(c, h, w, 7)
    gt = xcorr_ref.matrices(_map(c, h + 2, w + 1, 8), shifts)
    weight = 3.5
    x = f.clone().requires_grad_(True)
    (weight * xcorr_ref.value(x, gt, shifts)).backward()
    want = xcorr_ref.gradient(f, gt, shifts, weight)
    assert float(x.grad.abs().max()) > 0
    assert torch.allclose(x.grad, want, rtol=1e-12, atol=1e-18)
    # at the style itself value and gradient vanish
    own = xcorr_ref.matrices(f, shifts)
    assert float(xcorr_ref.value(f, own, shifts)) == 0.0 and not xcorr_ref.gradient(f, own, shifts).any()


def test_border_pixels_take_one_term_only():
    """A map with one nonzero pixel q0: dF is nonzero only at q0 - d (from the F(q + d) part) and q0 + d (from F(q - d)), where
    those lie in the map."""
    c, h, w = 3, 4, 6
    gt = xcorr_ref.matrices(_map(c, h, w, 9), ((2, 0),))
    for x0, want in ((0, {2}), (1, {3}), (2, {0, 4}), (4, {2}), (5, {3})):
        f = torch.zeros((1, c, h, w), dtype=torch.float64)
        f[0, :, 1, x0] = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
        g = xcorr_ref.gradient(f, gt, ((2, 0),))
        cols = {int(x) for x in torch.nonzero(g[0].abs().sum(dim=(0, 1)))[:, 0]}
        rows = {int(y) for y in torch.nonzero(g[0].abs().sum(dim=(0, 2)))[:, 0]}
        assert cols == want and rows == {1}, (x0, cols, rows)


# ---- the normaliser -------------------------------------------------------------------------------------------------------
def test_normalize_every_form():
    assert xcorr.DEFAULT_SHIFTS == (2, 4, 8) and xcorr.MAX_SHIFT == 64 and xcorr.MAX_SHIFTS == 16
    assert xcorr.normalize_shifts() == ((2, 0), (0, 2), (4, 0), (0, 4), (8, 0), (0, 8))
    assert xcorr.normalize_shifts(3) == ((3, 0), (0, 3))
    assert xcorr.normalize_shifts([(1, 2), 5, [0, 64], (64, 0)]) == ((1, 2), (5, 0), (0, 5), (0, 64), (64, 0))
    assert xcorr.normalize_shifts(np.array([1, 2])) == ((1, 0), (0, 1), (2, 0), (0, 2))
    assert len(xcorr.normalize_shifts(range(1, 9))) == 16
    for off in (None, 0, 0.0, [0] * 6, {}):
        assert xcorr.normalize_xcorr(off) is None
    assert xcorr.normalize_xcorr(2.0) == ((Z, 2.0, 2.0, 2.0, Z, Z), xcorr.normalize_shifts(), None)
    assert xcorr.normalize_xcorr(2.0, style_indices=[0, 2, 5])[0] == (Z, Z, 2.0, Z, Z, Z)
    assert xcorr.normalize_xcorr({"relu1_1": 1.0, 3: 4.0}, [(1, 1)], [1, 0, 1]) == ((1.0, Z, Z, 4.0, Z, Z), ((1, 1),), (0, 1))
    assert xcorr.normalize_xcorr([0, 0, 1, 0, 0, 0], 7)[0] == (Z, Z, 1.0, Z, Z, Z)


def test_normalize_every_refusal():
    for bad in ((), [], None, "2", {2: 1}, {2}, 2.0, True, [2.5], [-1], [65], [(1,)], [(1, 2, 3)], [(1, 65)], [(-1, 0)], [(1.0, 0)], [(0, 0)],
                [0], [2, (2, 0)], [(3, 1), (3, 1)], list(range(1, 10)), ["ab"], [None], [True]):
        with pytest.raises(ValueError, match="xcorr_shifts"):
            xcorr.normalize_shifts(bad)
    # the off setting is validated too
    with pytest.raises(ValueError, match="xcorr_shifts"):
        xcorr.normalize_xcorr(None, [0])
    for bad in (-1.0, float("nan"), float("inf"), "1", [1.0] * 5, {7: 1.0}, {"relu9_9": 1.0}, True):
        with pytest.raises(ValueError, match="xcorr_weight"):
            xcorr.normalize_xcorr(bad)
    for bad in ([], [8], [-1], 1, "0", [True]):
        with pytest.raises(ValueError, match="xcorr_levels"):
            xcorr.normalize_xcorr(1.0, xcorr_levels=bad)
    with pytest.raises(ValueError, match="xcorr_levels"):
        xcorr.normalize_xcorr(1.0, xcorr_levels=[2], levels_num=2)
    # a positive weight on a map that is not a style map; a bare number with none of its maps among them
    with pytest.raises(ValueError, match="map 4 has a positive weight but is not a style map"):
        xcorr.normalize_xcorr({4: 1.0}, style_indices=[0, 1, 2, 3, 5])
    with pytest.raises(ValueError, match="none of relu2_1, relu3_1, relu4_1"):
        xcorr.normalize_xcorr(1.0, style_indices=[0, 5])
    on = xcorr.normalize_xcorr(1.0)
    for kw in (dict(extra_styles=[object()]), dict(regions=object()), dict(stripes=True)):
        with pytest.raises(ValueError, match="xcorr_weight cannot be combined"):
            xcorr.check_exclusive(on, **kw)
        xcorr.check_exclusive(None, **kw)


def test_a_shift_must_be_smaller_than_every_weighted_map_of_a_carrying_level():
    st = xcorr.normalize_xcorr({1: 1.0, 3: 1.0}, [8])
    # relu4_1 of a 64x96 level is 8x12: dy = 8 does not fit; of its 32x48 level 4x6
    with pytest.raises(ValueError, match=r"the shift \(0, 8\) is not smaller than the map 3 of the image of level 0 \(8x12\)"):
        xcorr.level_carries(st, [(64, 96)], [(128, 128)])
    with pytest.raises(ValueError, match=r"style image of level 0 \(8x16\)"):
        xcorr.level_carries(st, [(128, 128)], [(64, 128)])
    assert xcorr.level_carries(st, [(160, 144)], [(128, 160)]) == [True]
    # a level outside xcorr_levels is not checked, and does not carry the term
    st0 = xcorr.normalize_xcorr({1: 1.0, 3: 1.0}, [8], [0])
    assert xcorr.level_carries(st0, [(128, 128), (64, 64)], [(128, 160), (16, 16)]) == [True, False]
    with pytest.raises(ValueError, match="not smaller"):
        xcorr.level_carries(xcorr.normalize_xcorr({1: 1.0, 3: 1.0}, [8]), [(128, 128), (64, 64)], [(128, 160), (64, 80)])
    with pytest.raises(ValueError, match="xcorr_levels: level 3 is outside"):
        xcorr.level_carries(xcorr.normalize_xcorr(1.0, xcorr_levels=[3]), [(64, 64)], [(64, 64)])
    assert xcorr.level_carries(None, [(64, 64)], [(64, 64)]) == [False]
    xcorr.check_map(9, 9, ((8, 0), (0, 8)))
    with pytest.raises(ValueError, match="not smaller"):
        xcorr.check_map(9, 8, ((8, 0),))


def test_module_is_free_of_torch():
    src = open(xcorr.__file__).read()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)


# ---- the job function -------------------------------------------------------------------------------------------------------
def test_signature_is_the_selfsim_jobs_plus_three_keywords():
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim
    from artstyletransfer_amd.xcorr_loss import neural_style_transfer_xcorr
    base = list(inspect.signature(neural_style_transfer_selfsim).parameters.values())
    ours = list(inspect.signature(neural_style_transfer_xcorr).parameters.values())
    assert [(p.name, p.kind, p.default) for p in ours[:len(base)]] == [(p.name, p.kind, p.default) for p in base]
    extra = ours[len(base):]
    assert [(p.name, p.default) for p in extra] == [("xcorr_weight", None), ("xcorr_shifts", (2, 4, 8)), ("xcorr_levels", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in extra)
    assert inspect.isasyncgenfunction(neural_style_transfer_xcorr)
    assert [p.name for p in base][-4:] == ["selfsim_weight", "selfsim_samples", "selfsim_epsilon", "selfsim_levels"]
    from artstyletransfer_amd.config import Config
    assert not any("xcorr" in name for name in vars(Config()))          # (data of one job: no Config field)


ARGS = (None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 2, 0.0, (), (), (), ())


def _collect(gen):
    async def run():
        return [item async for item in gen]
    return asyncio.run(run())


def test_off_delegates_and_on_goes_through_transfer_from(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl, selfsim_loss
    from artstyletransfer_amd.xcorr_loss import neural_style_transfer_xcorr
    calls = []

    async def fake_selfsim(*a, **kw):
        calls.append(("selfsim", a, kw))
        yield 100, "plain image"

    def fake_from(*a, **kw):
        calls.append(("from", a, kw))

        async def gen():
            yield 100, "xcorr image"
        return gen()

    monkeypatch.setattr(selfsim_loss, "neural_style_transfer_selfsim", fake_selfsim)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    for off in (None, 0, 0.0, [0] * 6, {}):
        calls.clear()
        out = _collect(neural_style_transfer_xcorr(*ARGS, "dev", pooling="avg", mrf_weight=2.0, selfsim_weight=3.0, selfsim_samples=16,
                                                   xcorr_weight=off, xcorr_shifts=[3]))
        assert out == [(100, "plain image")]
        (kind, a, kw), = calls
        assert kind == "selfsim" and a == ARGS + ("dev",) and kw["pooling"] == "avg" and kw["mrf_weight"] == 2.0
        assert kw["selfsim_weight"] == 3.0 and kw["selfsim_samples"] == 16 and not any(k.startswith("xcorr_") for k in kw)
    calls.clear()
    out = _collect(neural_style_transfer_xcorr(*ARGS, "dev", moment_weight=3.0, xcorr_weight={3: 2.0}, xcorr_shifts=[(1, 1)], xcorr_levels=[1]))
    assert out == [(100, "xcorr image")]
    (kind, a, kw), = calls
    assert kind == "from" and a == ARGS and kw["device"] == "dev" and kw["start"] is None and kw["moment_weight"] == 3.0
    assert kw["xcorr"] == ({3: 2.0}, [(1, 1)], [1])
    assert all(kw[k] is None for k in ("patches", "semantics", "histograms", "remd", "selfsim"))
    # beside the other per-map terms
    calls.clear()
    _collect(neural_style_transfer_xcorr(*ARGS, mrf_weight=1.0, mrf_stride=2, hist_weight=1.0, remd_weight=2.0, selfsim_weight=1.0, xcorr_weight=1.0))
    (kind, a, kw), = calls
    assert kw["patches"] == (1.0, 2, 1e-5, None) and kw["histograms"] == (1.0, 256, None) and kw["remd"] == (2.0, 4096, 1e-5, None)
    assert kw["selfsim"] == (1.0, 1024, 1e-5, None) and kw["xcorr"] == (1.0, (2, 4, 8), None)
    # a malformed setting never reaches either
    calls.clear()
    for bad in (dict(xcorr_weight=-1.0), dict(xcorr_weight=1.0, xcorr_shifts=[]), dict(xcorr_weight=None, xcorr_shifts=[65]),
                dict(xcorr_weight=1.0, xcorr_shifts=[(0, 0)]), dict(xcorr_weight=1.0, xcorr_levels=[])):
        with pytest.raises(ValueError, match="xcorr_"):
            _collect(neural_style_transfer_xcorr(*ARGS, **bad))
    assert calls == []


def _pair(h=64, w=96, hs=70, ws=110):
    from artstyletransfer_amd import neural_style_transfer as impl
    return impl.ContentStylePair(("c", np.zeros((h, w, 3), np.float32)), ("s", np.zeros((hs, ws, 3), np.float32)))


def test_refusals_before_any_gpu_work(monkeypatch):
    """With the job's taps and sizes: everything is refused in _transfer_from, before _transfer is even created."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.xcorr_loss import neural_style_transfer_xcorr

    def reached(*a, **kw):
        raise AssertionError("the job was started")

    monkeypatch.setattr(impl, "_transfer", reached)
    monkeypatch.setattr(impl, "shared_engine", reached)
    args = (_pair(),) + ARGS[1:]
    cases = [
        (dict(xcorr_weight=1.0, extra_styles=[np.zeros((32, 32, 3), np.float32)]), "extra_styles"),
        (dict(xcorr_weight=1.0, content_regions=np.zeros((64, 96), np.int64), style_regions=np.zeros((70, 110), np.int64)), "content_regions"),
        (dict(xcorr_weight={4: 1.0}), "not a style map of the job"),
        (dict(xcorr_weight={2: 1.0}, style_layers=[0, 5]), "not a style map of the job"),
        (dict(xcorr_weight=1.0, style_layers=[0, 5]), "none of relu2_1, relu3_1, relu4_1"),
        (dict(xcorr_weight=1.0, xcorr_levels=[2]), "xcorr_levels"),
        (dict(xcorr_weight={5: 1.0}, xcorr_shifts=[64]), "not smaller than"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            _collect(neural_style_transfer_xcorr(*args, **kw))


def test_a_setting_that_fits_reaches_the_job(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.xcorr_loss import neural_style_transfer_xcorr
    seen = []

    def fake_transfer(*a, xcorr=None):
        seen.append(xcorr)

        async def gen():
            yield 100, "image"
        return gen()

    monkeypatch.setattr(impl, "_transfer", fake_transfer)
    args = (_pair(),) + ARGS[1:]
    for kw in (dict(xcorr_weight=1.0), dict(xcorr_weight={1: 1.0}, xcorr_shifts=[(64, 64)], xcorr_levels=[0]),
               dict(xcorr_weight={"relu5_1": 1.0}, xcorr_shifts=[1], gram_shift=-1.0, remd_weight=1.0)):
        assert _collect(neural_style_transfer_xcorr(*args, **kw)) == [(100, "image")]
    assert [s[0] for s in seen] == [1.0, {1: 1.0}, {"relu5_1": 1.0}]


def test_stripe_sharding_refuses_the_term():
    with pytest.raises(ValueError, match="xcorr_weight cannot be combined with stripe sharding"):
        xcorr.check_exclusive(((Z, 1.0, Z, Z, Z, Z), ((1, 0),), None), stripes=True)
    src = open(os.path.join(os.path.dirname(xcorr.__file__), "engine.py")).read()
    assert "_xcorr.check_exclusive(" in src[src.index("def shard_stripes"):]


def test_set_shifted_gram_keeps_the_setting_and_refuses_a_malformed_one():
    from artstyletransfer_amd.neural_style_transfer import NeuralStyleTransfer
    nst = NeuralStyleTransfer(torch.device("cpu"), "vgg19", [np.zeros((16, 16, 3), np.float32)], "lbfgs")
    nst.set_shifted_gram(2.0, [3, (1, 1)], [0])
    assert nst._NeuralStyleTransfer__xcorr == (2.0, [3, (1, 1)], [0])
    nst.set_shifted_gram(0)
    assert nst._NeuralStyleTransfer__xcorr is None
    nst.set_shifted_gram()
    assert nst._NeuralStyleTransfer__xcorr is None
    for bad in (dict(weights=-1.0), dict(weights=1.0, shifts=[65]), dict(weights=1.0, shifts=[]), dict(weights=1.0, levels=[])):
        with pytest.raises(ValueError, match="xcorr_"):
            nst.set_shifted_gram(**bad)
    assert [p.default for p in list(inspect.signature(nst.set_shifted_gram).parameters.values())] == [None, (2, 4, 8), None]


def test_symbols_are_declared_in_the_header_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nst_hip.h")).read()
    names = ("nst_level_set_xcorr", "nst_level_xcorr", "nst_job_xcorr_losses", "nst_level_xcorr_matrices", "nst_xcorr", "nst_xcorr_term")
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS, name
    assert "mean over the shifts, not the paper's sum" in re.sub(r"\s+\*?\s*", " ", header).replace("MEAN", "mean")
    src = open(os.path.join(root, "artstyletransfer_amd", "csrc", "nst_kernels.h")).read()
    assert "constexpr int XCORR_MAX_SHIFTS = 16;" in src and "launch_xcorr_rows" in src
    ctx = open(os.path.join(root, "artstyletransfer_amd", "csrc", "nst_ctx.h")).read()
    assert "T_XCORR = 4" in ctx and "struct XcorrLevel : MapTerm" in ctx
    assert "xcorr.hip" in open(os.path.join(root, "artstyletransfer_amd", "csrc", "Makefile")).read()
    # the hot path is HIP: the kernels exist under their names, on the matrix pipes the definition names, without atomics
    hip = open(os.path.join(root, "artstyletransfer_amd", "csrc", "xcorr.hip")).read()
    for kernel in ("xcorr_partial_kernel", "xcorr_finish_kernel", "xcorr_value_kernel", "xcorr_rows_kernel", "xcorr_grad_kernel"):
        assert "void " + kernel in hip, kernel
    assert "__builtin_amdgcn_mfma_f32_32x32x16_f16" in hip and "__builtin_amdgcn_mfma_f32_32x32x2f32" in hip
    assert "atomic" not in re.sub(r"//.*", "", hip)
