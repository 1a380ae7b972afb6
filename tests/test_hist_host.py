"""CPU: the histogram loss (nst_level_set_histograms; Risser, Wilmot & Barnes 2017) - the numpy restatement the kernels are held
to (tests/hist_ref.py) against the properties the definition promises, the normaliser hist_modes.py, the job function
histogram_loss.neural_style_transfer_hist and the bindings."""
import asyncio
import inspect
import os
import re

import numpy as np
import pytest

import hist_ref
from artstyletransfer_amd import _lib, hist_modes as hist

Z = 0.0
U = 2.0 ** -24
ALL_BINS = (2, 4, 16, 256, 1024)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _maps(kind, n, ns, c=6, seed=0):
    g = np.random.default_rng(seed)
    if kind == "relu":           # half exact zeros
        f, fs = np.maximum(g.standard_normal((n, c)) * 3.0, 0.0), np.maximum(g.standard_normal((ns, c)) * 2.0 + 0.3, 0.0)
    else:                        # signed
        f, fs = g.standard_normal((n, c)) * 2.0 - 0.5, g.standard_normal((ns, c)) * 0.7 + 1.0
    f, fs = f.astype(np.float32), fs.astype(np.float32)
    f[:, 1] = np.float32(0.25)                       # a flat image channel
    fs[:, 2] = np.float32(-1.5)                      # a flat style channel
    fs[:, 4] = np.where(np.arange(ns) % 2 == 0, np.float32(0.0), np.float32(4.0))       # a gap: every middle bin empty
    return f, fs


@pytest.mark.parametrize("kind", ["relu", "signed"])
@pytest.mark.parametrize("bins", ALL_BINS)
def test_a_map_remapped_onto_its_own_histogram_comes_back(kind, bins):
    """With its own record as the style's, every non-empty bin b finds j = b with t = 0 for its start and t = 1 for its end:
    start_b = fl(lo + b width), end_b = fl(lo + (b + 1) width), width = (hi - lo) / B.  x = fl(fl(v - lo) scale) carries two
    roundings and scale = fl(B / (hi - lo)) a third, so lo + x width is within 3 u (hi - lo) of v, u = 2^-24; x - b is exact;
    the two ends are rounded to fp32 (together at most u M in the interpolation, M = max(|lo|, |hi|)).  |R - v| <=
    u (3 (hi - lo) + M), per channel; the device's three more roundings add u (hi - lo + M): tests/test_hip_hist.py uses
    u (4 (hi - lo) + 2 M)."""
    f, _ = _maps(kind, 700, 300, seed=bins)
    lo_hi, counts, _, _, ends = hist_ref.full(f, f, bins)
    r, flat, _ = hist_ref.remap(f, lo_hi, ends, bins)
    assert flat.tolist() == [False, True, False, False, False, False]
    lh = lo_hi.astype(np.float64)
    bound = U * (3.0 * (lh[:, 1] - lh[:, 0]) + np.abs(lh).max(axis=1))
    err = np.abs(r - f.astype(np.float64))
    assert (err <= bound[None, :]).all(), float((err / np.maximum(bound[None, :], 1e-300)).max())
    assert hist_ref.term(f, lo_hi, ends, bins)[0] <= float(bound.max()) ** 2


@pytest.mark.parametrize("kind", ["relu", "signed"])
@pytest.mark.parametrize("bins", ALL_BINS)
def test_the_remap_is_monotone_and_stays_inside_the_styles_range(kind, bins):
    f, fs = _maps(kind, 700, 300, seed=bins + 1)
    lo_hi, counts, s_lo_hi, s_counts, ends = hist_ref.full(f, fs, bins)
    r, flat, _ = hist_ref.remap(f, lo_hi, ends, bins)
    # the table itself: start_b <= end_b <= start_b' for the next non-empty b', all inside [slo, shi] (exactly: the ends are
    # roundings of numbers inside the range, whose bounds are fp32 numbers)
    for c in range(f.shape[1]):
        live = np.nonzero(counts[c])[0]
        if flat[c]:
            assert live.size == 0 and not ends[c].any()
            continue
        e = ends[c, live].astype(np.float64).reshape(-1)
        assert (np.diff(e) >= 0).all(), (c, bins)
        assert e.min() >= s_lo_hi[c, 0] and e.max() <= s_lo_hi[c, 1], (c, bins)
        assert e[0] == s_lo_hi[c, 0] and e[-1] == s_lo_hi[c, 1]           # the extremes of the image land on the style's
    order = np.argsort(f, axis=0, kind="stable")
    rs = np.take_along_axis(r, order, axis=0)[:, ~flat]
    assert (np.diff(rs, axis=0) >= 0).all()
    # a flat style channel: start = end = slo, whatever the image does; a flat image channel: no term
    assert (r[:, 2] == -1.5).all()
    assert (r[:, 1] == f[:, 1]).all()
    value, grad = hist_ref.term(f, lo_hi, ends, bins)
    assert not grad[:, 1].any() and value > 0
    # the gap: nothing is remapped into the inside of the style's empty stretch further than one image bin's share of it
    inside = (r[:, 4] > 4.0 / bins + 1e-6) & (r[:, 4] < 4.0 - 4.0 / bins - 1e-6)
    assert inside.sum() <= counts[4].max()


def test_two_ends_per_bin_where_one_knot_fails():
    """The case the definition's two ends are for: an image channel whose mass sits in the first and the last bin, against a
    style with the same shape.  The last bin follows empty bins: its start must be the style's upper cluster, not the lower
    end of the flat piece of the inverse CDF."""
    f = np.zeros((100, 1), np.float32)
    f[50:, 0] = np.linspace(9.0, 10.0, 50, dtype=np.float32)
    lo_hi, counts, _, _, ends = hist_ref.full(f, f, 16)
    live = np.nonzero(counts[0])[0]
    assert live[0] == 0 and live[-1] == 15
    assert ends[0, 15, 0] == np.float32(10.0 * 15 / 16) and ends[0, 15, 1] == np.float32(10.0)
    r, _, _ = hist_ref.remap(f, lo_hi, ends, 16)
    assert np.abs(r - f).max() <= U * 40.0


@pytest.mark.parametrize("bins", [2, 16, 256, 1024])
def test_values_on_bin_edges_and_the_maximum(bins):
    """A power-of-two range makes the edges exact: v = lo + k (hi - lo) / B lands in bin k with f = 0, the maximum in bin
    B - 1 with f = 1 (x = B is clamped), and a value one ulp below an edge in the bin before it.  (The range is [1, 5]: v - lo
    is then exact for every fp32 v of the range, the values one ulp below an edge included.)"""
    lo, hi = np.float32(1.0), np.float32(5.0)
    k = np.arange(bins + 1)
    v = (lo + k * (4.0 / bins)).astype(np.float32)
    below = np.nextafter(v[1:], np.float32(-np.inf)).astype(np.float32)
    f = np.concatenate([v, below])[:, None]
    b, fr, flat = hist_ref.bins_of(f, np.array([lo]), np.array([hi]), bins)
    assert not flat[0]
    assert (b[:bins, 0] == k[:bins]).all() and not fr[:bins, 0].any()
    assert b[bins, 0] == bins - 1 and fr[bins, 0] == 1.0
    assert (b[bins + 1:, 0] == k[:bins]).all() and (fr[bins + 1:, 0] < 1.0).all() and (fr[bins + 1:, 0] > 0.99).all()
    lo_hi, counts = hist_ref.range_counts(f, bins)
    assert lo_hi.tolist() == [[1.0, 5.0]] and counts.sum() == f.shape[0]
    assert counts[0, bins - 1] == 3 and (counts[0, :bins - 1] == 2).all()


def test_flat_channels_and_negative_zero():
    f = np.array([[0.0, 1.0, -0.0], [-0.0, 1.0, 3.0]], np.float32)
    lo_hi, counts = hist_ref.range_counts(f, 4)
    assert not np.signbit(lo_hi).any()                                   # -0 counts as +0
    assert not counts[0].any() and not counts[1].any() and counts[2].tolist() == [1, 0, 0, 1]
    ends = hist_ref.tables(counts, 2, lo_hi, counts, 2, 4)
    assert not ends[:2].any()
    value, grad = hist_ref.term(f, lo_hi, ends, 4)
    assert not grad[:, :2].any()


# ---- the normaliser ----------------------------------------------------------------------------------------------------------
def test_normalize_every_form():
    assert hist.normalize_hist(None) is None and hist.normalize_hist(0) is None and hist.normalize_hist(0.0) is None
    assert hist.normalize_hist([0] * 6) is None and hist.normalize_hist({}) is None
    assert hist.normalize_hist(2.0) == ((2.0, Z, Z, 2.0, Z, Z), 256, None)                   # relu1_1 and relu4_1
    assert hist.normalize_hist(2.0, style_indices=[0, 1, 2]) == ((2.0, Z, Z, Z, Z, Z), 256, None)
    assert hist.normalize_hist(2.0, style_indices=[1, 3]) == ((Z, Z, Z, 2.0, Z, Z), 256, None)
    assert hist.normalize_hist([1, 0, 0, 0, 0, 3], 16) == ((1.0, Z, Z, Z, Z, 3.0), 16, None)
    assert hist.normalize_hist({0: 1, "relu4_1": 5}, 1024, [1, 0, 1]) == ((1.0, Z, Z, 5.0, Z, Z), 1024, (0, 1))
    assert hist.normalize_hist({"conv5_1": 2.0}, use_relu=False)[0] == (Z, Z, Z, Z, Z, 2.0)
    assert hist.normalize_hist(np.float32(2.0), np.int64(2))[1] == 2
    assert hist.DEFAULT_BINS == 256 and hist.RISSER_MAPS == (0, 3)


def test_normalize_every_refusal():
    for bad in (-1.0, float("nan"), float("inf"), True, "1", b"1", {1, 2}, [1.0] * 5, [1.0] * 7, [0, 0, -1, 0, 0, 0], {7: 1.0},
                {"relu9_9": 1.0}, {0: -1.0}, {0: "x"}, object()):
        with pytest.raises(ValueError, match="hist_weight"):
            hist.normalize_hist(bad)
    for bad in (1, 0, -3, 1025, 2.0, True, "256", None):
        with pytest.raises(ValueError, match="hist_bins"):
            hist.normalize_hist(1.0, bad)
        with pytest.raises(ValueError, match="hist_bins"):
            hist.normalize_hist(None, bad)                               # the off setting is validated too
    for bad in ([], 1, "01", {0: 1}, [0.5], [-1], [8], [True]):
        with pytest.raises(ValueError, match="hist_levels"):
            hist.normalize_hist(1.0, 256, bad)
    with pytest.raises(ValueError, match="hist_levels"):
        hist.normalize_hist(1.0, 256, [2], levels_num=2)
    with pytest.raises(ValueError, match="not a style map"):
        hist.normalize_hist({4: 1.0}, style_indices=[0, 1, 2, 3, 5])
    with pytest.raises(ValueError, match="neither relu1_1 nor relu4_1"):
        hist.normalize_hist(1.0, style_indices=[1, 2, 5])
    with pytest.raises(ValueError, match="hist_weight"):
        hist.normalize_hist({"conv5_1": 2.0}, use_relu=True)             # the other flavour's name
    on = hist.normalize_hist(1.0)
    hist.check_exclusive(None, regions=object(), stripes=True, extra_styles=[1])
    hist.check_exclusive(on)
    hist.check_exclusive(on, extra_styles=[])
    for kw, text in ((dict(extra_styles=[1]), "extra_styles"), (dict(regions=object()), "content_regions"), (dict(stripes=True), "stripe sharding")):
        with pytest.raises(ValueError, match=text):
            hist.check_exclusive(on, **kw)


def test_module_is_free_of_torch():
    src = open(hist.__file__).read()
    assert "torch" not in re.sub(r'""".*?"""', "", src, flags=re.S)


# ---- the job function -------------------------------------------------------------------------------------------------------
def test_signature_is_the_semantic_mrf_jobs_plus_three_keywords():
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf_semantic
    base = list(inspect.signature(neural_style_transfer_mrf_semantic).parameters.values())
    ours = list(inspect.signature(neural_style_transfer_hist).parameters.values())
    assert [(p.name, p.kind, p.default) for p in ours[:len(base)]] == [(p.name, p.kind, p.default) for p in base]
    extra = ours[len(base):]
    assert [(p.name, p.default) for p in extra] == [("hist_weight", None), ("hist_bins", 256), ("hist_levels", None)]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in extra)
    assert inspect.isasyncgenfunction(neural_style_transfer_hist)


ARGS = (None, 1e3, 4e5, 1e2, "adam", "vgg19", "random", 1, 2, 0.0, (), (), (), ())


def _collect(gen):
    async def run():
        return [item async for item in gen]
    return asyncio.run(run())


def test_off_delegates_and_on_goes_through_transfer_from(monkeypatch):
    from artstyletransfer_amd import neural_style_transfer as impl, patch_match
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist
    calls = []

    async def fake_semantic(*a, **kw):
        calls.append(("semantic", a, kw))
        yield 100, "plain image"

    def fake_from(*a, **kw):
        calls.append(("from", a, kw))

        async def gen():
            yield 100, "hist image"
        return gen()

    monkeypatch.setattr(patch_match, "neural_style_transfer_mrf_semantic", fake_semantic)
    monkeypatch.setattr(impl, "_transfer_from", fake_from)
    for off in (None, 0, 0.0, [0] * 6, {}):
        calls.clear()
        out = _collect(neural_style_transfer_hist(*ARGS, "dev", pooling="avg", mrf_weight=2.0, semantic_weight=0.5, hist_weight=off, hist_bins=16))
        assert out == [(100, "plain image")]
        (kind, a, kw), = calls
        assert kind == "semantic" and a == ARGS + ("dev",) and kw["pooling"] == "avg" and kw["mrf_weight"] == 2.0
        assert kw["semantic_weight"] == 0.5 and not any(k.startswith("hist_") for k in kw)
    calls.clear()
    out = _collect(neural_style_transfer_hist(*ARGS, "dev", moment_weight=3.0, hist_weight={3: 2.0}, hist_bins=64, hist_levels=[1]))
    assert out == [(100, "hist image")]
    (kind, a, kw), = calls
    assert kind == "from" and a == ARGS and kw["device"] == "dev" and kw["start"] is None and kw["moment_weight"] == 3.0
    assert kw["histograms"] == ({3: 2.0}, 64, [1]) and kw["patches"] is None and kw["semantics"] is None
    # beside the MRF term and its semantic maps
    calls.clear()
    sem = np.zeros((8, 8), np.int64)
    _collect(neural_style_transfer_hist(*ARGS, mrf_weight=1.0, mrf_stride=2, semantic_content=sem, semantic_style=sem, hist_weight=1.0))
    (kind, a, kw), = calls
    assert kw["patches"] == (1.0, 2, 1e-5, None) and kw["semantics"][0] is sem and kw["semantics"][2] == 1.0
    assert kw["histograms"] == (1.0, 256, None)
    # a malformed setting never reaches either
    calls.clear()
    for bad in (dict(hist_weight=-1.0), dict(hist_weight=1.0, hist_bins=1), dict(hist_weight=None, hist_bins=2000),
                dict(hist_weight=1.0, hist_levels=[])):
        with pytest.raises(ValueError, match="hist_"):
            _collect(neural_style_transfer_hist(*ARGS, **bad))
    with pytest.raises(ValueError, match="mrf_weight is off"):
        _collect(neural_style_transfer_hist(*ARGS, semantic_content=sem, semantic_style=sem, hist_weight=1.0))
    assert calls == []


def _pair(h=64, w=96, hs=70, ws=110):
    from artstyletransfer_amd import neural_style_transfer as impl
    return impl.ContentStylePair(("c", np.zeros((h, w, 3), np.float32)), ("s", np.zeros((hs, ws, 3), np.float32)))


def test_refusals_before_any_gpu_work(monkeypatch):
    """With the job's style set: everything is refused in _transfer_from, before _transfer is even created."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist

    def reached(*a, **kw):
        raise AssertionError("the job was started")

    monkeypatch.setattr(impl, "_transfer", reached)
    monkeypatch.setattr(impl, "shared_engine", reached)
    args = (_pair(),) + ARGS[1:]
    cases = [
        (dict(hist_weight=1.0, extra_styles=[np.zeros((32, 32, 3), np.float32)]), "extra_styles"),
        (dict(hist_weight=1.0, content_regions=np.zeros((64, 96), np.int64), style_regions=np.zeros((70, 110), np.int64)), "content_regions"),
        (dict(hist_weight={4: 1.0}), "not a style map"),
        (dict(hist_weight=1.0, style_layers=[1, 2, 5]), "neither relu1_1 nor relu4_1"),
        (dict(hist_weight=1.0, hist_levels=[2]), "hist_levels"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            _collect(neural_style_transfer_hist(*args, **kw))


def test_set_histogram_loss_reaches_the_device_job_after_the_mrf_hooks(monkeypatch):
    """NeuralStyleTransfer.set_histogram_loss is data of the next process: handed to the device job once it exists, after
    set_patch_match and set_patch_semantics, with the checked weights; a job without it never calls the hook."""
    import torch
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class FakeJob:
        def __init__(self, *a, **kw):
            seen.append(("made", sorted(kw)))

        def set_patch_match(self, *a):
            seen.append(("patches", a))

        def set_patch_semantics(self, planes, weight):
            seen.append(("semantics", weight))

        def set_histogram_loss(self, *a):
            seen.append(("histograms", a))

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
    nst.set_histogram_loss(2.0, bins=64, levels=[1])
    assert run(nst) == []
    assert seen == [("made", []), ("histograms", ((2.0, Z, Z, 2.0, Z, Z), 64, (1,))), ("closed",)]
    seen.clear()
    nst.set_patch_match({2: 1.0}, levels=[0])
    nst.set_patch_semantics(np.zeros((64, 96), np.int64), np.zeros((70, 110), np.int64), 0.5)
    assert run(nst) == []
    assert [s[0] for s in seen] == ["made", "patches", "semantics", "histograms", "closed"]
    seen.clear()
    nst.set_patch_match(None)
    nst.set_patch_semantics(None, None)
    nst.set_histogram_loss(None)
    assert run(nst) == [] and seen == [("made", []), ("closed",)]
    # refusals of process(), where the style set is known: before the job exists
    seen.clear()
    nst.set_histogram_loss({4: 1.0})
    with pytest.raises(ValueError, match="not a style map"):
        run(nst)
    nst.set_histogram_loss(1.0)
    nst.set_feature_maps(4, [1, 2, 5])
    with pytest.raises(ValueError, match="neither relu1_1 nor relu4_1"):
        run(nst)
    assert seen == []
    with pytest.raises(ValueError, match="hist_bins"):
        nst.set_histogram_loss(1.0, bins=1)


def test_device_job_hook_gives_each_level_its_style_image():
    """_DeviceJob.set_histogram_loss: the levels named (None: all), each with the style level image its targets were made
    from, as set_patch_match does."""
    import contextlib
    import torch
    from artstyletransfer_amd import neural_style_transfer as impl
    seen = []

    class Engine:
        def set_histograms(self, level, style, weights, bins):
            seen.append((level, style, weights, bins))

    job = object.__new__(impl._DeviceJob)
    job.engine, job.dev, job.job_stream = Engine(), None, None
    job.style_levels = [lambda: "s0", lambda: "s1", lambda: "s2"]
    null = lambda *a, **kw: contextlib.nullcontext()                   # noqa: E731
    orig = torch.cuda.device, torch.cuda.stream
    torch.cuda.device, torch.cuda.stream = null, null
    try:
        job.set_histogram_loss((1.0,) * 6, 16, (0, 2))
        job.set_histogram_loss((2.0,) * 6, 32, None)
    finally:
        torch.cuda.device, torch.cuda.stream = orig
    assert seen == [(0, "s0", (1.0,) * 6, 16), (2, "s2", (1.0,) * 6, 16)] + [(i, f"s{i}", (2.0,) * 6, 32) for i in range(3)]


# ---- the bindings -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_in_the_header_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nst_hip.h")).read()
    for name, nargs in (("nst_level_set_histograms", 8), ("nst_level_histograms", 4), ("nst_job_histogram_losses", 3),
                        ("nst_level_histogram_tables", 7), ("nst_level_histogram_style", 6), ("nst_histogram_counts", 8),
                        ("nst_histogram_tables", 11), ("nst_histogram_term", 11)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
    lib_path = os.path.join(root, "artstyletransfer_amd", "libnst_hip.so")
    if os.path.exists(lib_path):                     # (the built library exports them: no GPU needed to look)
        import ctypes
        lib = ctypes.CDLL(lib_path)
        for name in _lib.SYMBOLS:
            if "histogram" in name:
                assert hasattr(lib, name), name
    from artstyletransfer_amd.engine import StyleEngine
    for method in ("set_histograms", "clear_histograms", "histograms_setting", "histogram_losses", "histogram_tables", "histogram_style",
                   "histogram_counts", "histogram_table", "histogram_term"):
        assert callable(getattr(StyleEngine, method)), method


def test_job_settings_tables_are_untouched():
    """The term is data of a job: no SETTINGS row, no keyword of neural_style_transfer()."""
    from artstyletransfer_amd import job_settings
    from artstyletransfer_amd.neural_style_transfer import neural_style_transfer
    assert not any("hist_" in str(row).lower() for row in job_settings.SETTINGS)
    assert not any(p.startswith("hist") for p in inspect.signature(neural_style_transfer).parameters)
