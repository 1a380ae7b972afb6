"""GPU: the self-similarity content term (nst_level_set_selfsim; the content half of Kolkin, Salavon & Shakhnarovich 2019) - the
column-normalised matrix of pairwise cosine distances between the sampled vectors of a map, held to the content's.
1. the distance matrix and its column sums alone (nst_selfsim_matrix) against fp64, held to torch-fp32's own error;
2. the signs of N - M against fp64; 3. value and gradient alone (nst_selfsim_term) against fp64 autograd of
   tests/selfsim_ref.py at the device's decisions; 4. image = content; 5. degenerate maps;
6. - 8. the closure under the device's decisions against a restated closure, over the paths the term's gradient takes;
9. bits; 10. refusals and the life cycle; 11. a whole job."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import selfsim_ref
from hip_helpers import (CW, SW, TVW, TERMS, check_rows, closure_vs_oracle_under_equal_decisions, dev, levels as _levels,
                         oracle_targets, rel_l2, report)
from oracle import cpu_ref
from test_hip_gram_shift import _bits, _job, prerelu_vgg19_features
from test_hip_mrf import nhwc

pytestmark = pytest.mark.gpu

EPS = 1e-5


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng_per_level(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, batched=False)
    yield e
    e.close()


def relu_noise(c, h, w, seed, base=None, scale=1.0):
    """ReLU of seeded normal noise, (1,C,h,w); with `base`: ReLU(base + scale noise)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((1, c, h, w), generator=g)
    return torch.relu(z if base is None else base + scale * z).contiguous()


# ---- 1. - 3. the pieces alone against fp64 -----------------------------------------------------------------------------------
# (C, h, w, stride, the image: "free" = independent of the content, "near" = the content plus 0.3 noise)
SHAPES = [(64, 12, 13, 1, "free"), (512, 5, 6, 1, "near"), (128, 9, 10, 2, "free"), (256, 7, 33, 1, "near"), (64, 40, 37, 1, "free"),
          (512, 33, 35, 1, "near"), (128, 70, 66, 2, "free"), (64, 3, 1, 1, "near"), (128, 4, 5, 8, "free")]
_CASES = {}


def _case(eng, shape):
    """Of one shape, computed once: the maps, fp64's and torch-fp32's (D, s, N - M), and the device's D, s, value, signs and
    gradient."""
    if shape not in _CASES:
        c, h, w, st, kind = shape
        fc = relu_noise(c, h, w, seed=c + h)
        f = relu_noise(c, h, w, seed=c + h + 100) if kind == "free" else relu_noise(c, h, w, seed=c + h + 100, base=fc, scale=0.3)
        ref = {}
        for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
            d, s, n_img = selfsim_ref.matrices(f.to(dt), st)
            m = selfsim_ref.normalised(selfsim_ref.distances(fc.to(dt), st))
            ref[name] = (d.double(), s.double(), (n_img - m).double())
        d_dev, s_dev = eng.selfsim_matrix(nhwc(f), st, EPS)
        val, sg, grad = eng.selfsim_term(nhwc(f), nhwc(fc), st, EPS, coef=1.0)
        _CASES[shape] = dict(f=f, fc=fc, ref=ref, D=d_dev.cpu(), s=s_dev.cpu(), val=float(val.cpu()[0]), sg=sg.cpu(),
                             grad=grad.cpu().permute(2, 0, 1).unsqueeze(0).double(), clamped=selfsim_ref.clamped(f.double(), st))
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_matrix_vs_fp64(eng, shape):
    """The max error of D and of s_j / n against fp64 is at most 4 x that of a torch-fp32 evaluation on the same input (measured
    here, never taken from the device); the diagonal is exactly 0; nothing is negative; no entry is clamped on these shapes,
    in fp64 or on the device."""
    c, h, w, st, kind = shape
    k = _case(eng, shape)
    d64, s64, _ = k["ref"]["fp64"]
    d32, s32, _ = k["ref"]["fp32"]
    n = selfsim_ref.counts(h, w, st)
    assert tuple(k["D"].shape) == (n, n) and tuple(k["s"].shape) == (n,) and k["D"].dtype == torch.float32 and k["s"].dtype == torch.float64
    e_d, e_d32 = float((k["D"].double() - d64).abs().max()), float((d32 - d64).abs().max())
    e_s, e_s32 = float((k["s"] - s64).abs().max()) / n, float((s32 - s64).abs().max()) / n
    report(f"selfsim matrix C={c} {h}x{w}/{st} [{kind}] n={n}: D err device {e_d:.2e} / torch fp32 {e_d32:.2e}; s/n err device {e_s:.2e} / "
           f"torch fp32 {e_s32:.2e}")
    assert not k["D"].diagonal().any()
    assert float(k["D"].min()) >= 0.0
    assert k["clamped"] == 0
    off = ~torch.eye(n, dtype=torch.bool)
    assert bool((k["D"][off] > 0).all())
    assert e_d <= 4.0 * e_d32, (e_d, e_d32)
    assert e_s <= 4.0 * e_s32, (e_s, e_s32)
    # s is the double sum of the device's own D, column by column
    np.testing.assert_allclose(k["s"].numpy(), k["D"].double().sum(dim=0).numpy(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("shape", SHAPES)
def test_decisions_vs_fp64(eng, shape):
    """Where the device's sign differs from fp64's, |N - M| in fp64 is at most 4 x torch-fp32's max error of N - M; at most 1e-4
    of the entries differ (a cap, not a measurement)."""
    c, h, w, st, kind = shape
    k = _case(eng, shape)
    _, _, nm64 = k["ref"]["fp64"]
    _, _, nm32 = k["ref"]["fp32"]
    delta = 4.0 * float((nm32 - nm64).abs().max())
    sg64 = torch.sign(nm64).to(torch.int8)
    differ = k["sg"] != sg64
    share = float(differ.double().mean())
    worst = float(nm64[differ].abs().max()) if bool(differ.any()) else 0.0
    share32 = float((torch.sign(nm32).to(torch.int8) != sg64).double().mean())
    report(f"selfsim signs C={c} {h}x{w}/{st} [{kind}]: {int(differ.sum())} of {differ.numel()} differ from fp64 (torch fp32: share "
           f"{share32:.1e}), worst |N - M| there {worst:.2e}, delta {delta:.2e}")
    assert k["sg"].dtype == torch.int8 and int(k["sg"].min()) >= -1 and int(k["sg"].max()) <= 1
    assert worst <= delta, (worst, delta)
    assert share <= 1e-4, share


@pytest.mark.parametrize("shape", SHAPES)
def test_term_vs_fp64_autograd_at_the_device_decisions(eng, shape):
    """Value and gradient at the device's decisions against fp64 autograd of the reference under the same signs: the value's
    error and the gradient's rel-L2 are at most 4 x those of a torch-fp32 evaluation of the same expression on the same input;
    the gradient is exactly zero off the sample grid; the value lies in [0, 2]."""
    c, h, w, st, kind = shape
    k = _case(eng, shape)
    live = (k["D"] != 0) | torch.eye(k["D"].shape[0], dtype=torch.bool)
    out = {}
    for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        x = k["f"].to(dt).clone().requires_grad_(True)
        v = selfsim_ref.value_under(x, k["fc"].to(dt), k["sg"], st, EPS, live)
        v.backward()
        out[name] = (float(v.detach()), x.grad.detach().double())
    v64, g64 = out["fp64"]
    v32, g32 = out["fp32"]
    e_v, e_v32 = abs(k["val"] - v64), abs(v32 - v64)
    n = selfsim_ref.counts(h, w, st)
    if n == 1:
        assert k["val"] == 0.0 and not k["grad"].any() and v64 == 0.0
        return
    e_g, e_g32 = rel_l2(k["grad"].numpy(), g64.numpy()), rel_l2(g32.numpy(), g64.numpy())
    report(f"selfsim term C={c} {h}x{w}/{st} [{kind}] value {v64:.6f}: value err device {e_v:.2e} / torch fp32 {e_v32:.2e} (rel "
           f"{e_v / v64:.2e} / {e_v32 / v64:.2e}); gradient rel-L2 device {e_g:.2e} / torch fp32 {e_g32:.2e}")
    assert 0.0 <= k["val"] <= 2.0
    assert e_v <= 4.0 * e_v32, (e_v, e_v32)
    assert e_g <= 4.0 * e_g32, (e_g, e_g32)
    off = torch.ones((h, w), dtype=torch.bool)
    off[::st, ::st] = False
    assert not k["grad"][0][:, off].any()
    # run to run, bitwise
    val2, sg2, grad2 = eng.selfsim_term(nhwc(k["f"]), nhwc(k["fc"]), st, EPS, coef=1.0)
    assert float(val2.cpu()[0]) == k["val"] and torch.equal(sg2.cpu(), k["sg"])
    assert torch.equal(grad2.cpu().permute(2, 0, 1).unsqueeze(0).double(), k["grad"])


# ---- 4. image = content, 5. degenerate maps ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 12, 13, 1), (256, 7, 33, 1), (512, 33, 35, 1), (128, 70, 66, 2)])
def test_image_equal_to_the_content_stand_alone(eng, shape):
    """N = M bit for bit: the value is exactly 0, every sign is 0 and every gradient entry is 0."""
    c, h, w, st = shape
    f = relu_noise(c, h, w, seed=7)
    val, sg, grad = eng.selfsim_term(nhwc(f), nhwc(f.clone()), st, EPS, coef=3.0)
    assert float(val.cpu()[0]) == 0.0 and not sg.cpu().any() and not grad.cpu().any()


def test_degenerate_maps(eng):
    """All-zero and constant maps on either side: a finite value in [0, 2] and a finite gradient (the clamp and s + eps).
    Exactly 0 is asserted for two IDENTICAL constant maps only (all-zero maps included).  Two different constants - (one, big)
    below - are held to finite and [0, 2]: every off-diagonal D of a constant map v is the same d(v) = 1 - |v|^2 / (|v|^2 + eps)
    as fp32 rounds it, N is d / ((n - 1) d + eps) off the diagonal, and with eps in both places that differs between two
    constants unless both d round to 0."""
    c, h, w = 128, 6, 5
    f = relu_noise(c, h, w, seed=3)
    zero, one, big = torch.zeros((1, c, h, w)), torch.ones((1, c, h, w)), torch.full((1, c, h, w), 5.0)
    for img, con in ((zero, f), (f, zero), (one, f), (f, big), (one, big), (zero, one)):
        val, sg, grad = eng.selfsim_term(nhwc(img), nhwc(con), 1, EPS)
        v = float(val.cpu()[0])
        assert np.isfinite(v) and 0.0 <= v <= 2.0, v
        assert torch.isfinite(grad).all()
    for same in (zero, one, big):
        val, sg, grad = eng.selfsim_term(nhwc(same), nhwc(same.clone()), 1, EPS)
        assert float(val.cpu()[0]) == 0.0 and not sg.cpu().any() and not grad.cpu().any()


def test_stand_alone_pieces_refuse_what_they_cannot_read(eng):
    from artstyletransfer_amd._lib import NstError
    f = nhwc(relu_noise(64, 6, 7, seed=1))
    view = dev(relu_noise(64, 6, 7, seed=1)).squeeze(0).permute(1, 2, 0)
    assert not view.is_contiguous()
    for bad in (view, f.double(), f.unsqueeze(0)):
        with pytest.raises(NstError):
            eng.selfsim_matrix(bad)
        with pytest.raises(NstError):
            eng.selfsim_term(bad, f)
    with pytest.raises(NstError):
        eng.selfsim_term(f, nhwc(relu_noise(64, 6, 8, seed=1)))
    for bad in (0, 257, 1.5):
        with pytest.raises(ValueError):
            eng.selfsim_matrix(f, stride=bad)
    with pytest.raises(ValueError):
        eng.selfsim_matrix(f, epsilon=0.0)
    big = torch.zeros((65, 64, 64), device="cuda:0")                 # 4160 samples at stride 1
    with pytest.raises(ValueError):
        eng.selfsim_matrix(big)
    assert eng.lib.nst_selfsim_matrix(eng.ctx, big.data_ptr(), 65, 64, 64, 1, 1e-5, big.data_ptr(), None, None) == -1
    g96 = torch.zeros((4, 4, 96), device="cuda:0")
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.selfsim_matrix(g96)


# ---- 6. - 8. the closure under the device's decisions ------------------------------------------------------------------------
class PatchedOracle:
    """cpu_ref.level_loss and cpu_ref.LevelTargets with the term at the device's decisions: LevelTargets gains the content's
    maps and its level number (the order the targets are made in), level_loss calls the original (or whatever a test patched
    in before), adds sum_k w_k selfsim_k (ascending map order) to the total of a level with the term and returns the same
    four-entry row.  `given[level][map]`: the device's (sg, live = D != 0 off the diagonal), which the test hands over before
    the first evaluation; `strides[level]`: six strides or None.  The term is in EVERY weighting of a closure - its weights are
    its own, as on the device.  `log` keeps, per level_loss call, (weighted term, {map: selfsim_k})."""

    def __init__(self, monkeypatch, w, strides):
        self.w, self.strides = tuple(w), strides
        self.level_loss0, self.targets0 = cpu_ref.level_loss, cpu_ref.LevelTargets
        self.given, self.log, self.made = {}, [], 0
        monkeypatch.setattr(cpu_ref, "level_loss", self.level_loss)
        monkeypatch.setattr(cpu_ref, "LevelTargets", self.targets)

    def targets(self, content_t, style_t, weights):
        tg = self.targets0(content_t, style_t, weights)
        with torch.no_grad():
            cf = cpu_ref.vgg19_features(content_t, weights)
            tg.selfsim_content = {i: cf[i].detach() for i in range(6) if self.w[i] > 0}
        tg.selfsim_level = self.made
        self.made += 1
        return tg

    def term(self, feats, tg):
        l = tg.selfsim_level
        if self.strides[l] is None:
            return None, {}
        total, vals = None, {}
        for i in range(6):
            if not self.w[i] > 0:
                continue
            sg, live = self.given[l][i]
            v = selfsim_ref.value_under(feats[i], tg.selfsim_content[i], sg, self.strides[l][i], EPS, live)
            vals[i] = float(v.detach())
            t = torch.tensor(np.float32(self.w[i])) * v
            total = t if total is None else total + t
        return total, vals

    def level_loss(self, x, tg, weights, cw, sw, tvw, decisions=None, record=None):
        seen = []
        inner = cpu_ref.vgg19_features

        def keep(*a, **k):
            seen.append(inner(*a, **k))
            return seen[-1]

        cpu_ref.vgg19_features = keep             # (the features the original computes, not a second forward pass)
        try:
            total, content, style, tv = self.level_loss0(x, tg, weights, cw, sw, tvw, decisions, record)
        finally:
            cpu_ref.vgg19_features = inner
        term, vals = self.term(seen[0], tg)
        self.log.append((float(term.detach()) if term is not None else 0.0, vals))
        return (total + term if term is not None else total), content, style, tv


NO_TV = TERMS[:3]
TV_ONLY = TERMS[3:]

# relu4_1 (a style map) and conv4_2 (the content map).  Measured on the CPU (the oracle and tests/selfsim_ref.py, the tests'
# synthetic weights): on the 64x96 two-level job the level totals are 3.1e4 / 3.7e4 and selfsim is 0.084 / 0.050 on relu4_1 and
# 0.065 / 0.035 on conv4_2 at stride 1, so these weights put the term at about 42 % / 25 % of the level totals
W_34 = (0.0, 0.0, 0.0, 1.5e5, 1.5e5, 0.0)
ONES = (1,) * 6


def _strides(levels_num, st=ONES, levels=None):
    return [tuple(st) if levels is None or l in levels else None for l in range(levels_num)]


def _set_selfsim(e, contents, w, strides, prep=cpu_ref.prepare_img):
    for i in range(len(contents)):
        if strides[i] is not None:
            e.set_selfsim(i, dev(prep(contents[i])), w, strides[i], EPS)


def _setup(e, contents, styles, w, strides, prepare=None):
    h, wd = contents[0].shape[:2]
    e.configure(len(contents), h, wd)
    if prepare:
        prepare(e)
    for i in range(len(contents)):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))
    _set_selfsim(e, contents, w, strides)


def _decisions_of(e, w, what=""):
    given = {}
    for l in range(e.levels):
        if e.selfsim_setting(l) is None:
            continue
        given[l] = {}
        for i in range(6):
            if w[i] > 0:
                d, s, sg = e.selfsim_decisions(l, i)
                d, sg = d.cpu(), sg.cpu()
                n = d.shape[0]
                live = (d != 0) | torch.eye(n, dtype=torch.bool)
                given[l][i] = (sg, live)
                report(f"selfsim {what} level {l} map {i}: n={n}, signs +/0/- {int((sg > 0).sum())}/{int((sg == 0).sum())}/{int((sg < 0).sum())}, "
                       f"clamped {int((~live).sum())}")
                assert not d.diagonal().any() and int((sg == 0).sum()) <= n + n * n // 100
    return given


def _the_term_counts(patched, xt, tg, weights, what, cache=None, lo=0.10, hi=0.60):
    """On the CPU: the term is between 10 % and 60 % of every level total that carries it - a build that ignores it cannot
    pass, and it does not drown the rest."""
    rec = []
    patched.log.clear()
    loss, grad, rows = cpu_ref.closure_eval(xt, tg, weights, CW, SW, TVW, record=rec)
    if cache is not None:
        cache["all"] = (loss, grad, rows, rec)
    assert len(patched.log) == len(rows)
    for l, ((term, vals), row) in enumerate(zip(patched.log, rows)):
        share = term / row[0]
        report(f"selfsim {what} level {l}: term {term:.4e} of total {row[0]:.4e} = {share:.1%}; selfsim_k = {vals}")
        if vals:
            assert lo <= share <= hi, (what, l, share)


def _additivity(e, xt, what):
    """The term is in every weighting with its own weights, so the sum of the content, style and tv gradients holds it three
    times and the weighted sum once; the closure with cw = sw = tvw = 0 is the term alone (same forward pass, same
    decisions): g(all) = g(content) + g(style) + g(tv) - 2 g(0, 0, 0), to hip_helpers' 2e-6."""
    xd = dev(xt)
    g = {name: e.closure(xd, *w3)[0].cpu().numpy().astype(np.float64) for name, w3 in TERMS + (("selfsim", (0.0, 0.0, 0.0)),)}
    s = g["content"] + g["style"] + g["tv"] - 2.0 * g["selfsim"]
    add = float(np.linalg.norm(g["all"] - s) / np.linalg.norm(s))
    share = float(np.linalg.norm(g["selfsim"]) / np.linalg.norm(g["all"]))
    report(f"selfsim {what}: |g(all) - (sum of the weightings - 2 g(term alone))| / |.| = {add:.1e}; |g(term alone)| / |g(all)| = {share:.2f}")
    assert add < 2e-6, (what, add)
    assert share > 0.01, (what, share)


def _strict(e, monkeypatch, vgg_weights, what, w, strides=None, prepare=None, job="64x96_L1"):
    c, s, xt = _job(job)
    strides = strides or _strides(len(c))
    patched = PatchedOracle(monkeypatch, w, strides)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, w, strides, prepare)
    e.closure(dev(xt), CW, SW, TVW)
    patched.given = _decisions_of(e, w, what)
    cache = {}
    _the_term_counts(patched, xt, tg, vgg_weights, what, cache)
    # losses 1e-5, rows 2e-5, gradient 2e-5 under the device's decisions (hip_helpers' standing tolerances), additivity 2e-6
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"selfsim {what}", terms=NO_TV, own_cache=cache)
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"selfsim {what}", terms=TV_ONLY)
    _additivity(e, xt, what)
    return patched


def test_path_batched_walker(eng, vgg_weights, monkeypatch):
    """Weights on the content map (4) and a style map (3): the mid-chain site with the content gradient in the addend, and the
    one without."""
    _strict(eng, monkeypatch, vgg_weights, "batched walker", W_34)


def test_path_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _strict(eng_per_level, monkeypatch, vgg_weights, "per-level walker", W_34)


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_strides_two_and_three_and_one_level_of_two(eng, eng_per_level, vgg_weights, monkeypatch, which):
    """Stride 2 on relu4_1 and 3 on conv4_2, on level 0 of two (the other level's row and gradient are what they are without
    the term).  Measured on the CPU: selfsim is 0.084 and 0.063 there, 42 % of the level total."""
    e = eng if which == "batched" else eng_per_level
    st = (1, 1, 1, 2, 3, 1)
    strides = _strides(2, st, levels=(0,))
    p = _strict(e, monkeypatch, vgg_weights, f"level 0 of two, strides 2 and 3 [{which}]", W_34, strides)
    assert e.selfsim_setting(1) is None and e.selfsim_setting(0) == (W_34, st, EPS)
    assert not e.selfsim_losses().cpu().numpy()[1].any()
    assert p.log[-1][1] == {}
    d, s, sg = e.selfsim_decisions(0, 4)
    assert d.shape[0] == selfsim_ref.counts(8, 12, 3) and s.numel() == d.shape[0] and tuple(sg.shape) == tuple(d.shape)


def test_path_average_pooling(eng, vgg_weights, monkeypatch):
    """Measured on the CPU: level totals 2.8e4 / 3.3e4, selfsim 0.083 + 0.064 and 0.042 + 0.028: 44 % / 24 %."""
    from test_hip_pooling import avg_vgg19_features
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "avg pooling", W_34, prepare=lambda e: e.set_pooling("avg"))
    finally:
        eng.reset_pooling()


# Under use_relu=False map 5 is conv5_1 before its ReLU - a signed map at the top of the chain, whose launch applies no mask.
# Measured on the CPU as above: selfsim is 0.065 / 0.035 on conv4_2 and 0.036 / 0.014 on conv5_1, so these weights put the term
# at about 40 % / 20 % of the level totals
W_45 = (0.0, 0.0, 0.0, 0.0, 1.5e5, 3e5)


def test_path_pre_relu_taps(eng, vgg_weights, monkeypatch):
    monkeypatch.setattr(cpu_ref, "vgg19_features", prerelu_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "pre-ReLU taps", W_45, prepare=lambda e: e.set_taps(4, [0, 1, 2, 3, 5], use_relu=False))
        assert float(eng.level_activation(0, 12).min().cpu()) < 0.0          # (the map is signed)
    finally:
        eng.reset_taps()


def _path_beside_the_other_terms_on_the_same_map(e, vgg_weights, monkeypatch):
    import test_hip_hist as th
    import test_hip_remd as tr
    from test_hip_mrf import PatchedOracle as MrfOracle, W_34 as MRF_W
    c, s, xt = _job("64x96_L1")
    w_hist = (0.0, 0.0, 0.0, 5000.0, 0.0, 0.0)
    mrf = MrfOracle(monkeypatch, MRF_W)
    hist = th.PatchedOracle(monkeypatch, w_hist)
    remd = tr.PatchedOracle(monkeypatch, tr.W_23, tr._strides(2))
    strides = _strides(2)
    patched = PatchedOracle(monkeypatch, W_34, strides)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, W_34, strides)
    for i in range(2):
        e.set_patches(i, dev(cpu_ref.prepare_img(s[i])), MRF_W, 1, EPS)
    th._set_histograms(e, s, w_hist)
    tr._set_remd(e, s, tr.W_23, tr._strides(2))
    try:
        hist.given = th._hand_over(e, dev(xt), w_hist, th.BINS, "beside selfsim")
        mrf.nn = {l: {i: e.patch_matches(l, i).cpu() for i in range(6) if MRF_W[i] > 0} for l in range(2)}
        remd.given = tr._matches_of(e, tr.W_23, "beside selfsim")
        patched.given = _decisions_of(e, W_34, "beside MRF, hist and EMD")
        cache = {}
        _the_term_counts(patched, xt, tg, vgg_weights, "beside MRF, hist and EMD", cache, lo=0.05)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "selfsim beside MRF, hist and EMD", terms=NO_TV, own_cache=cache)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "selfsim beside MRF, hist and EMD", terms=TV_ONLY)
    finally:
        e.clear_patches()
        e.clear_histograms()
        e.clear_remd()


def test_path_beside_the_other_terms_on_the_same_map(eng, vgg_weights, monkeypatch):
    """relu4_1 carries all four terms: the MRF term's addend first, the histogram loss and the relaxed EMD term added to it,
    then this term.  The oracles of the three other tests are patched first and handed the device's decisions; this one wraps
    them, as the loss row adds the term last."""
    _path_beside_the_other_terms_on_the_same_map(eng, vgg_weights, monkeypatch)


def test_path_beside_the_other_terms_on_the_same_map_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _path_beside_the_other_terms_on_the_same_map(eng_per_level, vgg_weights, monkeypatch)


# -- taps beyond cpu_ref.level_loss: test_hip_style_blend's restatement with the term added
def _restated_closure(x, targets, weights, cw, sw, tvw, taps, decisions, w, given):
    content_i, style_set = taps
    x = x.detach().clone().requires_grad_(True)
    lv, total, rows, terms = [x], None, [], []
    for l, tg in enumerate(targets):
        if l > 0:
            lv.append(cpu_ref.bicubic_half(lv[l - 1]))
        dec = decisions[l] if decisions is not None else None
        f = cpu_ref.vgg19_features(lv[l], weights, dec)
        content = F.mse_loss(tg.content, f[content_i].squeeze(0), reduction="mean")
        style = 0.0
        for i in style_set:
            style = style + F.mse_loss(tg.grams[i][0], cpu_ref.gram_matrix(f[i])[0], reduction="mean")
        style = style / len(style_set)
        tv = cpu_ref.total_variation(lv[l], dec.tv if dec is not None else None)
        term = None
        for i in range(6):
            if w[i] > 0:
                sg, live = given[l][i]
                t = torch.tensor(np.float32(w[i])) * selfsim_ref.value_under(f[i], tg.selfsim_content[i], sg, 1, EPS, live)
                term = t if term is None else term + t
        t = cw * content + sw * style + tvw * tv + term
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
        terms.append(float(term.detach()))
    total.backward()
    return total.detach(), x.grad.detach(), rows, terms


# Measured on the CPU: with every map a style map the level totals are 2.7e4 / 3.3e4 (W_34: 45 % / 27 %); with content 5 and
# styles 0..3 they are 3.6e4 / 4.1e4 and selfsim is 0.039 / 0.026 on relu5_1, so 4e5 there is 30 % / 20 %
OTHER_TAPS = {"the content map is also a style map": ((4, (0, 1, 2, 3, 4, 5)), W_34),
              "the content map alone at the top of the chain": ((5, (0, 1, 2, 3)), (0.0, 0.0, 0.0, 0.0, 0.0, 4e5))}


def _path_other_taps(e, vgg_weights, case):
    from test_hip_style_blend import device_decisions as decisions_of, restated_targets
    taps, w = OTHER_TAPS[case]
    c, s, xt = _job("64x96_L1")
    prep = cpu_ref.prepare_img
    try:
        e.configure(2, 64, 96)
        e.set_taps(taps[0], list(taps[1]))
        tg = []
        for i in range(2):
            e.set_targets(i, dev(prep(c[i])), dev(prep(s[i])))
            t = restated_targets(prep(c[i]), [prep(s[i])], ((1.0,) * 6,), vgg_weights, taps)
            with torch.no_grad():
                cf = cpu_ref.vgg19_features(prep(c[i]), vgg_weights)
            t.selfsim_content = {k: cf[k].detach() for k in range(6) if w[k] > 0}
            tg.append(t)
        _set_selfsim(e, c, w, _strides(2))
        xd = dev(xt)
        for name, (cw, sw, tvw) in (("term alone", (0.0, 0.0, 0.0)), ("all", (CW, SW, TVW))):
            grad, losses = e.closure(xd, cw, sw, tvw)
            dec = decisions_of(e, xd, vgg_weights, taps)
            given = _decisions_of(e, w, case)
            losses = losses.cpu().numpy()
            loss, g_ref, rows, terms = _restated_closure(xt, tg, vgg_weights, cw, sw, tvw, taps, dec, w, given)
            e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
            e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
            shares = [t / r[0] for t, r in zip(terms, rows)]
            report(f"selfsim {case} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}; share of the level "
                   f"totals {[round(v, 3) for v in shares]}")
            if name == "all":
                assert all(0.10 <= v <= 0.60 for v in shares), (case, shares)
            assert e_l < 1e-5, (case, name, e_l)
            check_rows(losses[:-1].reshape(2, 4), np.array(rows), 2e-5, cw, sw, tvw)
            assert e_g < 2e-5, (case, name, e_g)
    finally:
        e.reset_taps()


@pytest.mark.parametrize("case", list(OTHER_TAPS))
def test_path_other_taps(eng, vgg_weights, case):
    """style_mask 0x3F with the term on conv4_2 and relu4_1 (content gradient and the term in one addend, beside the Gram second
    source); and content 5 with styles 0..3: the content map is no style map and is the top of the chain, so the term's
    gradient joins the content gradient in front of the mask pass - the one walker site beyond those of the style terms."""
    _path_other_taps(eng, vgg_weights, case)


@pytest.mark.parametrize("case", list(OTHER_TAPS))
def test_path_other_taps_per_level_walker(eng_per_level, vgg_weights, case):
    _path_other_taps(eng_per_level, vgg_weights, case)


def test_path_luminance(eng, vgg_weights, monkeypatch):
    """The luminance closure with the term = the patched oracle's closure at E(u), gradient summed over the channels; the
    content's maps are those of the content's luminance plane."""
    from artstyletransfer_amd import host_image
    from test_hip_color import expand, lum_decisions, lum_targets, start_u
    c, s = _levels(64, 96, 2, 1), _levels(70, 110, 2, 2)
    # (measured with the oracle on the CPU: the luminance job's level totals are a third of the colour job's, and W_34 would be
    # 74 % / 52 % of them; a quarter of it is 42 % / 21 %)
    w = tuple(0.25 * v for v in W_34)
    patched = PatchedOracle(monkeypatch, w, _strides(2))
    try:
        eng.configure(2, 64, 96)
        eng.set_color("luminance")
        alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
        cu, su = lum_targets(c, s, alpha, beta)
        for i in range(2):
            eng.set_targets(i, dev(torch.from_numpy(cu[i])), dev(torch.from_numpy(su[i])))
            eng.set_selfsim(i, dev(torch.from_numpy(cu[i])), w, 1, EPS)
        tg = [cpu_ref.LevelTargets(expand(torch.from_numpy(a)), expand(torch.from_numpy(b)), vgg_weights) for a, b in zip(cu, su)]
        u = start_u(c[0])
        ud = dev(u.reshape(1, 1, 64, 96))
        xt = expand(u)
        grad, losses = eng.closure(ud, CW, SW, TVW)
        patched.given = _decisions_of(eng, w, "luminance")
        dec = lum_decisions(eng, ud)
        losses = losses.cpu().numpy()
        patched.log.clear()
        loss, _, rows = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW)
        shares = [m / r[0] for (m, _), r in zip(patched.log, rows)]
        report(f"selfsim luminance: share of the level totals {[round(v, 3) for v in shares]}")
        assert all(0.10 <= v <= 0.60 for v in shares), shares
        assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
        check_rows(losses[:-1].reshape(2, 4), np.array(rows), 1e-5, CW, SW, TVW)
        _, g_eq, _ = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_eq.sum(dim=1).numpy().reshape(64, 96))
        report(f"selfsim luminance: gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_g < 2e-5
    finally:
        eng.reset_color()


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_image_equal_to_the_content_through_a_job(eng, eng_per_level, which):
    """The level images of the content itself: every selfsim_k is exactly 0, every sign is 0, and the gradient of the closure
    with cw = sw = tvw = 0 - the term alone - is exactly 0.  One level: a lower level's image is the engine's own down-sampling
    of x, not the content level the setter was given."""
    e = eng if which == "batched" else eng_per_level
    c, s, _ = _job("64x96_L1")
    _setup(e, c[:1], s[:1], W_34, _strides(1))
    x = dev(cpu_ref.prepare_img(c[0]))
    g, l = e.closure(x, 0.0, 0.0, 0.0)
    assert not e.selfsim_losses().cpu().numpy().any()
    for i in (3, 4):
        d, sv, sg = e.selfsim_decisions(0, i)
        assert not sg.cpu().any() and bool((sv.cpu() > 0).all())
    l = l.cpu().numpy()
    assert not g.cpu().numpy().any() and l[0] == 0.0 and l[-1] == 0.0          # (the row's other entries are the unweighted terms)


# ---- 9. bits ---------------------------------------------------------------------------------------------------------------------
MIXED_W = (0.0, 0.0, 8e4, 1.5e5, 1.5e5, 0.0)
MIXED_ST = (1, 1, 2, 1, 1, 1)


def _mixed_job(e, name="64x96_L1"):
    c, s, xt = _job(name)
    _setup(e, c, s, MIXED_W, _strides(len(c), MIXED_ST))
    return dev(xt), c, s


def test_halves_equal_the_whole_and_run_to_run_bitwise(eng):
    x, _, _ = _mixed_job(eng)
    g, l = eng.closure(x, CW, SW, TVW)
    m = eng.selfsim_losses()
    dec = [eng.selfsim_decisions(lv, 3) for lv in range(2)]
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    assert np.array_equal(_bits(m), _bits(eng.selfsim_losses()))
    for lv, (d, s, sg) in enumerate(dec):
        d2, s2, sg2 = eng.selfsim_decisions(lv, 3)
        assert torch.equal(d, d2) and torch.equal(s, s2) and torch.equal(sg, sg2)
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_level_masks_add_up(eng, eng_per_level, which):
    e = eng if which == "batched" else eng_per_level
    x, _, _ = _mixed_job(e)
    g, l = e.closure(x, CW, SW, TVW)
    m = e.selfsim_losses().cpu().numpy()
    g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    gs, ls, ms = np.zeros_like(g), np.zeros_like(l), np.zeros_like(m)
    for mask in (1, 2):
        gm, lm = e.closure_levels(x, CW, SW, TVW, mask)
        mm = e.selfsim_losses().cpu().numpy()
        assert not mm[[lv for lv in range(2) if not (mask >> lv) & 1]].any()          # zeros for levels outside the mask
        gs += gm.cpu().numpy()
        ls += lm.cpu().numpy()
        ms += mm
    np.testing.assert_allclose(ls, l, rtol=1e-6)
    assert np.array_equal(ms, m)
    err = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
    report(f"selfsim level masks [{which}]: |sum - unsharded| / |.| = {err:.1e}")
    assert err <= 1e-6


def test_lbfgs_is_the_same_with_reuse_and_lazy_backward_on_or_off(eng):
    from artstyletransfer_amd.engine import PixelOptimizer
    x0, _, _ = _mixed_job(eng)
    runs = {}
    for reuse, lazy in ((False, False), (True, True)):
        opt = PixelOptimizer(eng, "lbfgs")
        try:
            opt.set_closure_reuse(reuse)
            opt.set_lazy_backward(lazy)
            x = x0.clone()
            out = []
            for _ in range(5):
                info, rows = opt.step(x, CW, SW, TVW)
                out.append((info.closures, info.total_closures, info.accepted, info.history, rows.view(np.uint32).copy(), _bits(x)))
            runs[(reuse, lazy)] = (out, opt.closure_stats(), opt.backward_stats())
        finally:
            opt.close()
    base = runs[(False, False)][0]
    out, stats, bw = runs[(True, True)]
    for k, (a, b) in enumerate(zip(out, base)):
        assert a[:4] == b[:4], (k, a[:4], b[:4])
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), k
    assert np.isfinite(base[-1][4].view(np.float32)).all()
    assert sum(stats) == base[-1][1], (stats, bw)


def test_selfsim_losses_times_the_weights_plus_the_other_terms_are_the_row_totals(eng):
    """total = ((cw content + sw style) + tvw tv) + w_2 selfsim_2 + w_3 selfsim_3 ... in ascending map order, every product and
    sum rounded to fp32: bitwise from what the closure returns; zeros for the maps without the term; every value in [0, 2]."""
    x, _, _ = _mixed_job(eng)
    _, l = eng.closure(x, CW, SW, TVW)
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    m = eng.selfsim_losses().cpu().numpy()
    on = [i for i in range(6) if MIXED_W[i] > 0]
    assert m.shape == (2, 6) and not m[:, [0, 1, 5]].any() and (m[:, on] > 0).all() and (m <= 2.0).all()
    f32 = np.float32
    for lv in range(2):
        total = (f32(CW) * rows[lv, 1] + f32(SW) * rows[lv, 2]) + f32(TVW) * rows[lv, 3]
        for i in on:
            total = f32(total + f32(MIXED_W[i]) * m[lv, i])
        assert total == rows[lv, 0], (lv, total, rows[lv, 0])


@pytest.mark.parametrize("how", ["cleared", "all-zero weights"])
@pytest.mark.parametrize("batched", [True, False])
def test_no_term_is_bitwise_an_engine_that_never_called_the_setter(vgg_weights, batched, how):
    """A job whose term was cleared, or whose setter was given all-zero weights, equals a job never given one: bits, recorded
    launches and nst_ctx_bytes."""
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt = _job("64x96_L1")
    out = []
    for call in (False, True):
        e = StyleEngine(vgg_weights, 0, batched=batched)
        try:
            e.set_timing(2)
            e.configure(2, 64, 96)
            for i in range(2):
                e.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
            if call:
                before = e.bytes()
                if how == "cleared":
                    _set_selfsim(e, c, MIXED_W, _strides(2, MIXED_ST))
                    assert e.bytes() > before
                    e.closure(dev(xt), CW, SW, TVW)
                    assert e.selfsim_losses().cpu().numpy().any()
                    e.clear_selfsim()
                else:
                    _set_selfsim(e, c, (0.0,) * 6, _strides(2, MIXED_ST))
                assert e.bytes() == before
                assert all(e.selfsim_setting(i) is None for i in range(2))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            assert not e.selfsim_losses().cpu().numpy().any()
            out.append((_bits(g), _bits(l), e.last_closure_launches()))
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    strip = lambda rec: [{k: v for k, v in d.items() if k not in ("ms",)} for d in rec]        # noqa: E731
    assert strip(out[0][2]) == strip(out[1][2]) and len(out[0][2]) > 0


# ---- 10. life cycle and refusals ---------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(eng, vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine, _ptr, _stream
    x, c, s = _mixed_job(eng)
    g0, l0 = eng.closure(x, CW, SW, TVW)
    before = [eng.selfsim_setting(i) for i in range(2)]
    assert before[0] == (MIXED_W, MIXED_ST, EPS) and before[1] == (MIXED_W, MIXED_ST, EPS)
    content = dev(cpu_ref.prepare_img(c[0]))
    i6 = lambda v: (C.c_int * 6)(*v)                                    # noqa: E731

    def raw(level=0, w=MIXED_W, st=MIXED_ST, eps=1e-5, img=content, h=64, wd=96, e=eng):
        return e.lib.nst_level_set_selfsim(e.ctx, level, _ptr(img), h, wd, (C.c_float * 6)(*w), i6(st), eps, _stream(e.device))

    # NST_E_ARG, and a refusal leaves the level as it was
    assert raw(level=-1) == -1 and raw(level=2) == -1
    for bad in (-1.0, float("nan"), float("inf")):
        assert raw(w=(0.0, 0.0, bad, 1.0, 0.0, 0.0)) == -1
    for eps in (0.0, -1e-5, float("nan"), float("inf")):
        assert raw(eps=eps) == -1
    for bad in (0, 257, -1):
        assert raw(st=(1, 1, bad, 1, 1, 1)) == -1 and raw(st=(1, 1, 1, 1, 1, bad)) == -1
    assert raw(h=32, wd=48) == -1 and raw(h=70, wd=110) == -1          # the size must be the level's
    assert raw(level=1) == -1                                           # (64x96 is not level 1's size)
    assert raw(w=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0)) == -1                 # relu1_1 at stride 1: 6144 samples
    assert raw(w=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0), st=(2, 1, 1, 1, 1, 1)) == 0       # 1536 samples
    assert eng.selfsim_setting(0) == ((1.0, 0.0, 0.0, 0.0, 0.0, 0.0), (2, 1, 1, 1, 1, 1), EPS)
    _mixed_job(eng)
    # a map the job does not use: conv4_2 when another map is the content map and it is no style map
    eng.set_taps(5, [0, 1, 2, 3])
    try:
        assert raw(w=(0.0, 0.0, 0.0, 0.0, 1.0, 0.0)) == -1
        assert raw(w=(0.0, 0.0, 0.0, 1.0, 0.0, 1.0)) == 0              # a style map and the content map
    finally:
        eng.reset_taps()
    x, c, s = _mixed_job(eng)
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # a guided level, in either order of the two calls
    planes = torch.ones((2, 64, 96), device="cuda:0") * 0.5
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_guidance(0, planes)
    eng.clear_selfsim(0)
    eng.set_guidance(0, planes)
    assert raw() == -2 and eng.selfsim_setting(0) is None
    eng.clear_guidance()
    # a pending backward half goes with a new term
    _mixed_job(eng)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_selfsim(0, content, W_34)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure_backward(x, CW, SW, TVW)
    # configure, set_taps, set_pooling and set_color drop the term
    for drop, undo in ((lambda: eng.configure(2, 64, 96), None), (lambda: eng.set_taps(4, [0, 1, 2, 3]), eng.reset_taps),
                       (lambda: eng.set_pooling("avg"), eng.reset_pooling), (lambda: eng.set_color("luminance"), eng.reset_color)):
        _mixed_job(eng)
        assert eng.selfsim_setting(0) is not None
        drop()
        try:
            assert all(eng.selfsim_setting(i) is None for i in range(2))
        finally:
            if undo:
                undo()
    # the Python setter refuses before the library does
    _mixed_job(eng)
    for bad in ({1: -1.0}, [1.0] * 5, "x", {"relu9_9": 1.0}):
        with pytest.raises(ValueError):
            eng.set_selfsim(0, content, bad)
    with pytest.raises(ValueError):
        eng.set_selfsim(0, content, W_34, strides=0)
    with pytest.raises(ValueError):
        eng.set_selfsim(0, content, W_34, epsilon=0.0)
    # the stripe closure, and the stripe sharding of the optimiser before any stripe engine is made; the bytes come back
    e1 = StyleEngine(vgg_weights, 0)
    try:
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        assert raw(e=e1, img=xs) == -2                                  # no configured job
        e1.configure(1, 64, 96)
        e1.set_targets(0, xs, xs)
        before = e1.bytes()
        e1.set_selfsim(0, xs, W_34)
        assert e1.bytes() > before
        d, sv, sg = e1.selfsim_decisions(0, 4)                           # zeros before any closure
        assert not d.cpu().any() and not sv.cpu().any() and not sg.cpu().any()
        with pytest.raises(NstError, match=r"\(-2\)"):
            e1.window_begin(xs, 0, 64, 64)
        opt = PixelOptimizer(e1, "lbfgs")
        try:
            with pytest.raises(ValueError, match="selfsim_weight cannot be combined with stripe sharding"):
                opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
        finally:
            opt.close()
        # the readers name a level out of range the same way, and a map without the term
        assert e1.lib.nst_level_selfsim(e1.ctx, 1, None, None, None) == -1
        assert e1.lib.nst_level_selfsim_decisions(e1.ctx, 1, 3, _ptr(xs), None, None, _stream(e1.device)) == -1
        assert e1.lib.nst_level_selfsim_decisions(e1.ctx, 0, 0, _ptr(xs), None, None, _stream(e1.device)) == -2
        e1.clear_selfsim()
        assert e1.bytes() == before
        e1.window_begin(xs, 0, 64, 64)
    finally:
        e1.close()


@pytest.mark.parametrize("kw", [{"conv_mode": "f32"}, {"conv_mode": "bf16x3"}, {"use_graph": True}])
def test_other_arithmetic_modes_and_a_graph_context_refuse_the_term(vgg_weights, kw):
    from artstyletransfer_amd.engine import StyleEngine, _ptr, _stream
    e = StyleEngine(vgg_weights, 0, **kw)
    try:
        e.configure(1, 64, 96)
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        ones = (C.c_int * 6)(*ONES)
        assert e.lib.nst_level_set_selfsim(e.ctx, 0, _ptr(xs), 64, 96, (C.c_float * 6)(*W_34), ones, 1e-5, _stream(e.device)) == -2
        e.clear_selfsim()                                          # clearing is no setting
        assert e.selfsim_setting(0) is None
    finally:
        e.close()


# ---- 11. a whole job -------------------------------------------------------------------------------------------------------------
def _run_job(fn, seed=1, **kw):
    import neural_style_transfer as nst
    content = cpu_ref.synthetic_image(64, 96, seed=seed)
    style = cpu_ref.synthetic_image(70, 110, seed=seed + 1)
    pair = nst.ContentStylePair(("c", content), ("s", style))
    np.random.seed(1234)

    async def run():
        return [img async for _, img in fn(pair, CW, SW, TVW, "adam", "vgg19", "content+noise", 40, 1, 0.95, (9, 18, 36, -1, 0),
                                           (0.3, 0.2, 0.1, 0.2, 0.2), (0.2, 0.3, 0.4, 0.1, 0.0), (0.2, 0.3, 0.4, 0.6, 0.3),
                                           device=torch.device("cuda", 0), **kw)]
    return asyncio.run(run()), content


def test_whole_job(eng, vgg_weights):
    """neural_style_transfer_selfsim on a 64x96 pair (one level, which the driver resizes to a short edge of 256), 40 Adam steps:
    the image moves at every step (under L-BFGS as the reference constructs it almost every trial step of a short run is
    rejected, and the runs with and without the term would end within a digit of each other).  With selfsim_weight=None it is neural_style_transfer_remd(), bitwise.  With the term on the
    content map at a weight that makes it at least 30 % of the start image's total (asserted from the engine's own rows), the
    term's value after the run - read with the stand-alone pieces on the result's own map against the content level image's -
    is below that of the same job with the weight off, and the image has moved: the term's value at the end differs from its
    value after the first step in both runs."""
    from artstyletransfer_amd import host_image, selfsim_modes
    from artstyletransfer_amd.remd_loss import neural_style_transfer_remd
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim
    samples, weight = 256, 2e6
    out, content = _run_job(neural_style_transfer_selfsim, selfsim_weight=weight, selfsim_samples=samples)
    assert len(out) >= 1 and all(np.isfinite(o).all() for o in out)
    plain, _ = _run_job(neural_style_transfer_remd)
    off, _ = _run_job(neural_style_transfer_selfsim, selfsim_weight=None, selfsim_samples=samples)
    assert len(plain) == len(off) >= 1
    assert all(np.array_equal(a, b) for a, b in zip(plain, off))
    ch, cw_ = host_image.level_size(content.shape[0], content.shape[1], 0)
    content_level = eng.resize(dev(torch.from_numpy(content)), ch, cw_).cpu().numpy()
    with torch.no_grad():
        fc = cpu_ref.vgg19_features(cpu_ref.prepare_img(content_level), vgg_weights)[4]
        st = selfsim_modes.stride_for(fc.shape[2], fc.shape[3], samples)

        def selfsim_of(img):
            f = cpu_ref.vgg19_features(cpu_ref.prepare_img(np.ascontiguousarray(img, dtype=np.float32)), vgg_weights)[4]
            return float(eng.selfsim_term(nhwc(f), nhwc(fc), st, EPS, want_grad=False)[0].cpu()[0])
        first, with_term, without = selfsim_of(out[0]), selfsim_of(out[-1]), selfsim_of(plain[-1])
        first_plain = selfsim_of(plain[0])
    # the share at the job's start, from the engine: the same level, the same term, the first yielded image
    eng.configure(1, ch, cw_)
    lvl_c = dev(cpu_ref.prepare_img(content_level))
    style_level = eng.resize(dev(torch.from_numpy(cpu_ref.synthetic_image(70, 110, seed=2))), *host_image.level_size(70, 110, 0)).cpu().numpy()
    eng.set_targets(0, lvl_c, dev(cpu_ref.prepare_img(style_level)))
    eng.set_selfsim(0, lvl_c, weight, (1, 1, 1, 1, st, 1), EPS)
    _, rows = eng.closure(dev(cpu_ref.prepare_img(np.ascontiguousarray(plain[-1], dtype=np.float32))), CW, SW, TVW)
    total = float(rows.cpu()[0])
    term = weight * float(eng.selfsim_losses().cpu()[0, 4])
    eng.clear_selfsim()
    report(f"selfsim whole job: {len(out)} images; selfsim of conv4_2 after the first step {first:.5f} (without the term {first_plain:.5f}), at "
           f"the end with the term {with_term:.5f}, without {without:.5f}; the term is {term / total:.1%} of the total at the plain job's result")
    assert term / total >= 0.30, (term, total)
    assert len(out) > 1 and with_term != first and without != first_plain, (len(out), first, with_term, first_plain, without)
    assert with_term < without, (with_term, without)
