"""GPU: the histogram loss (nst_level_set_histograms; Risser, Wilmot & Barnes 2017) - every channel of a tapped map remapped
onto the style's histogram.
1. the pieces alone (nst_histogram_counts / _tables / _term) against tests/hist_ref.py: range and counts exactly, tables to
   1 ulp, remap and gradient to the bound of their roundings, the value to 1e-5, two runs bitwise;
2. the closure against the oracle with cpu_ref.level_loss replaced by a test-local one that adds the term EVALUATED ON THE
   DEVICE'S OWN MAP (monkeypatch: no oracle edit): the remap is steep, so a reference that recomputed it from features 1e-6
   away would land percent away on single units - the constant hist_i and the linear form <dF, F_oracle> carry
   the term's value and gradient through the oracle's network under the device's decisions, at hip_helpers' standing
   tolerances, over the paths the term's gradient takes;
3. closure halves, reproducibility, L-BFGS, level masks; 4. the loss row; 5. a cleared term; 6. life cycle and refusals;
7. a whole job."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch

import hist_ref
from hip_helpers import (CW, SW, TVW, TERMS, check_rows, closure_vs_oracle_under_equal_decisions, dev, levels as _levels,
                         oracle_targets, rel_l2, report)
from oracle import cpu_ref
from test_hip_gram_shift import _bits, _job, prerelu_vgg19_features

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                      # unit roundoff of fp32
TAP_LAYER = (0, 2, 4, 8, 9, 12)     # conv layer of each map index (kTapLayer)


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


# ---- 1. the pieces alone ------------------------------------------------------------------------------------------------------
def make_map(kind, n, c, seed):
    """(n, c) float32.  relu: half exact zeros; signed; edges: multiples of 1 / 16 in the power-of-two range [-2, 2], so that
    x = (v + 2) bins / 4 is exact and every value lies exactly on a bin edge at 256 and 1024 bins, every fourth at 16, and the
    maximum itself (x = bins: the last bin, f = 1) occurs in every channel; a flat channel (3) and an almost flat one (5, a
    range of one part in 2^20) in each."""
    g = np.random.default_rng(seed)
    if kind == "relu":
        x = np.maximum(g.standard_normal((n, c)) * 3.0, 0.0)
    elif kind == "signed":
        x = g.standard_normal((n, c)) * 2.0 - 0.5
    else:
        x = g.integers(-32, 33, size=(n, c)) / 16.0
        x[0, :], x[-1, :] = -2.0, 2.0               # the range is [-2, 2] in every channel: edges at k 4 / bins
    x = x.astype(np.float32)
    x[:, 3] = np.float32(0.75)
    x[:, 5] = np.float32(1.0)
    x[n // 2, 5] = np.float32(1.0) + np.float32(2.0 ** -20)
    return x


# (C, N image, N style, bins): two slabs of 32 channels and more; N = 15 (a 3x5 map, fewer pixels than lanes), 24, 96; 2500
# spans three workgroups of the counts pass (1024 threads, 128 pixels a step) with a share of 834, 777 and 1000 are no multiple
# of a workgroup's step; bins on either side of the 64 KB of dynamic LDS (512 bins) that needs the raised limit
PIECE_SHAPES = [(64, 15, 24, 2), (64, 24, 15, 16), (128, 96, 40, 256), (512, 15, 96, 1024), (64, 2500, 777, 256), (128, 1000, 96, 1024),
                (512, 96, 1000, 16)]
KINDS = ["relu", "signed", "edges"]
_PIECES = {}


def _pieces(eng, shape, kind, skind=None):
    """Device and reference results of one case, computed once and left unchanged."""
    key = (shape, kind, skind)
    if key not in _PIECES:
        c, n, ns, bins = shape
        f, fs = make_map(kind, n, c, seed=n + c), make_map(skind or kind, ns, c, seed=ns + c + 1)
        if skind == "flat-style-only":
            fs = make_map(kind, ns, c, seed=ns + c + 1)
            f[:, 3] = np.linspace(0.0, 1.0, n, dtype=np.float32)          # the image's channel 3 is live, the style's flat
        if skind == "flat-image-only":
            fs = make_map(kind, ns, c, seed=ns + c + 1)
            fs[:, 3] = np.linspace(-1.0, 1.0, ns, dtype=np.float32)
        fd, fsd = dev(torch.from_numpy(f)), dev(torch.from_numpy(fs))
        lo_hi, counts = eng.histogram_counts(fd, bins)
        s_lo_hi, s_counts = eng.histogram_counts(fsd, bins)
        ends = eng.histogram_table(lo_hi, counts, n, s_lo_hi, s_counts, ns)
        coef = 2.0 * 1000.0 / (c * n)
        val, grad = eng.histogram_term(fd, lo_hi, ends, coef)
        again = (eng.histogram_counts(fd, bins), eng.histogram_table(lo_hi, counts, n, s_lo_hi, s_counts, ns),
                 eng.histogram_term(fd, lo_hi, ends, coef))
        d = dict(f=f, fs=fs, coef=coef, lo_hi=lo_hi.cpu().numpy(), counts=counts.cpu().numpy(), s_lo_hi=s_lo_hi.cpu().numpy(),
                 s_counts=s_counts.cpu().numpy(), ends=ends.cpu().numpy(), val=float(val.cpu()), grad=grad.cpu().numpy(),
                 again=again, first=((lo_hi, counts), ends, (val, grad)))
        d["ref"] = hist_ref.full(f, fs, bins)
        _PIECES[key] = d
    return _PIECES[key]


def _ulps(a, b):
    """Distance in units of the last place of b's fp32 grid (both float32 arrays)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ulp = np.maximum(np.spacing(np.abs(b).astype(np.float32)).astype(np.float64), 2.0 ** -149)
    return np.abs(a - b) / ulp


def _check_pieces(d, shape, what):
    c, n, ns, bins = shape
    lo_hi, counts, s_lo_hi, s_counts, ends = d["ref"]
    # range and counts: exactly
    assert np.array_equal(d["lo_hi"], lo_hi), what
    assert np.array_equal(d["s_lo_hi"], s_lo_hi), what
    assert np.array_equal(d["counts"].astype(np.int64), counts), what
    assert np.array_equal(d["s_counts"].astype(np.int64), s_counts), what
    live = lo_hi[:, 1] != lo_hi[:, 0]
    assert (counts.sum(axis=1) == np.where(live, n, 0)).all()
    # tables: double arithmetic from equal integers, one final rounding; a contraction may move the double by an ulp of
    # double, which moves the fp32 result by at most 1 ulp
    worst = float(_ulps(d["ends"], ends).max())
    assert worst <= 1.0, (what, worst)
    assert not d["ends"][counts == 0].any()
    # remap and gradient at the DEVICE's tables.  R = fl(start + fl(f fl(end - start))): with d = end - start, p = f d,
    # |R_dev - R| <= u (|d| f + |p| + |R|) (1 + O(u)) <= u (2 |d| + |R|); then g = fl(coef fl(v - R_dev)):
    # |g_dev - g| <= |coef| (|R_dev - R| + u |v - R_dev|) + u |g|.  1.01 covers the second-order terms.
    r, flat, (start, fr, end) = hist_ref.remap(d["f"], d["lo_hi"], d["ends"], bins)
    coef = np.float64(np.float32(d["coef"]))
    g_ref = coef * (d["f"].astype(np.float64) - r)
    tol_r = U * (2.0 * np.abs(end - start) + np.abs(r))
    tol_g = 1.01 * (abs(coef) * (tol_r + U * np.abs(d["f"] - r)) + U * np.abs(g_ref)) + 2.0 ** -149
    err = np.abs(d["grad"].astype(np.float64) - g_ref)
    assert (err <= tol_g).all(), (what, float((err / tol_g).max()))
    assert not d["grad"][:, flat].any()
    # the value to the suite's 1e-5
    v_ref = float(((d["f"].astype(np.float64) - r) ** 2).sum() / r.size)
    assert d["val"] == pytest.approx(v_ref, rel=1e-5, abs=1e-30), what
    # two runs, bitwise
    (lh2, cn2), e2, (v2, g2) = d["again"]
    (lh1, cn1), e1, (v1, g1) = d["first"]
    assert torch.equal(cn1, cn2) and np.array_equal(_bits(lh1), _bits(lh2)) and np.array_equal(_bits(e1), _bits(e2))
    assert np.array_equal(_bits(v1), _bits(v2)) and np.array_equal(_bits(g1), _bits(g2))
    # what the definition promises: monotone per channel, inside [slo, shi]
    rs = r[:, ~flat]
    order = np.argsort(d["f"][:, ~flat], axis=0, kind="stable")
    assert (np.diff(np.take_along_axis(rs, order, axis=0), axis=0) >= -1e-6 * (1.0 + np.abs(rs).max())).all(), what
    slo, shi = d["s_lo_hi"][~flat, 0].astype(np.float64), d["s_lo_hi"][~flat, 1].astype(np.float64)
    span = np.maximum(np.abs(slo), np.abs(shi))
    assert (rs >= slo - 4 * U * span).all() and (rs <= shi + 4 * U * span).all(), what
    return worst, float((err / tol_g).max()), abs(d["val"] - v_ref) / max(v_ref, 1e-30)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PIECE_SHAPES)
def test_pieces_vs_the_reference(eng, shape, kind):
    d = _pieces(eng, shape, kind)
    worst, g, v = _check_pieces(d, shape, f"{shape} {kind}")
    report(f"hist pieces C={shape[0]} N={shape[1]} Ns={shape[2]} B={shape[3]} {kind}: tables {worst:.2f} ulp, gradient "
           f"{g:.2f} of its bound, value rel {v:.1e}")


@pytest.mark.parametrize("skind", ["flat-style-only", "flat-image-only"])
def test_a_flat_channel_on_one_side_only(eng, skind):
    """Channel 3 flat in the style and live in the image: start = end = slo, the remap is that constant.  Flat in the image and
    live in the style: no counts, value and gradient 0.  (Flat on both sides: every case of test_pieces_vs_the_reference.)"""
    shape = (64, 96, 40, 16)
    d = _pieces(eng, shape, "signed", skind)
    _check_pieces(d, shape, skind)
    if skind == "flat-style-only":
        live = d["counts"][3] > 0
        assert live.any() and (d["ends"][3][live] == np.float32(0.75)).all()
        r, _, _ = hist_ref.remap(d["f"], d["lo_hi"], d["ends"], 16)
        assert (r[:, 3] == 0.75).all()
    else:
        assert not d["counts"][3].any() and not d["grad"][:, 3].any()


def test_a_map_remapped_onto_its_own_histogram_comes_back(eng):
    """The device's tables of a map against itself: |R(v) - v| <= u (4 (hi - lo) + 2 max(|lo|, |hi|)), u = 2^-24
    (tests/test_hist_host.py derives the bound), and hist is below its square."""
    f = make_map("relu", 1000, 64, seed=5)
    fd = dev(torch.from_numpy(f))
    lo_hi, counts = eng.histogram_counts(fd, 256)
    ends = eng.histogram_table(lo_hi, counts, 1000, lo_hi, counts, 1000)
    val, grad = eng.histogram_term(fd, lo_hi, ends, 1.0)
    lh = lo_hi.cpu().numpy().astype(np.float64)
    bound = U * (4.0 * (lh[:, 1] - lh[:, 0]) + 2.0 * np.abs(lh).max(axis=1))
    back = np.abs(grad.cpu().numpy().astype(np.float64))                   # coef 1: the gradient is F - R
    assert (back <= bound[None, :] * 1.01).all(), float((back / np.maximum(bound[None, :], 1e-300)).max())
    assert float(val.cpu()) <= float(bound.max()) ** 2


def test_stand_alone_pieces_refuse_what_they_cannot_read(eng):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import _ptr, _stream
    f = dev(torch.from_numpy(make_map("relu", 24, 64, seed=1)))
    lo_hi, counts = eng.histogram_counts(f, 16)
    s = _stream(eng.device)
    lib, ctx = eng.lib, eng.ctx
    for c in (32, 96, 1024):                         # C not one of 64, 128, 256, 512
        assert lib.nst_histogram_counts(ctx, _ptr(f), 4, c, 16, _ptr(lo_hi), _ptr(counts), s) == -1
    for bins in (1, 0, 1025):
        assert lib.nst_histogram_counts(ctx, _ptr(f), 24, 64, bins, _ptr(lo_hi), _ptr(counts), s) == -1
    assert lib.nst_histogram_counts(ctx, _ptr(f), 0, 64, 16, _ptr(lo_hi), _ptr(counts), s) == -1
    assert lib.nst_histogram_counts(ctx, None, 24, 64, 16, _ptr(lo_hi), _ptr(counts), s) == -1
    ends = eng.histogram_table(lo_hi, counts, 24, lo_hi, counts, 24)
    assert lib.nst_histogram_term(ctx, _ptr(f), 24, 64, 16, _ptr(lo_hi), _ptr(ends), 1.0, None, None, s) == -1
    assert lib.nst_histogram_term(ctx, _ptr(f), 24, 64, 16, _ptr(lo_hi), _ptr(ends), float("nan"), None, _ptr(f.clone()), s) == -1
    with pytest.raises(NstError):
        eng.histogram_counts(f.double(), 16)
    with pytest.raises(NstError):
        eng.histogram_table(lo_hi, counts.long(), 24, lo_hi, counts, 24)
    with pytest.raises(ValueError):
        eng.histogram_counts(f, 1)


# ---- 2. the closure against the oracle, the term evaluated on the device's own map --------------------------------------------
def device_map(e, level, i):
    """(N, C) float32: map index i of a level as the last closure left it (NHWC rows)."""
    a = e.level_activation(level, TAP_LAYER[i]).cpu()
    return a.squeeze(0).permute(1, 2, 0).reshape(-1, a.shape[1]).contiguous().numpy()


def reference_on_the_device_map(e, level, i, w_i, bins):
    """(hist_i, dF as a (1,C,h,w) float32 tensor, N) by tests/hist_ref.py from the device's map and the device's tables - which
    are themselves held to the reference's from the same map and the style's record: counts exactly, ends to 1 ulp."""
    f = device_map(e, level, i)
    n, c = f.shape
    lo_hi, counts, ends = (t.cpu().numpy() for t in e.histogram_tables(level, i))
    s_lo_hi, s_counts = (t.cpu().numpy() for t in e.histogram_style(level, i))
    r_lo_hi, r_counts = hist_ref.range_counts(f, bins)
    assert np.array_equal(lo_hi, r_lo_hi) and np.array_equal(counts.astype(np.int64), r_counts), (level, i)
    ns = int(s_counts[s_lo_hi[:, 1] != s_lo_hi[:, 0]].sum(axis=1).max())
    assert (s_counts.sum(axis=1) == np.where(s_lo_hi[:, 1] != s_lo_hi[:, 0], ns, 0)).all()
    r_ends = hist_ref.tables(r_counts, n, s_lo_hi, s_counts.astype(np.int64), ns, bins)
    assert float(_ulps(ends, r_ends).max()) <= 1.0, (level, i)
    hist, d_f = hist_ref.term(f, lo_hi, ends, bins, coef=2.0 * w_i / (c * n))
    a = e.level_activation(level, TAP_LAYER[i])
    h, w = a.shape[-2:]
    return hist, torch.from_numpy(d_f.astype(np.float32).reshape(h, w, c)).permute(2, 0, 1).unsqueeze(0).contiguous(), n


class PatchedOracle:
    """cpu_ref.level_loss with the term as the DEVICE's map gives it: per (level, map) the constant hist_i and the linear form
    <dF, F_oracle> - <dF, F_oracle>.detach(), so that the level total gains sum_i w_i hist_i (ascending map order, fp32) and
    its gradient dF carried back through the oracle's network under the decisions it is given.  cpu_ref.LevelTargets only
    numbers the levels (the order the targets are made in).  The term is in EVERY weighting of a closure - its weights are
    its own, as on the device.  `log` keeps, per level_loss call, (weighted term, {map: hist_i})."""

    def __init__(self, monkeypatch, w, levels=None):
        self.w, self.levels = tuple(w), levels
        self.level_loss0, self.targets0 = cpu_ref.level_loss, cpu_ref.LevelTargets
        self.given, self.log, self.made = {}, [], 0
        monkeypatch.setattr(cpu_ref, "level_loss", self.level_loss)
        monkeypatch.setattr(cpu_ref, "LevelTargets", self.targets)

    def targets(self, content_t, style_t, weights):
        tg = self.targets0(content_t, style_t, weights)
        tg.hist_level = self.made
        self.made += 1
        return tg

    def term(self, feats, l):
        if l not in self.given:
            return None, {}
        total, vals = None, {}
        for i in sorted(self.given[l]):
            hist, d_f = self.given[l][i]
            lin = (d_f * feats[i]).sum()
            t = torch.tensor(np.float32(self.w[i])) * torch.tensor(np.float32(hist)) + (lin - lin.detach())
            vals[i] = hist
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
        term, vals = self.term(seen[0], tg.hist_level)
        self.log.append((float(term.detach()) if term is not None else 0.0, vals))
        return (total + term if term is not None else total), content, style, tv


NO_TV = TERMS[:3]
TV_ONLY = TERMS[3:]
BINS = 256
# relu1_1 and relu4_1, Risser's layers.  Measured under the patched oracle on the CPU with the reference on the device's maps
# (profiles/r23_hist.txt): on the 64x96 two-level job at 256 bins hist is 10.26 / 9.87 on relu1_1 and 0.81 / 1.44 on relu4_1, and
# these weights put the term at 31.7 % / 31.5 % of the level totals (4.5e4 / 5.4e4) on both walkers; 30.6 % at 16 bins on level 0
# alone, 31.8 % / 26.7 % under average pooling, 46.6 % / 42.0 % beside the centred Gram and the moment term, 25.8 % / 25.3 %
# beside the MRF term, 33.9 % / 31.4 % with the term on the content map, 23.2 % / 23.7 % on the top map of the chain, 37.8 % /
# 34.4 % in luminance mode, and W_15 (the signed conv5_1) at 43.7 % / 37.3 %.  Every path reports its shares and holds them
# between 10 % and 60 %
W_14 = (1000.0, 0.0, 0.0, 5000.0, 0.0, 0.0)
W_15 = (1000.0, 0.0, 0.0, 0.0, 0.0, 5000.0)


def _set_histograms(e, styles, w, bins=BINS, levels=None, prep=cpu_ref.prepare_img):
    for i in range(len(styles)):
        if levels is None or i in levels:
            e.set_histograms(i, dev(prep(styles[i])), w, bins)


def _setup(e, contents, styles, w, bins=BINS, levels=None, prepare=None):
    h, wd = contents[0].shape[:2]
    e.configure(len(contents), h, wd)
    if prepare:
        prepare(e)
    for i in range(len(contents)):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))
    _set_histograms(e, styles, w, bins, levels)


def _hand_over(e, xd, w, bins=BINS, what=""):
    """One closure, then per (level, weighted map) the reference's hist_i and dF from the device's map: hist_i against
    histogram_losses() to 1e-5."""
    e.closure(xd, CW, SW, TVW)
    losses = e.histogram_losses().cpu().numpy()
    given = {}
    for l in range(e.levels):
        if e.histograms_setting(l) is None:
            assert not losses[l].any()
            continue
        given[l] = {}
        for i in range(6):
            if not w[i] > 0:
                assert losses[l, i] == 0.0
                continue
            hist, d_f, n = reference_on_the_device_map(e, l, i, w[i], bins)
            report(f"hist {what} level {l} map {i} (N = {n}): device hist_i {losses[l, i]:.6e}, reference on the device's map "
                   f"{hist:.6e}, rel {abs(float(losses[l, i]) - hist) / hist:.1e}")
            assert losses[l, i] == pytest.approx(hist, rel=1e-5), (what, l, i)
            given[l][i] = (hist, d_f)
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
        report(f"hist {what} level {l}: term {term:.4e} of total {row[0]:.4e} = {share:.1%}; hist_i = {vals}")
        if vals:
            assert lo <= share <= hi, (what, l, share)


def _additivity(e, xt, what):
    """The term is in every weighting with its own weights, so the sum of the content, style and tv gradients holds it three
    times and the weighted sum once; the closure with cw = sw = tvw = 0 is the term alone (same forward pass, same tables):
    g(all) = g(content) + g(style) + g(tv) - 2 g(0, 0, 0), to hip_helpers' 2e-6."""
    xd = dev(xt)
    g = {name: e.closure(xd, *w3)[0].cpu().numpy().astype(np.float64) for name, w3 in TERMS + (("hist", (0.0, 0.0, 0.0)),)}
    s = g["content"] + g["style"] + g["tv"] - 2.0 * g["hist"]
    add = float(np.linalg.norm(g["all"] - s) / np.linalg.norm(s))
    share = float(np.linalg.norm(g["hist"]) / np.linalg.norm(g["all"]))
    report(f"hist {what}: |g(all) - (sum of the weightings - 2 g(term alone))| / |.| = {add:.1e}; |g(term alone)| / |g(all)| = {share:.2f}")
    assert add < 2e-6, (what, add)
    assert share > 0.01, (what, share)


def _strict(e, monkeypatch, vgg_weights, what, w, bins=BINS, levels=None, prepare=None, job="64x96_L1"):
    c, s, xt = _job(job)
    patched = PatchedOracle(monkeypatch, w, levels)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, w, bins, levels, prepare)
    patched.given = _hand_over(e, dev(xt), w, bins, what)
    cache = {}
    _the_term_counts(patched, xt, tg, vgg_weights, what, cache)
    # losses 1e-5, rows 2e-5, gradient 2e-5 under the device's decisions (hip_helpers' standing tolerances), additivity 2e-6
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"hist {what}", terms=NO_TV, own_cache=cache)
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"hist {what}", terms=TV_ONLY)
    _additivity(e, xt, what)
    return patched


def test_path_batched_walker(eng, vgg_weights, monkeypatch):
    _strict(eng, monkeypatch, vgg_weights, "batched walker", W_14)


def test_path_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _strict(eng_per_level, monkeypatch, vgg_weights, "per-level walker", W_14)


def test_path_one_level_of_two(eng, vgg_weights, monkeypatch):
    """hist_levels naming one level of two (the other level's row and gradient are what they are without the term), at 16 bins."""
    p = _strict(eng, monkeypatch, vgg_weights, "level 0 of two, 16 bins", W_14, bins=16, levels=(0,))
    assert eng.histograms_setting(1) is None and eng.histograms_setting(0) == (W_14, 16)
    assert not eng.histogram_losses().cpu().numpy()[1].any()
    assert p.log[-1][1] == {}


def test_path_average_pooling(eng, vgg_weights, monkeypatch):
    from test_hip_pooling import avg_vgg19_features
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "avg pooling", W_14, prepare=lambda e: e.set_pooling("avg"))
    finally:
        eng.reset_pooling()


def test_path_pre_relu_taps(eng, vgg_weights, monkeypatch):
    """A signed map: under use_relu=False conv5_1 is tapped before its ReLU (every other map feeds the next layer through
    its ReLU), so the term sits on map 5, the top of the chain, whose launch applies no mask.  4x6 and 2x3 pixels."""
    monkeypatch.setattr(cpu_ref, "vgg19_features", prerelu_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "pre-ReLU taps", W_15, prepare=lambda e: e.set_taps(4, [0, 1, 2, 3, 5], use_relu=False))
        assert float(eng.histogram_tables(0, 5)[0][:, 0].min().cpu()) < 0.0          # (the map is signed)
    finally:
        eng.reset_taps()


def test_path_beside_a_centred_gram_and_the_moment_term(eng, vgg_weights, monkeypatch):
    """The term's addend beside the Gram second source, its row bias (o S of the centred Gram) and the moment term's fold."""
    from test_hip_gram_shift import MEAN, PatchedGram
    from test_hip_moments import PatchedOracle as MomentOracle, on_maps as mom_maps
    monkeypatch.setattr(cpu_ref, "gram_matrix", PatchedGram((MEAN,) * 6))
    MomentOracle(monkeypatch, mom_maps(1e2), mom_maps(1e2))            # (patched first: the histogram oracle wraps it)

    def prepare(e):
        e.set_gram_shift("mean")
        e.set_moments(mom_maps(1e2), mom_maps(1e2))

    _strict(eng, monkeypatch, vgg_weights, "'mean' Gram + moments", W_14, prepare=prepare)


def _path_beside_the_mrf_term_on_the_same_map(e, vgg_weights, monkeypatch):
    from test_hip_mrf import EPS, PatchedOracle as MrfOracle, W_34
    c, s, xt = _job("64x96_L1")
    mrf = MrfOracle(monkeypatch, W_34)
    patched = PatchedOracle(monkeypatch, W_14)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, W_14)
    for i in range(2):
        e.set_patches(i, dev(cpu_ref.prepare_img(s[i])), W_34, 1, EPS)
    try:
        patched.given = _hand_over(e, dev(xt), W_14, BINS, "beside MRF")
        mrf.nn = {l: {i: e.patch_matches(l, i).cpu() for i in range(6) if W_34[i] > 0} for l in range(2)}
        cache = {}
        _the_term_counts(patched, xt, tg, vgg_weights, "beside MRF", cache)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "hist beside MRF", terms=NO_TV, own_cache=cache)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "hist beside MRF", terms=TV_ONLY)
    finally:
        e.clear_patches()


def test_path_beside_the_mrf_term_on_the_same_map(eng, vgg_weights, monkeypatch):
    """relu4_1 carries both terms: the MRF term's addend first, the histogram loss added to it.  The MRF oracle of
    tests/test_hip_mrf.py is patched first and handed the device's matches; the histogram oracle wraps it."""
    _path_beside_the_mrf_term_on_the_same_map(eng, vgg_weights, monkeypatch)


def test_path_beside_the_mrf_term_on_the_same_map_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    """The same on the per-level walker (the mid-chain site with two terms on one map), to the same bounds."""
    _path_beside_the_mrf_term_on_the_same_map(eng_per_level, vgg_weights, monkeypatch)


# -- taps beyond cpu_ref.level_loss: test_hip_style_blend's restatement with the term added
def _restated_closure(x, targets, weights, cw, sw, tvw, taps, decisions, w, given):
    import torch.nn.functional as F
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
        for i in sorted(given[l]):
            hist, d_f = given[l][i]
            lin = (d_f * f[i]).sum()
            t = torch.tensor(np.float32(w[i])) * torch.tensor(np.float32(hist)) + (lin - lin.detach())
            term = t if term is None else term + t
        t = cw * content + sw * style + tvw * tv + term
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
        terms.append(float(term.detach()))
    total.backward()
    return total.detach(), x.grad.detach(), rows, terms


OTHER_TAPS = ["content map carries the term", "term on the top map of the chain"]


def _path_other_taps(e, vgg_weights, case):
    from test_hip_style_blend import device_decisions as decisions_of, restated_targets
    if case.startswith("content"):
        taps, w = (4, (0, 1, 2, 3, 4, 5)), (1000.0, 0.0, 0.0, 0.0, 5000.0, 0.0)
    else:
        taps, w = (2, (0, 1, 2, 3)), W_14
    c, s, xt = _job("64x96_L1")
    prep = cpu_ref.prepare_img
    try:
        e.configure(2, 64, 96)
        e.set_taps(taps[0], list(taps[1]))
        tg = []
        for i in range(2):
            e.set_targets(i, dev(prep(c[i])), dev(prep(s[i])))
            tg.append(restated_targets(prep(c[i]), [prep(s[i])], ((1.0,) * 6,), vgg_weights, taps))
        _set_histograms(e, s, w)
        xd = dev(xt)
        given = _hand_over(e, xd, w, BINS, case)
        for name, (cw, sw, tvw) in (("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW))):
            grad, losses = e.closure(xd, cw, sw, tvw)
            dec = decisions_of(e, xd, vgg_weights, taps)
            losses = losses.cpu().numpy()
            loss, g_ref, rows, terms = _restated_closure(xt, tg, vgg_weights, cw, sw, tvw, taps, dec, w, given)
            e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
            e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
            shares = [t / r[0] for t, r in zip(terms, rows)]
            report(f"hist {case} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}; share of the level "
                   f"totals {[round(v, 3) for v in shares]}")
            if name == "all":
                assert all(0.10 <= v <= 0.60 for v in shares), (case, shares)
            assert e_l < 1e-5, (case, name, e_l)
            check_rows(losses[:-1].reshape(2, 4), np.array(rows), 2e-5, cw, sw, tvw)
            assert e_g < 2e-5, (case, name, e_g)
    finally:
        e.reset_taps()


@pytest.mark.parametrize("case", OTHER_TAPS)
def test_path_other_taps(eng, vgg_weights, case):
    """style_mask 0x3F with the term on conv4_2, the content map (content gradient and the term in one addend, beside the Gram
    second source); and style maps ending at relu4_1 with the term on it: the top-of-chain launch's addend."""
    _path_other_taps(eng, vgg_weights, case)


@pytest.mark.parametrize("case", OTHER_TAPS)
def test_path_other_taps_per_level_walker(eng_per_level, vgg_weights, case):
    """The same two cases on the per-level walker - its content-map and top-of-chain sites with the term on them - to the
    same bounds."""
    _path_other_taps(eng_per_level, vgg_weights, case)


def test_path_luminance(eng, vgg_weights, monkeypatch):
    """The luminance closure with the term = the patched oracle's closure at E(u), gradient summed over the channels; the
    style's record is that of the matched luminance plane."""
    from artstyletransfer_amd import host_image
    from test_hip_color import expand, lum_decisions, lum_targets, start_u
    c, s = _levels(64, 96, 2, 1), _levels(70, 110, 2, 2)
    w = W_14
    patched = PatchedOracle(monkeypatch, w)
    try:
        eng.configure(2, 64, 96)
        eng.set_color("luminance")
        alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
        cu, su = lum_targets(c, s, alpha, beta)
        for i in range(2):
            eng.set_targets(i, dev(torch.from_numpy(cu[i])), dev(torch.from_numpy(su[i])))
            eng.set_histograms(i, dev(torch.from_numpy(su[i])), w, BINS)
        tg = [cpu_ref.LevelTargets(expand(torch.from_numpy(a)), expand(torch.from_numpy(b)), vgg_weights) for a, b in zip(cu, su)]
        u = start_u(c[0])
        ud = dev(u.reshape(1, 1, 64, 96))
        xt = expand(u)
        patched.given = _hand_over(eng, ud, w, BINS, "luminance")
        grad, losses = eng.closure(ud, CW, SW, TVW)
        dec = lum_decisions(eng, ud)
        losses = losses.cpu().numpy()
        patched.log.clear()
        loss, _, rows = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW)
        shares = [m / r[0] for (m, _), r in zip(patched.log, rows)]
        report(f"hist luminance: share of the level totals {[round(v, 3) for v in shares]}")
        assert all(0.10 <= v <= 0.60 for v in shares), shares
        assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
        check_rows(losses[:-1].reshape(2, 4), np.array(rows), 1e-5, CW, SW, TVW)
        _, g_eq, _ = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_eq.sum(dim=1).numpy().reshape(64, 96))
        report(f"hist luminance: gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_g < 2e-5
    finally:
        eng.reset_color()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_other_arithmetic_modes_run_the_term(vgg_weights, mode):
    """The addend is the walkers' own and does not depend on the convolution arithmetic: one closure in each other mode, held
    by the value check (hist_i against the reference on the device's map, the tables against the reference's) and additivity."""
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt = _job("64x96_L1")
    e = StyleEngine(vgg_weights, 0, conv_mode=mode)
    try:
        _setup(e, c, s, W_14)
        _hand_over(e, dev(xt), W_14, BINS, mode)
        _additivity(e, xt, mode)
    finally:
        e.close()


# ---- 3. halves, reproducibility, L-BFGS, level masks ----------------------------------------------------------------------
MIXED_W = (1000.0, 0.0, 300.0, 5000.0, 0.0, 0.0)


def _mixed_job(e, name="64x96_L1"):
    c, s, xt = _job(name)
    _setup(e, c, s, MIXED_W)
    return dev(xt), c, s


def test_halves_equal_the_whole_and_run_to_run_bitwise(eng):
    x, _, _ = _mixed_job(eng)
    g, l = eng.closure(x, CW, SW, TVW)
    m = eng.histogram_losses()
    tb = [[t.clone() for t in eng.histogram_tables(lv, 3)] for lv in range(2)]
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    assert np.array_equal(_bits(m), _bits(eng.histogram_losses()))
    for lv in range(2):
        lo_hi, counts, ends = eng.histogram_tables(lv, 3)
        assert np.array_equal(_bits(lo_hi), _bits(tb[lv][0])) and torch.equal(counts, tb[lv][1]) and np.array_equal(_bits(ends), _bits(tb[lv][2]))
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_level_masks_add_up(eng, eng_per_level, which):
    e = eng if which == "batched" else eng_per_level
    x, _, _ = _mixed_job(e)
    g, l = e.closure(x, CW, SW, TVW)
    m = e.histogram_losses().cpu().numpy()
    g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    gs, ls, ms = np.zeros_like(g), np.zeros_like(l), np.zeros_like(m)
    for mask in (1, 2):
        gm, lm = e.closure_levels(x, CW, SW, TVW, mask)
        mm = e.histogram_losses().cpu().numpy()
        assert not mm[[lv for lv in range(2) if not (mask >> lv) & 1]].any()          # zeros for levels outside the mask
        gs += gm.cpu().numpy()
        ls += lm.cpu().numpy()
        ms += mm
    np.testing.assert_allclose(ls, l, rtol=1e-6)
    assert np.array_equal(ms, m)
    err = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
    report(f"hist level masks [{which}]: |sum - unsharded| / |.| = {err:.1e}")
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


# ---- 4. the loss row -----------------------------------------------------------------------------------------------------------
def test_histogram_losses_times_the_weights_plus_the_other_terms_are_the_row_totals(eng):
    """total = ((cw content + sw style) + tvw tv) + w_0 hist_0 + w_2 hist_2 ... in ascending map order, every product and sum
    rounded to fp32: bitwise from what the closure returns; and zeros for the maps without the term."""
    x, _, _ = _mixed_job(eng)
    _, l = eng.closure(x, CW, SW, TVW)
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    m = eng.histogram_losses().cpu().numpy()
    on = [i for i in range(6) if MIXED_W[i] > 0]
    assert m.shape == (2, 6) and not m[:, [1, 4, 5]].any() and (m[:, on] > 0).all()
    f32 = np.float32
    for lv in range(2):
        total = (f32(CW) * rows[lv, 1] + f32(SW) * rows[lv, 2]) + f32(TVW) * rows[lv, 3]
        for i in on:
            total = f32(total + f32(MIXED_W[i]) * m[lv, i])
        assert total == rows[lv, 0], (lv, total, rows[lv, 0])


# ---- 5. a cleared term ---------------------------------------------------------------------------------------------------------
def setter_bytes(w, bins):
    """What nst_level_set_histograms allocates: the six values, and per weighted map of C channels the style's and the image's
    range (2 C floats each) and counts (C B words each), the ends (2 C B floats) and HIST_VALUE_BLOCKS = 2048 double partials."""
    from artstyletransfer_amd.engine import TAP_CHANNELS
    return 6 * 4 + sum(4 * (4 * c + 4 * c * bins) + 8 * 2048 for c, wi in zip(TAP_CHANNELS, w) if wi > 0)


@pytest.mark.parametrize("batched", [True, False])
def test_cleared_term_is_bitwise_an_engine_that_never_called_the_setter(vgg_weights, batched):
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
                _set_histograms(e, s, MIXED_W)
                assert e.bytes() == before + 2 * setter_bytes(MIXED_W, BINS)
                e.closure(dev(xt), CW, SW, TVW)
                assert len(e.last_closure_launches()) > len(out[0][2])
                assert e.bytes() == before + 2 * setter_bytes(MIXED_W, BINS)        # a closure allocates nothing
                e.clear_histograms()
                assert e.bytes() == before
                assert all(e.histograms_setting(i) is None for i in range(2))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            assert not e.histogram_losses().cpu().numpy().any()
            out.append((_bits(g), _bits(l), e.last_closure_launches()))
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    strip = lambda rec: [{k: v for k, v in d.items() if k not in ("ms",)} for d in rec]        # noqa: E731
    assert strip(out[0][2]) == strip(out[1][2]) and len(out[0][2]) > 0


# ---- 6. life cycle and refusals --------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(eng, vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine, _ptr, _stream
    x, c, s = _mixed_job(eng)
    g0, l0 = eng.closure(x, CW, SW, TVW)
    before = [eng.histograms_setting(i) for i in range(2)]
    assert before[0] == (MIXED_W, BINS)
    style = dev(cpu_ref.prepare_img(s[0]))
    hs, ws = style.shape[-2:]

    def raw(level=0, w=MIXED_W, bins=BINS, img=style):
        return eng.lib.nst_level_set_histograms(eng.ctx, level, _ptr(img), hs, ws, (C.c_float * 6)(*w), bins, _stream(eng.device))

    # NST_E_ARG, and a refusal leaves the level as it was
    assert raw(level=-1) == -1 and raw(level=2) == -1
    for bad in (-1.0, float("nan"), float("inf")):
        assert raw(w=(0.0, 0.0, bad, 1.0, 0.0, 0.0)) == -1
    for bins in (1, 0, -4, 1025):
        assert raw(bins=bins) == -1
    assert raw(w=(0.0, 0.0, 0.0, 0.0, 1.0, 0.0)) == -1                 # conv4_2 is no style map under the default taps
    assert [eng.histograms_setting(i) for i in range(2)] == before
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # a guided level, in either order of the two calls
    planes = torch.ones((2, 64, 96), device="cuda:0") * 0.5
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_guidance(0, planes)
    eng.clear_histograms(0)
    eng.set_guidance(0, planes)
    assert raw() == -2 and eng.histograms_setting(0) is None
    eng.clear_guidance()
    # a pending backward half goes with a new term
    _mixed_job(eng)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_histograms(0, style, W_14)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure_backward(x, CW, SW, TVW)
    # configure, set_taps, set_pooling and set_color drop the term
    for drop, undo in ((lambda: eng.configure(2, 64, 96), None), (lambda: eng.set_taps(4, [0, 1, 2, 3]), eng.reset_taps),
                       (lambda: eng.set_pooling("avg"), eng.reset_pooling), (lambda: eng.set_color("luminance"), eng.reset_color)):
        _mixed_job(eng)
        assert eng.histograms_setting(0) is not None
        drop()
        try:
            assert all(eng.histograms_setting(i) is None for i in range(2))
        finally:
            if undo:
                undo()
    # no configured job; the stripe closure; the stripe sharding of the optimiser before any stripe engine is made
    e1 = StyleEngine(vgg_weights, 0)
    try:
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        assert e1.lib.nst_level_set_histograms(e1.ctx, 0, _ptr(xs), 64, 96, (C.c_float * 6)(*W_14), BINS, _stream(e1.device)) == -2
        e1.configure(1, 64, 96)
        e1.set_targets(0, xs, xs)
        e1.set_histograms(0, xs, W_14)
        with pytest.raises(NstError, match=r"\(-2\)"):
            e1.window_begin(xs, 0, 64, 64)
        opt = PixelOptimizer(e1, "lbfgs")
        try:
            with pytest.raises(ValueError, match="hist_weight cannot be combined with stripe sharding"):
                opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
        finally:
            opt.close()
        # the readers name a level out of range the same way, and a map without the term
        assert e1.lib.nst_level_histograms(e1.ctx, 1, None, None) == -1
        assert e1.lib.nst_level_histogram_tables(e1.ctx, 1, 3, None, None, None, _stream(e1.device)) == -1
        assert e1.lib.nst_level_histogram_style(e1.ctx, 0, 6, None, None, _stream(e1.device)) == -1
        assert e1.lib.nst_level_histogram_tables(e1.ctx, 0, 1, None, None, None, _stream(e1.device)) == -2
        e1.clear_histograms()
        e1.window_begin(xs, 0, 64, 64)
    finally:
        e1.close()


def test_a_graph_context_refuses_the_term(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine, _ptr, _stream
    e = StyleEngine(vgg_weights, 0, use_graph=True)
    try:
        e.configure(1, 64, 96)
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        assert e.lib.nst_level_set_histograms(e.ctx, 0, _ptr(xs), 64, 96, (C.c_float * 6)(*W_14), BINS, _stream(e.device)) == -2
        e.clear_histograms()                                          # clearing is no setting
        assert e.histograms_setting(0) is None
    finally:
        e.close()


# ---- 7. a whole job ----------------------------------------------------------------------------------------------------------
def test_whole_job():
    """neural_style_transfer_hist on a 64x96 pair (one level) yields finite images that the term has moved; with
    hist_weight=None its yields are neural_style_transfer_mrf_semantic()'s, bitwise."""
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf_semantic
    from test_hip_mrf import _run_job
    out = _run_job(neural_style_transfer_hist, hist_weight=1000.0, hist_bins=64)
    assert len(out) == 3 and all(np.isfinite(o).all() for o in out)
    plain = _run_job(neural_style_transfer_mrf_semantic)
    off = _run_job(neural_style_transfer_hist, hist_weight=None, hist_bins=64)
    assert len(plain) == len(off) == 3
    assert all(np.array_equal(a, b) for a, b in zip(plain, off))
    assert not np.array_equal(plain[-1], out[-1])                  # (the term moved the result)
