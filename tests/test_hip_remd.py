"""GPU: the relaxed EMD style term (nst_level_set_remd; Kolkin, Salavon & Shakhnarovich 2019) - the sampled feature vectors of a
map matched both ways, by cosine, to those of the style's map.
1. the decisions of the match alone (nst_remd_match), both directions, against fp64, held to torch-fp32's own error of the same
   cosines;
2. ties and degenerate vectors, bitwise: the lowest index of equal scores in both directions, all-zero samples and maps;
3. value and gradient alone (nst_remd_term) against fp64 autograd of tests/remd_ref.py at the device's matches, for the decided
   side and with each side forced;
4. the closure under equal decisions - the device's matches and side handed to the oracle - against the oracle with
   cpu_ref.level_loss and cpu_ref.LevelTargets replaced by test-local ones that add the term (monkeypatch: no oracle edit), at
   hip_helpers' standing tolerances, over the paths the term's gradient takes;
5. closure halves, reproducibility, L-BFGS, level masks, the loss row, a cleared term; 6. life cycle and refusals;
7. a whole job."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import remd_ref
from hip_helpers import (CW, SW, TVW, TERMS, check_rows, closure_vs_oracle_under_equal_decisions, dev, levels as _levels,
                         oracle_targets, rel_l2, report)
from oracle import cpu_ref
from test_hip_gram_shift import _bits, _job, prerelu_vgg19_features
from test_hip_mrf import feature_like, nhwc

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


# ---- 1. decisions against fp64 ---------------------------------------------------------------------------------------------
# (C, h, w, hs, ws, si, ss)
SHAPES = [(64, 12, 13, 11, 9, 1, 1), (128, 9, 10, 14, 7, 2, 1), (256, 7, 33, 8, 19, 1, 2), (512, 5, 6, 6, 5, 1, 1), (64, 40, 37, 33, 45, 1, 1),
          (64, 1, 1, 1, 1, 1, 1), (512, 17, 19, 16, 21, 3, 2), (128, 33, 65, 5, 4, 1, 1), (256, 64, 48, 40, 70, 1, 1)]
SIDE_B = (SHAPES[1], SHAPES[4], SHAPES[6])          # fp64's active side is B on these, A on the others (checked on the CPU)
_CASES = {}


def _case(eng, shape):
    """(f, fs, fp64 cosines, device nnA, device nnB) of one shape, computed once."""
    if shape not in _CASES:
        c, h, w, hs, ws, si, ss = shape
        f, fs = feature_like(c, h, w, seed=c + h), feature_like(c, hs, ws, seed=c + hs + 100)
        cos64 = remd_ref.cosines(f.double(), fs.double(), si, ss)
        nna, nnb = eng.remd_match(nhwc(f), nhwc(fs), si, ss, EPS)
        _CASES[shape] = (f, fs, cos64, nna.cpu(), nnb.cpu())
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_match_decisions_vs_fp64(eng, shape):
    """For nnA and for nnB: the fp64 cosine of every device choice is within delta of the fp64 best, delta = 4 x the largest
    error of a torch-fp32 evaluation of the same cosines against fp64 on this input (measured here, never taken from the
    device); at most 1 % of the samples differ from the fp64 arg-max at all; indices in range, shapes right.

    Measured on the GPU (profiles/r24_remd.txt): no sample differs from the fp64 arg-max in either direction on any shape
    (delta 1.4e-8 ... 9.4e-7)."""
    c, h, w, hs, ws, si, ss = shape
    f, fs, cos64, nna, nnb = _case(eng, shape)
    cos32 = remd_ref.cosines(f, fs, si, ss).double()
    delta = 4.0 * float((cos32 - cos64).abs().max())
    n, m = cos64.shape
    assert (n, m) == (remd_ref.counts(h, w, si), remd_ref.counts(hs, ws, ss))
    assert tuple(nna.shape) == (n,) and tuple(nnb.shape) == (m,) and nna.dtype == torch.int32 and nnb.dtype == torch.int32
    arg_a, arg_b = remd_ref.matches(cos64)
    arg32_a, arg32_b = remd_ref.matches(cos32)
    for name, nn, table, arg, arg32, other in (("nnA", nna, cos64, arg_a, arg32_a, m), ("nnB", nnb, cos64.t(), arg_b, arg32_b, n)):
        idx = nn.long()
        assert int(idx.min()) >= 0 and int(idx.max()) < other, name
        best = table.max(dim=1).values
        chosen = table.gather(1, idx[:, None]).squeeze(1)
        differ = float((idx != arg).double().mean())
        report(f"remd match C={c} {h}x{w}/{si} vs {hs}x{ws}/{ss} {name}: n={n} m={m}, delta {delta:.2e}, worst shortfall "
               f"{float((best - chosen).max()):.2e}, samples off the fp64 arg-max {differ:.2%} (torch fp32: "
               f"{float((arg32 != arg).double().mean()):.2%})")
        assert bool((chosen >= best - delta).all()), (name, float((best - chosen).max()), delta)
        assert differ <= 0.01, (name, differ)


# ---- 2. ties and degenerate vectors, bitwise -------------------------------------------------------------------------------------
def test_ties_pick_the_lowest_index_in_both_directions(eng):
    """A style map tiled from a 4x5 block three times in each direction: style sample (a, b) repeats at (a + 4, b + 5), bitwise,
    so every image sample must pick the member (a % 4, b % 5) of its class.  An image map tiled likewise: every style sample
    picks the lowest i of its class.  An all-zero image sample picks style sample 0."""
    c = 64
    block = feature_like(c, 4, 5, seed=11)
    tiled = block.repeat(1, 1, 3, 3).contiguous()                    # 12 x 15
    other = feature_like(c, 9, 11, seed=12)
    other[:, :, 0, 0] = 0.0                                          # sample 0 is all zero
    nna, nnb = eng.remd_match(nhwc(other), nhwc(tiled), 1, 1, EPS)
    nna = nna.cpu().long()
    a, b = nna // 15, nna % 15
    assert bool((a < 4).all()) and bool((b < 5).all()), (a.max(), b.max())
    assert int(nna[0]) == 0
    arg = remd_ref.matches(remd_ref.cosines(other.double(), tiled.double()))[0]
    assert float((((arg // 15) % 4 == a) & ((arg % 15) % 5 == b)).double().mean()) >= 0.99
    # the other direction: the image is the tiled map
    nna2, nnb2 = eng.remd_match(nhwc(tiled), nhwc(other), 1, 1, EPS)
    nnb2 = nnb2.cpu().long()
    a, b = nnb2 // 15, nnb2 % 15
    assert bool((a < 4).all()) and bool((b < 5).all()), (a.max(), b.max())
    # (the all-zero style sample 0 scores +0 against everything: the lowest image sample)
    assert int(nnb2[0]) == 0
    # on a stride grid the period is seen through the stride: rows repeat every 2 samples (4 / 2), columns every 5
    nna3, _ = eng.remd_match(nhwc(other), nhwc(tiled), 1, 2, EPS)
    nna3 = nna3.cpu().long()
    nb = (15 - 1) // 2 + 1
    assert bool((nna3 // nb < 2).all()) and bool((nna3 % nb < 5).all())
    # run to run, bitwise
    again = eng.remd_match(nhwc(other), nhwc(tiled), 1, 1, EPS)
    assert torch.equal(again[0].cpu().long(), nna) and torch.equal(again[1].cpu(), nnb.cpu())
    val, side, grad = eng.remd_term(nhwc(other), nhwc(tiled), again[0], again[1])
    val2, side2, grad2 = eng.remd_term(nhwc(other), nhwc(tiled), again[0], again[1])
    assert side == side2 and np.array_equal(_bits(val), _bits(val2)) and np.array_equal(_bits(grad), _bits(grad2))


def test_all_zero_samples_and_maps(eng):
    """An all-zero image map: every score is +0, so nnA = 0 everywhere, every cosine is 0 and rA = rB = 1 exactly; an all-zero
    style map likewise; nothing is non-finite, gradients included."""
    c = 128
    f, z = feature_like(c, 5, 7, seed=3), torch.zeros((1, c, 4, 6))
    for img, sty in ((torch.zeros((1, c, 5, 7)), feature_like(c, 4, 6, seed=4)), (f, z), (torch.zeros((1, c, 5, 7)), z)):
        nna, nnb = eng.remd_match(nhwc(img), nhwc(sty), 1, 1, EPS)
        assert not nna.cpu().any() and not nnb.cpu().any()
        val, side, grad = eng.remd_term(nhwc(img), nhwc(sty), nna, nnb)
        assert val.cpu().tolist() == [1.0, 1.0, 1.0] and side == 0
        assert torch.isfinite(grad).all()


def test_stand_alone_pieces_refuse_what_they_cannot_read(eng):
    """The pieces take raw pointers: a view that is not contiguous, another dtype, another rank or unequal channel counts are
    refused before the call, as are matches of the wrong size or type, a stride outside 1..256 and a bad side."""
    from artstyletransfer_amd._lib import NstError
    f, fs = nhwc(feature_like(64, 6, 7, seed=1)), nhwc(feature_like(64, 5, 5, seed=2))
    nna = torch.zeros(42, dtype=torch.int32, device="cuda:0")
    nnb = torch.zeros(25, dtype=torch.int32, device="cuda:0")
    view = dev(feature_like(64, 6, 7, seed=1)).squeeze(0).permute(1, 2, 0)            # NHWC strides over CHW memory
    assert not view.is_contiguous()
    for bad_f, bad_fs in ((view, fs), (f, fs.double()), (f.unsqueeze(0), fs), (f, nhwc(feature_like(128, 5, 5, seed=2)))):
        with pytest.raises(NstError):
            eng.remd_match(bad_f, bad_fs)
        with pytest.raises(NstError):
            eng.remd_term(bad_f, bad_fs, nna, nnb)
    for bad in (nna.long(), nna[:41].contiguous(), nna.cpu()):
        with pytest.raises(NstError):
            eng.remd_term(f, fs, bad, nnb)
    with pytest.raises(NstError):
        eng.remd_term(f, fs, nna, nna)
    for bad in (0, 257, 1.5):
        with pytest.raises(ValueError):
            eng.remd_match(f, fs, si=bad)
        with pytest.raises(ValueError):
            eng.remd_match(f, fs, ss=bad)
    with pytest.raises(ValueError):
        eng.remd_term(f, fs, nna, nnb, side=2)
    with pytest.raises(ValueError):
        eng.remd_match(f, fs, epsilon=0.0)
    # a map of 96 channels is the library's to refuse
    g96 = torch.zeros((4, 4, 96), device="cuda:0")
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.remd_match(g96, g96)
    val, side, grad = eng.remd_term(f, fs, nna, nnb)
    assert torch.isfinite(val).all() and torch.isfinite(grad).all() and side in (0, 1)


# ---- 3. value and gradient alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_term_vs_fp64_autograd_at_the_device_matches(eng, shape):
    """remd, rA, rB and d remd / dF at the device's matches against fp64 autograd of the reference: for the decided side and
    with each side forced, the value's error and the gradient's rel-L2 are at most 4 x those of a torch-fp32 evaluation of the
    same expression on the same input; the gradient is exactly zero off the sample grid; the decided side is fp64's.

    Measured on the GPU (profiles/r24_remd.txt): value error 9.9e-10 ... 2.9e-8 (torch fp32 1.7e-9 ... 4.8e-8), gradient rel-L2
    5.0e-8 ... 9.3e-8 (torch fp32 6.4e-8 ... 1.7e-7)."""
    c, h, w, hs, ws, si, ss = shape
    f, fs, _, nna, nnb = _case(eng, shape)
    off = torch.ones((h, w), dtype=torch.bool)
    off[::si, ::si] = False
    want_side = 1 if shape in SIDE_B else 0
    for forced in (-1, 0, 1):
        out = {}
        for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
            x = f.to(dt).clone().requires_grad_(True)
            v, sd, rA, rB = remd_ref.value(x, fs.to(dt), nna, nnb, si, ss, side=forced if forced >= 0 else (want_side if name == "fp32" else -1))
            v.backward()
            out[name] = (float(v.detach()), x.grad.detach().double(), sd, float(rA.detach()), float(rB.detach()))
        v64, g64, sd64, rA64, rB64 = out["fp64"]
        val, side, grad = eng.remd_term(nhwc(f), nhwc(fs), dev(nna), dev(nnb), si, ss, EPS, side=forced, coef=1.0)
        val, grad = val.cpu().double().numpy(), grad.cpu().permute(2, 0, 1).unsqueeze(0).double()
        if forced < 0:
            assert sd64 == want_side, (shape, rA64, rB64)              # (the CPU fact behind SIDE_B)
        assert side == sd64, (shape, forced, side, rA64, rB64, val)
        v32, g32 = out["fp32"][0], out["fp32"][1]
        e_v, e_v32 = abs(val[0] - v64), abs(v32 - v64)
        e_r = max(abs(val[1] - rA64), abs(val[2] - rB64))
        e_r32 = max(abs(out["fp32"][3] - rA64), abs(out["fp32"][4] - rB64))
        e_g, e_g32 = rel_l2(grad.numpy(), g64.numpy()), rel_l2(g32.numpy(), g64.numpy())
        report(f"remd term C={c} {h}x{w}/{si} vs {hs}x{ws}/{ss} side {forced} -> {side} (rA {rA64:.6f}, rB {rB64:.6f}): value err device "
               f"{e_v:.2e} / torch fp32 {e_v32:.2e}; rA, rB err device {e_r:.2e} / torch fp32 {e_r32:.2e}; gradient rel-L2 device {e_g:.2e} "
               f"/ torch fp32 {e_g32:.2e}")
        assert e_v <= 4.0 * e_v32, (forced, e_v, e_v32)
        assert e_r <= 4.0 * e_r32, (forced, e_r, e_r32)
        assert e_g <= 4.0 * e_g32, (forced, e_g, e_g32)
        assert not grad[0][:, off].any()
        assert val[0] == (val[2] if side else val[1])


# ---- 4. the closure under equal decisions ------------------------------------------------------------------------------------
class PatchedOracle:
    """cpu_ref.level_loss and cpu_ref.LevelTargets with the term at FIXED matches and a FIXED side: LevelTargets gains the
    style's maps and its level number (the order the targets are made in), level_loss calls the original, adds sum_i w_i remd_i
    (ascending map order) to the total of a level with the term and returns the same four-entry row.  `given[level][map]`:
    the device's (nnA, nnB, side), which the test hands over before the first evaluation; `strides[level]`: (image strides,
    style strides) or None.  The term is in EVERY weighting of a closure - its weights are its own, as on the device.  `log`
    keeps, per level_loss call, (weighted term, {map: remd_i})."""

    def __init__(self, monkeypatch, w, strides):
        self.w, self.strides = tuple(w), strides
        self.level_loss0, self.targets0 = cpu_ref.level_loss, cpu_ref.LevelTargets
        self.given, self.log, self.made = {}, [], 0
        monkeypatch.setattr(cpu_ref, "level_loss", self.level_loss)
        monkeypatch.setattr(cpu_ref, "LevelTargets", self.targets)

    def targets(self, content_t, style_t, weights):
        tg = self.targets0(content_t, style_t, weights)
        with torch.no_grad():
            sf = cpu_ref.vgg19_features(style_t, weights)
            tg.remd_style = {i: sf[i].detach() for i in range(6) if self.w[i] > 0}
        tg.remd_level = self.made
        self.made += 1
        return tg

    def term(self, feats, tg):
        l = tg.remd_level
        if self.strides[l] is None:
            return None, {}
        total, vals = None, {}
        for i in range(6):
            if not self.w[i] > 0:
                continue
            nna, nnb, side = self.given[l][i]
            v = remd_ref.value(feats[i], tg.remd_style[i], nna, nnb, self.strides[l][0][i], self.strides[l][1][i], side=side)[0]
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

# relu3_1 and relu4_1.  Measured on the CPU (the oracle and tests/remd_ref.py, the tests' synthetic weights): on the 64x96
# two-level job the level totals are 3.1e4 / 3.7e4 and remd is 0.082 / 0.136 on relu3_1 and 0.106 / 0.097 on relu4_1 at strides
# (1, 1), so these weights put the term at about 30 % of the level totals; fp64's active side there is B on relu3_1 and A on
# relu4_1, on both levels
W_23 = (0.0, 0.0, 7e4, 7e4, 0.0, 0.0)
ONES = (1,) * 6


def _strides(levels_num, si=ONES, ss=ONES, levels=None):
    return [(tuple(si), tuple(ss)) if levels is None or l in levels else None for l in range(levels_num)]


def _set_remd(e, styles, w, strides, prep=cpu_ref.prepare_img):
    for i in range(len(styles)):
        if strides[i] is not None:
            e.set_remd(i, dev(prep(styles[i])), w, strides[i][0], strides[i][1], EPS)


def _setup(e, contents, styles, w, strides, prepare=None):
    h, wd = contents[0].shape[:2]
    e.configure(len(contents), h, wd)
    if prepare:
        prepare(e)
    for i in range(len(contents)):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))
    _set_remd(e, styles, w, strides)


def _matches_of(e, w, what=""):
    given = {}
    for l in range(e.levels):
        if e.remd_setting(l) is None:
            continue
        given[l] = {}
        for i in range(6):
            if w[i] > 0:
                nna, nnb, side = e.remd_matches(l, i)
                given[l][i] = (nna.cpu(), nnb.cpu(), side)
                report(f"remd {what} level {l} map {i}: n={nna.numel()} m={nnb.numel()} active side {'AB'[side]}")
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
        report(f"remd {what} level {l}: term {term:.4e} of total {row[0]:.4e} = {share:.1%}; remd_i = {vals}")
        if vals:
            assert lo <= share <= hi, (what, l, share)


def _additivity(e, xt, what):
    """The term is in every weighting with its own weights, so the sum of the content, style and tv gradients holds it three
    times and the weighted sum once; the closure with cw = sw = tvw = 0 is the term alone (same forward pass, same matches):
    g(all) = g(content) + g(style) + g(tv) - 2 g(0, 0, 0), to hip_helpers' 2e-6."""
    xd = dev(xt)
    g = {name: e.closure(xd, *w3)[0].cpu().numpy().astype(np.float64) for name, w3 in TERMS + (("remd", (0.0, 0.0, 0.0)),)}
    s = g["content"] + g["style"] + g["tv"] - 2.0 * g["remd"]
    add = float(np.linalg.norm(g["all"] - s) / np.linalg.norm(s))
    share = float(np.linalg.norm(g["remd"]) / np.linalg.norm(g["all"]))
    report(f"remd {what}: |g(all) - (sum of the weightings - 2 g(term alone))| / |.| = {add:.1e}; |g(term alone)| / |g(all)| = {share:.2f}")
    assert add < 2e-6, (what, add)
    assert share > 0.01, (what, share)


def _strict(e, monkeypatch, vgg_weights, what, w, strides=None, prepare=None, job="64x96_L1"):
    c, s, xt = _job(job)
    strides = strides or _strides(len(c))
    patched = PatchedOracle(monkeypatch, w, strides)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, w, strides, prepare)
    e.closure(dev(xt), CW, SW, TVW)
    patched.given = _matches_of(e, w, what)
    cache = {}
    _the_term_counts(patched, xt, tg, vgg_weights, what, cache)
    # losses 1e-5, rows 2e-5, gradient 2e-5 under the device's decisions (hip_helpers' standing tolerances), additivity 2e-6
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"remd {what}", terms=NO_TV, own_cache=cache)
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"remd {what}", terms=TV_ONLY)
    _additivity(e, xt, what)
    return patched


def _both_sides_were_active(patched):
    """Across the (level, map) pairs of a path each side is the active one at least once: on this job fp64 has side B on
    relu3_1 (rA 0.0796 / rB 0.0821 on level 0) and side A on relu4_1 (0.1059 / 0.1051), so both gradients are exercised."""
    sides = {side for per_map in patched.given.values() for _, _, side in per_map.values()}
    assert sides == {0, 1}, patched.given.keys()
    assert all(per_map[2][2] == 1 and per_map[3][2] == 0 for per_map in patched.given.values())


def test_path_batched_walker(eng, vgg_weights, monkeypatch):
    _both_sides_were_active(_strict(eng, monkeypatch, vgg_weights, "batched walker", W_23))


def test_path_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _both_sides_were_active(_strict(eng_per_level, monkeypatch, vgg_weights, "per-level walker", W_23))


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_strides_two_and_three_and_one_level_of_two(eng, eng_per_level, vgg_weights, monkeypatch, which):
    """Strides (2, 3) on every map, on level 0 of two (the other level's row and gradient are what they are without the term)."""
    e = eng if which == "batched" else eng_per_level
    strides = _strides(2, (2,) * 6, (3,) * 6, levels=(0,))
    p = _strict(e, monkeypatch, vgg_weights, f"level 0 of two, strides (2, 3) [{which}]", W_23, strides)
    assert e.remd_setting(1) is None and e.remd_setting(0)[:4] == (W_23, (2,) * 6, (3,) * 6, EPS)
    assert not e.remd_losses().cpu().numpy()[1].any()
    assert p.log[-1][1] == {}
    nna, nnb, _ = e.remd_matches(0, 2)
    assert nna.numel() == remd_ref.counts(16, 24, 2) and nnb.numel() == remd_ref.counts(70 >> 2, 110 >> 2, 3)


def test_path_average_pooling(eng, vgg_weights, monkeypatch):
    from test_hip_pooling import avg_vgg19_features
    monkeypatch.setattr(cpu_ref, "vgg19_features", avg_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "avg pooling", W_23, prepare=lambda e: e.set_pooling("avg"))
    finally:
        eng.reset_pooling()


# relu5_1 is 4x6 and 2x3 pixels: a term of a few samples.  Under use_relu=False it is conv5_1 before its ReLU - a signed map at
# the top of the chain, whose launch applies no mask.  Measured on the CPU as above: remd is 0.061 / 0.034 there, so these
# weights put the term at about 27 % of the level totals
W_25 = (0.0, 0.0, 7e4, 0.0, 0.0, 1e5)


def test_path_pre_relu_taps(eng, vgg_weights, monkeypatch):
    monkeypatch.setattr(cpu_ref, "vgg19_features", prerelu_vgg19_features)
    try:
        _strict(eng, monkeypatch, vgg_weights, "pre-ReLU taps", W_25, prepare=lambda e: e.set_taps(4, [0, 1, 2, 3, 5], use_relu=False))
        assert float(eng.level_activation(0, 12).min().cpu()) < 0.0          # (the map is signed)
    finally:
        eng.reset_taps()


def _path_beside_the_mrf_and_the_histogram_terms_on_the_same_map(e, vgg_weights, monkeypatch):
    import test_hip_hist as th
    from test_hip_mrf import PatchedOracle as MrfOracle, W_34
    c, s, xt = _job("64x96_L1")
    w_hist = (0.0, 0.0, 0.0, 5000.0, 0.0, 0.0)
    mrf = MrfOracle(monkeypatch, W_34)
    hist = th.PatchedOracle(monkeypatch, w_hist)
    strides = _strides(2)
    patched = PatchedOracle(monkeypatch, W_23, strides)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, W_23, strides)
    for i in range(2):
        e.set_patches(i, dev(cpu_ref.prepare_img(s[i])), W_34, 1, EPS)
    th._set_histograms(e, s, w_hist)
    try:
        hist.given = th._hand_over(e, dev(xt), w_hist, th.BINS, "beside remd")
        mrf.nn = {l: {i: e.patch_matches(l, i).cpu() for i in range(6) if W_34[i] > 0} for l in range(2)}
        patched.given = _matches_of(e, W_23, "beside MRF and hist")
        cache = {}
        _the_term_counts(patched, xt, tg, vgg_weights, "beside MRF and hist", cache, lo=0.05)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "remd beside MRF and hist", terms=NO_TV, own_cache=cache)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, "remd beside MRF and hist", terms=TV_ONLY)
    finally:
        e.clear_patches()
        e.clear_histograms()


def test_path_beside_the_mrf_and_the_histogram_terms_on_the_same_map(eng, vgg_weights, monkeypatch):
    """relu4_1 carries all three terms: the MRF term's addend first, the histogram loss added to it, then this term.  The
    oracles of tests/test_hip_mrf.py and tests/test_hip_hist.py are patched first and handed the device's decisions; this
    one wraps them, as the loss row adds the term last."""
    _path_beside_the_mrf_and_the_histogram_terms_on_the_same_map(eng, vgg_weights, monkeypatch)


def test_path_beside_the_mrf_and_the_histogram_terms_on_the_same_map_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    """The same on the per-level walker (the mid-chain site with all three terms on one map), to the same bounds."""
    _path_beside_the_mrf_and_the_histogram_terms_on_the_same_map(eng_per_level, vgg_weights, monkeypatch)


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
                nna, nnb, side = given[l][i]
                t = torch.tensor(np.float32(w[i])) * remd_ref.value(f[i], tg.remd_style[i], nna, nnb, side=side)[0]
                term = t if term is None else term + t
        t = cw * content + sw * style + tvw * tv + term
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
        terms.append(float(term.detach()))
    total.backward()
    return total.detach(), x.grad.detach(), rows, terms


OTHER_TAPS = ["content map is a weighted map", "weighted map at the top of the chain"]


def _path_other_taps(e, vgg_weights, case):
    from test_hip_style_blend import device_decisions as decisions_of, restated_targets
    if case.startswith("content"):
        taps, w = (4, (0, 1, 2, 3, 4, 5)), (0.0, 0.0, 7e4, 0.0, 7e4, 0.0)
    else:
        taps, w = (2, (0, 1, 2, 3)), W_23
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
                sf = cpu_ref.vgg19_features(prep(s[i]), vgg_weights)
            t.remd_style = {k: sf[k].detach() for k in range(6) if w[k] > 0}
            tg.append(t)
        _set_remd(e, s, w, _strides(2))
        xd = dev(xt)
        for name, (cw, sw, tvw) in (("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW))):
            grad, losses = e.closure(xd, cw, sw, tvw)
            dec = decisions_of(e, xd, vgg_weights, taps)
            given = _matches_of(e, w, case)
            losses = losses.cpu().numpy()
            loss, g_ref, rows, terms = _restated_closure(xt, tg, vgg_weights, cw, sw, tvw, taps, dec, w, given)
            e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
            e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
            shares = [t / r[0] for t, r in zip(terms, rows)]
            report(f"remd {case} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}; share of the level "
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
    style's maps are those of the matched luminance plane."""
    from artstyletransfer_amd import host_image
    from test_hip_color import expand, lum_decisions, lum_targets, start_u
    c, s = _levels(64, 96, 2, 1), _levels(70, 110, 2, 2)
    w = W_23
    patched = PatchedOracle(monkeypatch, w, _strides(2))
    try:
        eng.configure(2, 64, 96)
        eng.set_color("luminance")
        alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
        cu, su = lum_targets(c, s, alpha, beta)
        for i in range(2):
            eng.set_targets(i, dev(torch.from_numpy(cu[i])), dev(torch.from_numpy(su[i])))
            eng.set_remd(i, dev(torch.from_numpy(su[i])), w, 1, 1, EPS)
        tg = [cpu_ref.LevelTargets(expand(torch.from_numpy(a)), expand(torch.from_numpy(b)), vgg_weights) for a, b in zip(cu, su)]
        u = start_u(c[0])
        ud = dev(u.reshape(1, 1, 64, 96))
        xt = expand(u)
        grad, losses = eng.closure(ud, CW, SW, TVW)
        patched.given = _matches_of(eng, w, "luminance")
        dec = lum_decisions(eng, ud)
        losses = losses.cpu().numpy()
        patched.log.clear()
        loss, _, rows = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW)
        shares = [m / r[0] for (m, _), r in zip(patched.log, rows)]
        report(f"remd luminance: share of the level totals {[round(v, 3) for v in shares]}")
        assert all(0.10 <= v <= 0.60 for v in shares), shares
        assert float(losses[-1]) == pytest.approx(float(loss), rel=1e-5)
        check_rows(losses[:-1].reshape(2, 4), np.array(rows), 1e-5, CW, SW, TVW)
        _, g_eq, _ = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_eq.sum(dim=1).numpy().reshape(64, 96))
        report(f"remd luminance: gradient rel-L2 under equal decisions {e_g:.2e}")
        assert e_g < 2e-5
    finally:
        eng.reset_color()


# ---- 5. halves, reproducibility, L-BFGS, level masks, the loss row, a cleared term ----------------------------------------------
MIXED_W = (0.0, 3e4, 7e4, 7e4, 0.0, 0.0)
MIXED_SI, MIXED_SS = (1, 2, 1, 1, 1, 1), (1, 3, 2, 1, 1, 1)


def _mixed_job(e, name="64x96_L1"):
    c, s, xt = _job(name)
    _setup(e, c, s, MIXED_W, _strides(len(c), MIXED_SI, MIXED_SS))
    return dev(xt), c, s


def test_halves_equal_the_whole_and_run_to_run_bitwise(eng):
    x, _, _ = _mixed_job(eng)
    g, l = eng.closure(x, CW, SW, TVW)
    m = eng.remd_losses()
    nn = [eng.remd_matches(lv, 2) for lv in range(2)]
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    assert np.array_equal(_bits(m), _bits(eng.remd_losses()))
    for lv, (a, b, sd) in enumerate(nn):
        a2, b2, sd2 = eng.remd_matches(lv, 2)
        assert torch.equal(a, a2) and torch.equal(b, b2) and sd == sd2
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_level_masks_add_up(eng, eng_per_level, which):
    e = eng if which == "batched" else eng_per_level
    x, _, _ = _mixed_job(e)
    g, l = e.closure(x, CW, SW, TVW)
    m = e.remd_losses().cpu().numpy()
    g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    gs, ls, ms = np.zeros_like(g), np.zeros_like(l), np.zeros_like(m)
    for mask in (1, 2):
        gm, lm = e.closure_levels(x, CW, SW, TVW, mask)
        mm = e.remd_losses().cpu().numpy()
        assert not mm[[lv for lv in range(2) if not (mask >> lv) & 1]].any()          # zeros for levels outside the mask
        gs += gm.cpu().numpy()
        ls += lm.cpu().numpy()
        ms += mm
    np.testing.assert_allclose(ls, l, rtol=1e-6)
    assert np.array_equal(ms, m)
    err = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
    report(f"remd level masks [{which}]: |sum - unsharded| / |.| = {err:.1e}")
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


def test_remd_losses_times_the_weights_plus_the_other_terms_are_the_row_totals(eng):
    """total = ((cw content + sw style) + tvw tv) + w_1 remd_1 + w_2 remd_2 ... in ascending map order, every product and sum
    rounded to fp32: bitwise from what the closure returns; and zeros for the maps without the term."""
    x, _, _ = _mixed_job(eng)
    _, l = eng.closure(x, CW, SW, TVW)
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    m = eng.remd_losses().cpu().numpy()
    on = [i for i in range(6) if MIXED_W[i] > 0]
    assert m.shape == (2, 6) and not m[:, [0, 4, 5]].any() and (m[:, on] > 0).all()
    f32 = np.float32
    for lv in range(2):
        total = (f32(CW) * rows[lv, 1] + f32(SW) * rows[lv, 2]) + f32(TVW) * rows[lv, 3]
        for i in on:
            total = f32(total + f32(MIXED_W[i]) * m[lv, i])
        assert total == rows[lv, 0], (lv, total, rows[lv, 0])


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
                _set_remd(e, s, MIXED_W, _strides(2, MIXED_SI, MIXED_SS))
                assert e.bytes() > before
                e.closure(dev(xt), CW, SW, TVW)
                e.clear_remd()
                assert e.bytes() == before
                assert all(e.remd_setting(i) is None for i in range(2))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            assert not e.remd_losses().cpu().numpy().any()
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
    before = [eng.remd_setting(i) for i in range(2)]
    assert before[0] == (MIXED_W, MIXED_SI, MIXED_SS, EPS, (70, 110)) and before[1][4] == (35, 55)
    style = dev(cpu_ref.prepare_img(s[0]))
    hs, ws = style.shape[-2:]
    i6 = lambda v: (C.c_int * 6)(*v)                                    # noqa: E731

    def raw(level=0, w=MIXED_W, si=MIXED_SI, ss=MIXED_SS, eps=1e-5, img=style, e=eng):
        return e.lib.nst_level_set_remd(e.ctx, level, _ptr(img), hs, ws, (C.c_float * 6)(*w), i6(si), i6(ss), eps, _stream(e.device))

    # NST_E_ARG, and a refusal leaves the level as it was
    assert raw(level=-1) == -1 and raw(level=2) == -1
    for bad in (-1.0, float("nan"), float("inf")):
        assert raw(w=(0.0, 0.0, bad, 1.0, 0.0, 0.0)) == -1
    for eps in (0.0, -1e-5, float("nan"), float("inf")):
        assert raw(eps=eps) == -1
    for bad in (0, 257, -1):
        assert raw(si=(1, 1, bad, 1, 1, 1)) == -1 and raw(ss=(1, 1, 1, 1, 1, bad)) == -1
    assert raw(w=(0.0, 0.0, 0.0, 0.0, 1.0, 0.0)) == -1                 # conv4_2 is no style map under the default taps
    assert [eng.remd_setting(i) for i in range(2)] == before
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # a guided level, in either order of the two calls
    planes = torch.ones((2, 64, 96), device="cuda:0") * 0.5
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_guidance(0, planes)
    eng.clear_remd(0)
    eng.set_guidance(0, planes)
    assert raw() == -2 and eng.remd_setting(0) is None
    eng.clear_guidance()
    # a pending backward half goes with a new term
    _mixed_job(eng)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_remd(0, style, W_23)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure_backward(x, CW, SW, TVW)
    # configure, set_taps, set_pooling and set_color drop the term, and the bytes come back
    for drop, undo in ((lambda: eng.configure(2, 64, 96), None), (lambda: eng.set_taps(4, [0, 1, 2, 3]), eng.reset_taps),
                       (lambda: eng.set_pooling("avg"), eng.reset_pooling), (lambda: eng.set_color("luminance"), eng.reset_color)):
        _mixed_job(eng)
        assert eng.remd_setting(0) is not None
        drop()
        try:
            assert all(eng.remd_setting(i) is None for i in range(2))
        finally:
            if undo:
                undo()
    # the stripe closure, and the stripe sharding of the optimiser before any stripe engine is made
    e1 = StyleEngine(vgg_weights, 0)
    try:
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        assert e1.lib.nst_level_set_remd(e1.ctx, 0, _ptr(xs), 64, 96, (C.c_float * 6)(*W_23), i6(ONES), i6(ONES), 1e-5, _stream(e1.device)) == -2
        e1.configure(1, 64, 96)
        e1.set_targets(0, xs, xs)
        before = e1.bytes()
        e1.set_remd(0, xs, W_23)
        assert e1.bytes() > before
        with pytest.raises(NstError, match=r"\(-2\)"):
            e1.window_begin(xs, 0, 64, 64)
        opt = PixelOptimizer(e1, "lbfgs")
        try:
            with pytest.raises(ValueError, match="remd_weight cannot be combined with stripe sharding"):
                opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
        finally:
            opt.close()
        # the readers name a level out of range the same way, and a map without the term
        assert e1.lib.nst_level_remd(e1.ctx, 1, None, None, None, None, None, None) == -1
        assert e1.lib.nst_level_remd_matches(e1.ctx, 1, 3, _ptr(xs), None, None, _stream(e1.device)) == -1
        assert e1.lib.nst_level_remd_matches(e1.ctx, 0, 0, _ptr(xs), None, None, _stream(e1.device)) == -2
        e1.clear_remd()
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
        assert e.lib.nst_level_set_remd(e.ctx, 0, _ptr(xs), 64, 96, (C.c_float * 6)(*W_23), ones, ones, 1e-5, _stream(e.device)) == -2
        e.clear_remd()                                             # clearing is no setting
        assert e.remd_setting(0) is None
    finally:
        e.close()


# ---- 7. a whole job ----------------------------------------------------------------------------------------------------------
def _run_job(fn, seed=1, **kw):
    import neural_style_transfer as nst
    content = cpu_ref.synthetic_image(64, 96, seed=seed)
    style = cpu_ref.synthetic_image(70, 110, seed=seed + 1)
    pair = nst.ContentStylePair(("c", content), ("s", style))
    np.random.seed(1234)

    async def run():
        return [img async for _, img in fn(pair, CW, SW, TVW, "lbfgs", "vgg19", "content+noise", 30, 1, 0.95, (9, 18, 36, -1, 0),
                                           (0.3, 0.2, 0.1, 0.2, 0.2), (0.2, 0.3, 0.4, 0.1, 0.0), (0.2, 0.3, 0.4, 0.6, 0.3),
                                           device=torch.device("cuda", 0), **kw)]
    return asyncio.run(run()), style


def test_whole_job(eng, vgg_weights):
    """neural_style_transfer_remd on a 64x96 pair (one level, which the driver resizes to a short edge of 256), L-BFGS steps
    until 30 closures have run: finite images, and the remd values of the result - read with the stand-alone pieces on the result's own maps
    against the maps of the job's style level image - are lower than those of the same job run without the term.  With
    remd_weight=None it is neural_style_transfer_hist(), bitwise."""
    from artstyletransfer_amd import host_image, remd_modes
    from artstyletransfer_amd.histogram_loss import neural_style_transfer_hist
    from artstyletransfer_amd.remd_loss import neural_style_transfer_remd
    samples = 1024
    out, style = _run_job(neural_style_transfer_remd, remd_weight=1e5, remd_samples=samples)
    assert len(out) >= 1 and all(np.isfinite(o).all() for o in out)
    plain, _ = _run_job(neural_style_transfer_hist)
    off, _ = _run_job(neural_style_transfer_remd, remd_weight=None, remd_samples=samples)
    assert len(plain) == len(off) >= 1
    assert all(np.array_equal(a, b) for a, b in zip(plain, off))
    sh, sw = host_image.level_size(style.shape[0], style.shape[1], 0)
    style_level = eng.resize(dev(torch.from_numpy(style)), sh, sw).cpu().numpy()
    with torch.no_grad():
        fs = cpu_ref.vgg19_features(cpu_ref.prepare_img(style_level), vgg_weights)

        def remd_of(img):
            f = cpu_ref.vgg19_features(cpu_ref.prepare_img(np.ascontiguousarray(img, dtype=np.float32)), vgg_weights)
            vals = []
            for i in remd_modes.DEFAULT_MAPS:
                si = remd_modes.stride_for(f[i].shape[2], f[i].shape[3], samples)
                ss = remd_modes.stride_for(fs[i].shape[2], fs[i].shape[3], samples)
                a, b = nhwc(f[i]), nhwc(fs[i])
                nna, nnb = eng.remd_match(a, b, si, ss, EPS)
                vals.append(float(eng.remd_term(a, b, nna, nnb, si, ss, EPS, want_grad=False)[0][0].cpu()))
            return vals
        with_term, without = remd_of(out[-1]), remd_of(plain[-1])
    report(f"remd whole job: remd of relu2_1, relu3_1, relu4_1 with the term {with_term}, without {without}")
    assert all(a < b for a, b in zip(with_term, without)), (with_term, without)
