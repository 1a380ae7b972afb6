"""GPU: the long-range style term, xcorr (nst_level_set_xcorr; Berger & Memisevic 2017) - Gram matrices of a map against its
spatially shifted copy.
1. the statistic alone (nst_xcorr) against fp64, per 32 x 32 block, row, column and whole matrix, held to torch-fp32's own error;
2. exact cases, bitwise: row ends, split boundaries, an all-zero map, the style itself, repeated and interleaved calls;
3. value and gradient alone (nst_xcorr_term) against fp64 autograd of tests/xcorr_ref.py;
4. the closure against the oracle with cpu_ref.level_loss and cpu_ref.LevelTargets replaced by test-local ones that add the term
   (monkeypatch: no oracle edit), at hip_helpers' standing tolerances, over the paths the term's gradient takes;
5. closure halves, reproducibility, L-BFGS, level masks, the loss row, a cleared term; 6. life cycle and refusals;
7. a whole job."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import xcorr_ref
from hip_helpers import (CW, SW, TVW, TERMS, check_rows, closure_vs_oracle_under_equal_decisions, dev, oracle_targets, rel_l2, report)
from local_accuracy import FACTOR, FLOOR, MAX_FACTOR, assert_locally_as_accurate
from oracle import cpu_ref
from test_hip_gram_shift import _bits, _job
from test_hip_mrf import feature_like, nhwc

pytestmark = pytest.mark.gpu


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


# ---- 1. the statistic against fp64 ---------------------------------------------------------------------------------------------
# (C, h, w, shifts).  The first six: a pair count below one chunk of 32; one pair column or pair row left; shifts of 8 and 32,
# which cross a lane's staging group of 8 pixels and a chunk; many splits with row ends inside chunks.  The last two: T = 2 and
# T = 4 tiles a side, off-diagonal tile pairs in both orders.
SHAPES = [(64, 12, 13, ((1, 0), (5, 0), (12, 0), (0, 11))),
          (128, 9, 10, ((1, 0), (8, 0), (9, 0), (0, 8))),
          (256, 7, 33, ((1, 0), (32, 0), (0, 6))),
          (512, 5, 6, ((1, 0), (0, 4), (3, 2))),
          (128, 40, 37, ((3, 0), (17, 0), (36, 0), (0, 39), (5, 7))),
          (64, 33, 65, ((2, 0), (64, 0), (0, 32))),
          (256, 64, 48, ((7, 0), (0, 7))),
          (512, 17, 19, ((2, 0), (0, 9)))]
_CASES = {}


def _case(eng, k):
    """(f, the device's stack, its geometry, the fp64 stack, the torch-fp32 stack) of shape k, computed once; both references
    on the CPU from the same fp32 input."""
    if k not in _CASES:
        c, h, w, shifts = SHAPES[k]
        f = feature_like(c, h, w, seed=c + h)
        got, geo = eng.xcorr(nhwc(f), shifts, want_geometry=True)
        _CASES[k] = (f, got.cpu(), geo, xcorr_ref.matrices(f.double(), shifts), xcorr_ref.matrices(f, shifts))
    return _CASES[k]


def _stats(got, ref):
    """family -> (largest class error, where): errors normalised by the rms of the whole fp64 matrix; classes: every 32 x 32
    block (one MFMA accumulator), every row, every column; and the whole matrix."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    c = ref.shape[0]
    scale = float(np.sqrt(np.mean(ref * ref)))
    assert scale > 0 and np.isfinite(scale)
    sq = (got - ref) ** 2
    errs = {"blocks": np.sqrt(sq.reshape(c // 32, 32, c // 32, 32).mean(axis=(1, 3))) / scale, "rows": np.sqrt(sq.mean(axis=1)) / scale,
            "columns": np.sqrt(sq.mean(axis=0)) / scale}
    out = {"matrix": (float(np.sqrt(sq.mean())) / scale, None)}
    for fam, e in errs.items():
        i = np.unravel_index(int(np.argmax(e)), e.shape)
        out[fam] = (float(e[i]), tuple(int(v) for v in i))
    return out


def _held(got, ref64, ref32, what, factor=FACTOR, floor=FLOOR):
    """local_accuracy's standing rule: every statistic of the device's matrix is at most max(factor x torch-fp32's, floor)."""
    assert factor <= MAX_FACTOR
    d, t = _stats(got, ref64), _stats(ref32, ref64)
    bad, parts = [], []
    for fam in ("matrix", "blocks", "rows", "columns"):
        parts.append(f"{fam} {d[fam][0]:.2e} / {t[fam][0]:.2e} = " + (f"{d[fam][0] / t[fam][0]:.2f}x" if t[fam][0] > 0 else "-") +
                     ("" if d[fam][1] is None else f" @{d[fam][1]}"))
        if not d[fam][0] <= max(factor * t[fam][0], floor):
            bad.append((fam, d[fam], t[fam][0]))
    report(f"xcorr local {what}: device / torch-fp32 vs fp64 - " + ", ".join(parts))
    assert not bad, (what, bad)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_matrices_vs_fp64(eng, k):
    """Every G_d of every shape, per 32 x 32 block, row, column and whole matrix, within max(4 x torch-fp32's error, 5e-7) of
    fp64; the reported geometry is the split rule's: whole chunks of 32 pairs, all pairs covered."""
    c, h, w, shifts = SHAPES[k]
    f, got, geo, g64, g32 = _case(eng, k)
    assert tuple(got.shape) == (len(shifts), c, c) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    for j, (dx, dy) in enumerate(shifts):
        nsplit, pps = geo[j]
        npairs = (h - dy) * w - dx
        assert nsplit >= 1 and pps % 32 == 0 and (nsplit - 1) * pps < npairs <= nsplit * pps, (shifts[j], geo[j], npairs)
        _held(got[j].numpy(), g64[j].numpy(), g32[j].numpy(), f"C={c} {h}x{w} d=({dx},{dy}) nsplit={nsplit} pps={pps}")
    if k == 0:
        assert (h - 11) * w < 32                                      # (a pair count below one chunk)
    if k in (4, 5):
        assert max(g[0] for g in geo) >= 8, geo                         # (many splits)


# ---- 2. exact cases, bitwise ------------------------------------------------------------------------------------------------
def _one_hot_map(c, h, w, entries):
    """(1,c,h,w) zeros with f[ch, y, x] = v for (y, x, ch, v) in entries"""
    f = torch.zeros((1, c, h, w), dtype=torch.float32)
    for y, x, ch, v in entries:
        f[0, ch, y, x] = v
    return f


def _exact(f, d):
    """The exact G_d of a map whose entries are powers of two and whose G_d entries each hold at most one product: fp32(a b / Z)."""
    dx, dy = d
    _, c, h, w = f.shape
    a = f[0, :, dy:, dx:].reshape(c, -1).double()
    b = f[0, :, :h - dy, :w - dx].reshape(c, -1).double()
    assert int(((a != 0).double() @ (b != 0).double().t()).max()) <= 1
    return (a @ b.t()).float().numpy() / np.float32(c * (h - dy) * (w - dx))


@pytest.mark.parametrize("shape", [(64, 5, 7), (128, 4, 9), (256, 3, 5)])
def test_row_ends_are_not_paired_with_the_next_row(eng, shape):
    """One-hot vectors of power-of-two height at (y, w-1) and (y+1, 0): G_(1,0) is exactly zero.  At (y, x) and (y, x+1): the one
    entry fp32(a b / Z) at [channel of the right pixel][channel of the left pixel], and transposed when the roles swap."""
    c, h, w = shape
    a, b, ca, cb = 0.125, 32.0, 3, c - 2
    f = _one_hot_map(c, h, w, [(1, w - 1, ca, a), (2, 0, cb, b)])
    g = eng.xcorr(nhwc(f), [(1, 0)]).cpu().numpy()
    assert not g.any()
    for left, right in (((ca, a), (cb, b)), ((cb, b), (ca, a))):
        f = _one_hot_map(c, h, w, [(1, 2, left[0], left[1]), (1, 3, right[0], right[1])])
        g = eng.xcorr(nhwc(f), [(1, 0)]).cpu().numpy()[0]
        want = np.zeros((c, c), np.float32)
        want[right[0], left[0]] = np.float32(a * b) / np.float32(c * h * (w - 1))
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (shape, np.argwhere(g != want)[:4])
        assert np.array_equal(g, _exact(f, (1, 0)))
    # the same at the last pair column and across rows with a (w-1, 1) shift: (y, 0) pairs with (y+1, w-1) and nothing else
    f = _one_hot_map(c, h, w, [(0, 0, ca, a), (1, w - 1, cb, b), (1, 0, ca + 1, 2.0), (0, w - 1, cb - 1, 4.0)])
    g = eng.xcorr(nhwc(f), [(w - 1, 1)]).cpu().numpy()[0]
    assert np.array_equal(g, _exact(f, (w - 1, 1))) and np.count_nonzero(g) == 1 and g[cb, ca] != 0


@pytest.mark.parametrize("k", [4, 5])
def test_pairs_across_every_split_boundary(eng, k):
    """With the geometry the device reports: for every shift and every split boundary b a pair (p, p + d) with p < b <= p + d -
    the shifted operand of a split's last pixels lies in the next split - each on channels of its own, gives its one exact
    entry."""
    c, h, w, shifts = SHAPES[k]
    _, _, geo, _, _ = _case(eng, k)
    straddled = 0
    for (dx, dy), (nsplit, pps) in zip(shifts, geo):
        off = dy * w + dx
        pairs = []
        for s in range(1, nsplit):
            b = s * pps
            p = b - 1
            while p % w >= w - dx:            # (the last pixel before the boundary that has a partner in its row)
                p -= 1
            if p + off >= b:
                pairs.append((p, p + off))
        straddled += len(pairs)
        assert len(pairs) >= (nsplit - 1) * 3 // 4, ((dx, dy), len(pairs), nsplit)
        group = c // 2
        for g0 in range(0, len(pairs), group):
            entries = []
            for j, (p, q) in enumerate(pairs[g0:g0 + group]):
                entries.append((p // w, p % w, 2 * j, 2.0 ** (j % 5 - 2)))
                entries.append((q // w, q % w, 2 * j + 1, 2.0 ** (3 - j % 7)))
            f = _one_hot_map(c, h, w, entries)
            got = eng.xcorr(nhwc(f), [(dx, dy)]).cpu().numpy()[0]
            want = _exact(f, (dx, dy))
            for j in range(len(entries) // 2):
                assert want[2 * j + 1, 2 * j] != 0
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ((dx, dy), g0, np.argwhere(got != want)[:4])
    report(f"xcorr split boundaries C={c} {h}x{w}: {straddled} straddling pairs, geometry {geo}")


def test_all_zero_map(eng):
    for c, h, w in ((64, 6, 7), (256, 9, 5)):
        f = torch.zeros((1, c, h, w))
        sh = [(1, 0), (0, 2), (2, 1)]
        g = eng.xcorr(nhwc(f), sh)
        assert not g.cpu().numpy().any()
        val, grad = eng.xcorr_term(nhwc(f), g, sh, coef=3.0)
        assert float(val.cpu()) == 0.0 and not grad.cpu().numpy().any()
        gt = xcorr_ref.matrices(feature_like(c, h, w, seed=5), sh)
        val, grad = eng.xcorr_term(nhwc(f), dev(gt), sh, coef=3.0)
        assert float(val.cpu()) == pytest.approx(float(xcorr_ref.value(f.double(), gt.double(), sh)), rel=1e-6)
        assert bool(torch.isfinite(grad).all()) and not grad.cpu().numpy().any()      # (dF is linear in F)


@pytest.mark.parametrize("k", [0, 3, 4, 6])
def test_the_style_itself_gives_exactly_zero(eng, k):
    c, h, w, shifts = SHAPES[k]
    f = nhwc(_case(eng, k)[0])
    val, grad = eng.xcorr_term(f, eng.xcorr(f, shifts), shifts, coef=1e6)
    assert float(val.cpu()) == 0.0 and not grad.cpu().numpy().any()


def test_two_calls_give_equal_bits_and_shapes_do_not_leak(eng):
    first = {}
    for rnd in range(2):
        for k in (1, 6, 0, 7):
            c, h, w, shifts = SHAPES[k]
            f = _case(eng, k)[0]
            gt = dev(xcorr_ref.matrices(feature_like(c, h, w, seed=99), shifts))
            g = eng.xcorr(nhwc(f), shifts)
            val, grad = eng.xcorr_term(nhwc(f), gt, shifts, coef=2.0)
            bits = (_bits(g), _bits(val), _bits(grad))
            if rnd == 0:
                first[k] = bits
                assert np.array_equal(bits[0], _bits(_case(eng, k)[1]))
            else:
                assert all(np.array_equal(a, b) for a, b in zip(bits, first[k])), k


# ---- 3. value and gradient alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 3, 4, 6])
def test_term_vs_fp64_autograd(eng, k):
    """eng.xcorr_term against fp64 autograd of coef x xcorr_ref.value, the gradient held per row, column, channel group and
    block by assert_locally_as_accurate at the standing factor and floor.  The targets come from a differently seeded map, so
    G - Gt is of the size of G and no cancellation sets the error."""
    c, h, w, shifts = SHAPES[k]
    f = _case(eng, k)[0]
    gt = xcorr_ref.matrices(feature_like(c, h + 1, w + 2, seed=1000 + k), shifts)
    coef = 1e4
    out = {}
    for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        x = f.to(dt).clone().requires_grad_(True)
        v = xcorr_ref.value(x, gt.to(dt), shifts)
        (coef * v).backward()
        out[name] = (float(v.detach()), x.grad.detach())
    val, grad = eng.xcorr_term(nhwc(f), dev(gt), shifts, coef=coef)
    val, grad = float(val.cpu()), grad.cpu().permute(2, 0, 1).unsqueeze(0)
    v64, v32 = out["fp64"][0], out["fp32"][0]
    e_v, e_v32 = abs(val - v64) / v64, abs(v32 - v64) / v64
    report(f"xcorr term C={c} {h}x{w} |D|={len(shifts)}: value {v64:.6e}, rel err device {e_v:.2e} / torch fp32 {e_v32:.2e}")
    assert e_v <= max(FACTOR * e_v32, FLOOR), (e_v, e_v32)
    assert torch.allclose(out["fp64"][1], xcorr_ref.gradient(f.double(), gt.double(), shifts, coef), rtol=1e-10, atol=1e-16)
    assert_locally_as_accurate(grad, out["fp64"][1], out["fp32"][1], f"xcorr gradient C={c} {h}x{w}")


@pytest.mark.parametrize("c", [64, 128])
def test_border_pixels_take_one_term_only(eng, c):
    """A map with a single nonzero pixel q0 and the shift (2, 0): dF is nonzero at q0 - d and q0 + d only, where those lie in
    the map - at x < dx and at x >= w - dx one term only."""
    h, w, sh = 5, 9, ((2, 0),)
    gt = xcorr_ref.matrices(feature_like(c, h, w, seed=7), sh)
    for x0, cols in ((0, {2}), (1, {3}), (4, {2, 6}), (7, {5}), (8, {6})):
        f = torch.zeros((1, c, h, w))
        f[0, :, 3, x0] = feature_like(c, 1, 1, seed=8)[0, :, 0, 0] + 1.0
        _, grad = eng.xcorr_term(nhwc(f), dev(gt), sh, coef=1.0)
        grad = grad.cpu().permute(2, 0, 1).unsqueeze(0)
        want = xcorr_ref.gradient(f.double(), gt.double(), sh)
        on = {int(x) for x in torch.nonzero(grad[0].abs().sum(dim=(0, 1)))[:, 0]}
        assert on == cols and not grad[0, :, [0, 1, 2, 4]].any(), (x0, on)
        assert rel_l2(grad.numpy(), want.numpy()) < 1e-6


def test_stand_alone_pieces_refuse_what_they_cannot_read(eng):
    from artstyletransfer_amd._lib import NstError
    f = nhwc(feature_like(64, 6, 7, seed=1))
    for bad in ([(7, 0)], [(0, 6)], [(3, 0), (9, 1)]):
        with pytest.raises(ValueError, match="not smaller"):
            eng.xcorr(f, bad)
    with pytest.raises(ValueError, match="xcorr_shifts"):
        eng.xcorr(f, [(0, 0)])
    with pytest.raises(NstError):
        eng.xcorr(nhwc(feature_like(96, 6, 7, seed=1)), [(1, 0)])          # C = 96
    with pytest.raises(NstError):
        eng.xcorr_term(f, dev(torch.zeros((2, 64, 64))), [(1, 0)])


# ---- 4. the closure against the patched oracle ---------------------------------------------------------------------------------
SHIFTS = ((1, 0), (0, 2), (3, 1))        # relu4_1 of the lower level of the 64x96 job is 4 x 6


class PatchedOracle:
    """cpu_ref.level_loss and cpu_ref.LevelTargets with the term: LevelTargets gains the style's G_d stacks and its level number
    (the order the targets are made in), level_loss calls the original, adds sum_i w_i xcorr_i (ascending map order) to the
    total of a level with the term and returns the same four-entry row.  The term has no decisions of its own.  It is in EVERY
    weighting of a closure - its weights are its own, as on the device.  `log` keeps, per level_loss call, (weighted term,
    {map: xcorr_i})."""

    def __init__(self, monkeypatch, w, shifts=SHIFTS, levels=None):
        self.w, self.shifts, self.levels = tuple(w), tuple(shifts), levels
        self.level_loss0, self.targets0 = cpu_ref.level_loss, cpu_ref.LevelTargets
        self.log, self.made = [], 0
        monkeypatch.setattr(cpu_ref, "level_loss", self.level_loss)
        monkeypatch.setattr(cpu_ref, "LevelTargets", self.targets)

    def targets(self, content_t, style_t, weights):
        tg = self.targets0(content_t, style_t, weights)
        with torch.no_grad():
            sf = cpu_ref.vgg19_features(style_t, weights)
            tg.xcorr_gt = {i: xcorr_ref.matrices(sf[i], self.shifts).detach() for i in range(6) if self.w[i] > 0}
        tg.xcorr_level = self.made
        self.made += 1
        return tg

    def term(self, feats, tg):
        if self.levels is not None and tg.xcorr_level not in self.levels:
            return None, {}
        total, vals = None, {}
        for i in range(6):
            if not self.w[i] > 0:
                continue
            v = xcorr_ref.value(feats[i], tg.xcorr_gt[i], self.shifts)
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
# Measured on the CPU (the oracle and tests/xcorr_ref.py, the tests' synthetic weights, SHIFTS): on the 64x96 two-level job the
# level totals are 3.1e4 / 3.7e4 and xcorr is 0.0247 / 0.0226 on relu2_1, 0.00235 / 0.00378 on relu3_1 and 9.9e-5 / 1.97e-4 on
# relu4_1, so these weights put the term at about a quarter of the level totals
W_12 = (0.0, 2e5, 2e6, 0.0, 0.0, 0.0)
W_3 = (0.0, 0.0, 0.0, 1e8, 0.0, 0.0)


def _set_xcorr(e, styles, w, shifts=SHIFTS, levels=None, prep=cpu_ref.prepare_img):
    for i in range(len(styles)):
        if levels is None or i in levels:
            e.set_xcorr(i, dev(prep(styles[i])), w, shifts)


def _setup(e, contents, styles, w, shifts=SHIFTS, levels=None, prepare=None):
    h, wd = contents[0].shape[:2]
    e.configure(len(contents), h, wd)
    if prepare:
        prepare(e)
    for i in range(len(contents)):
        e.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))
    _set_xcorr(e, styles, w, shifts, levels)


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
        report(f"xcorr {what} level {l}: term {term:.4e} of total {row[0]:.4e} = {share:.1%}; xcorr_i = {vals}")
        if vals:
            assert lo <= share <= hi, (what, l, share)
    return [v for _, v in patched.log]


def _additivity(e, xt, what):
    """The term is in every weighting with its own weights: g(all) = g(content) + g(style) + g(tv) - 2 g(0, 0, 0), to 2e-6."""
    xd = dev(xt)
    g = {name: e.closure(xd, *w3)[0].cpu().numpy().astype(np.float64) for name, w3 in TERMS + (("xcorr", (0.0, 0.0, 0.0)),)}
    s = g["content"] + g["style"] + g["tv"] - 2.0 * g["xcorr"]
    add = float(np.linalg.norm(g["all"] - s) / np.linalg.norm(s))
    share = float(np.linalg.norm(g["xcorr"]) / np.linalg.norm(g["all"]))
    report(f"xcorr {what}: |g(all) - (sum of the weightings - 2 g(term alone))| / |.| = {add:.1e}; |g(term alone)| / |g(all)| = {share:.2f}")
    assert add < 2e-6, (what, add)
    assert share > 0.01, (what, share)


def _values_agree(e, vals, w, what):
    """xcorr_losses() of the last closure against the oracle's values of the same image, to 2e-5."""
    m = e.xcorr_losses().cpu().numpy()
    for l, per_map in enumerate(vals):
        for i in range(6):
            if i in per_map:
                assert m[l, i] == pytest.approx(per_map[i], rel=2e-5), (what, l, i)
            else:
                assert m[l, i] == 0.0, (what, l, i)


def _strict(e, monkeypatch, vgg_weights, what, w, shifts=SHIFTS, levels=None, prepare=None, job="64x96_L1"):
    c, s, xt = _job(job)
    patched = PatchedOracle(monkeypatch, w, shifts, levels)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, w, shifts, levels, prepare)
    cache = {}
    vals = _the_term_counts(patched, xt, tg, vgg_weights, what, cache)
    # losses 1e-5, rows 2e-5, gradient 2e-5 under the device's decisions (hip_helpers' standing tolerances), additivity 2e-6
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"xcorr {what}", terms=NO_TV, own_cache=cache)
    closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"xcorr {what}", terms=TV_ONLY)
    _additivity(e, xt, what)
    e.closure(dev(xt), CW, SW, TVW)
    _values_agree(e, vals, w, what)
    return patched


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_the_weighted_map_in_the_middle_of_the_chain(eng, eng_per_level, vgg_weights, monkeypatch, which):
    """relu2_1 and relu3_1 under the default taps: the term's gradient joins the Gram addend of the launch below the map."""
    _strict(eng if which == "batched" else eng_per_level, monkeypatch, vgg_weights, f"mid-chain [{which}]", W_12)


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_one_level_of_two_and_the_default_axis_shifts(eng, eng_per_level, vgg_weights, monkeypatch, which):
    """The int form of the shifts, (2, 0) and (0, 2), on level 0 of two: the other level's row and gradient are what they are
    without the term."""
    e = eng if which == "batched" else eng_per_level
    p = _strict(e, monkeypatch, vgg_weights, f"level 0 of two, shifts [2] [{which}]", W_12, ((2, 0), (0, 2)), levels=(0,))
    assert e.xcorr_setting(1) is None and e.xcorr_setting(0) == (W_12, ((2, 0), (0, 2)), (70, 110))
    assert p.log[-1][1] == {}
    assert tuple(e.xcorr_matrices(0, 2).shape) == (2, 256, 256)


def _path_beside_another_term_on_the_same_map(e, vgg_weights, monkeypatch, other):
    """relu4_1 carries the other term and this one: the other's addend first, this term's gradient added to it.  The other
    term's oracle is patched first and handed the device's decisions; this one wraps it, as the loss row adds the term last."""
    c, s, xt = _job("64x96_L1")
    if other == "remd":
        import test_hip_remd as tr
        inner = tr.PatchedOracle(monkeypatch, tr.W_23, tr._strides(2))
    else:
        import test_hip_hist as th
        w_hist = (0.0, 0.0, 0.0, 5000.0, 0.0, 0.0)
        inner = th.PatchedOracle(monkeypatch, w_hist)
    patched = PatchedOracle(monkeypatch, W_3)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, W_3)
    try:
        if other == "remd":
            tr._set_remd(e, s, tr.W_23, tr._strides(2))
            e.closure(dev(xt), CW, SW, TVW)
            inner.given = tr._matches_of(e, tr.W_23, "beside xcorr")
        else:
            th._set_histograms(e, s, w_hist)
            inner.given = th._hand_over(e, dev(xt), w_hist, th.BINS, "beside xcorr")
        cache = {}
        vals = _the_term_counts(patched, xt, tg, vgg_weights, f"beside {other}", cache, lo=0.05)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"xcorr beside {other}", terms=NO_TV, own_cache=cache)
        closure_vs_oracle_under_equal_decisions(e, xt, tg, vgg_weights, f"xcorr beside {other}", terms=TV_ONLY)
        _values_agree(e, vals, W_3, f"beside {other}")
    finally:
        e.clear_remd()
        e.clear_histograms()


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_on_a_map_that_also_carries_the_relaxed_emd_term(eng, eng_per_level, vgg_weights, monkeypatch, which):
    _path_beside_another_term_on_the_same_map(eng if which == "batched" else eng_per_level, vgg_weights, monkeypatch, "remd")


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_on_a_map_that_also_carries_the_histogram_loss(eng, eng_per_level, vgg_weights, monkeypatch, which):
    _path_beside_another_term_on_the_same_map(eng if which == "batched" else eng_per_level, vgg_weights, monkeypatch, "hist")


# -- taps beyond cpu_ref.level_loss: test_hip_style_blend's restatement with the term added
def _restated_closure(x, targets, weights, cw, sw, tvw, taps, decisions, w, shifts):
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
                t = torch.tensor(np.float32(w[i])) * xcorr_ref.value(f[i], tg.xcorr_gt[i], shifts)
                term = t if term is None else term + t
        t = cw * content + sw * style + tvw * tv + term
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
        terms.append(float(term.detach()))
    total.backward()
    return total.detach(), x.grad.detach(), rows, terms


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_path_the_weighted_map_at_the_top_of_the_chain(eng, eng_per_level, vgg_weights, which):
    """Style maps ending at relu4_1 (content on relu3_1) with the term on relu4_1: the top-of-chain launch's addend."""
    from test_hip_style_blend import device_decisions as decisions_of, restated_targets
    e = eng if which == "batched" else eng_per_level
    taps, w = (2, (0, 1, 2, 3)), W_3
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
            t.xcorr_gt = {k: xcorr_ref.matrices(sf[k], SHIFTS).detach() for k in range(6) if w[k] > 0}
            tg.append(t)
        _set_xcorr(e, s, w)
        xd = dev(xt)
        for name, (cw, sw, tvw) in (("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW))):
            grad, losses = e.closure(xd, cw, sw, tvw)
            dec = decisions_of(e, xd, vgg_weights, taps)
            losses = losses.cpu().numpy()
            loss, g_ref, rows, terms = _restated_closure(xt, tg, vgg_weights, cw, sw, tvw, taps, dec, w, SHIFTS)
            e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
            e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
            shares = [t / r[0] for t, r in zip(terms, rows)]
            report(f"xcorr top of the chain [{which}, {name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}; "
                   f"share of the level totals {[round(v, 3) for v in shares]}")
            if name == "all":
                assert all(0.10 <= v <= 0.60 for v in shares), shares
            assert e_l < 1e-5, (name, e_l)
            check_rows(losses[:-1].reshape(2, 4), np.array(rows), 2e-5, cw, sw, tvw)
            assert e_g < 2e-5, (name, e_g)
    finally:
        e.reset_taps()


# ---- 5. halves, reproducibility, L-BFGS, level masks, the loss row, a cleared term ----------------------------------------------
MIXED_W = (0.0, 2e5, 2e6, 1e8, 0.0, 0.0)


def _mixed_job(e, name="64x96_L1"):
    c, s, xt = _job(name)
    _setup(e, c, s, MIXED_W)
    return dev(xt), c, s


def test_halves_equal_the_whole_and_run_to_run_bitwise(eng):
    x, _, _ = _mixed_job(eng)
    g, l = eng.closure(x, CW, SW, TVW)
    m = eng.xcorr_losses()
    mats = [eng.xcorr_matrices(lv, 2) for lv in range(2)]
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    assert np.array_equal(_bits(m), _bits(eng.xcorr_losses()))
    for lv in range(2):
        assert np.array_equal(_bits(mats[lv]), _bits(eng.xcorr_matrices(lv, 2))) and mats[lv].cpu().numpy().any()
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))
    # the G_d stack of the closure is the stand-alone statistic of the level's own map (relu3_1 = conv layer 4 after its ReLU)
    for lv in range(2):
        own = eng.xcorr(nhwc(eng.level_activation(lv, 4).cpu()), SHIFTS)
        assert rel_l2(mats[lv].cpu().numpy(), own.cpu().numpy()) < 1e-6, lv


@pytest.mark.parametrize("which", ["batched", "per_level"])
def test_level_masks_add_up(eng, eng_per_level, which):
    e = eng if which == "batched" else eng_per_level
    x, _, _ = _mixed_job(e)
    g, l = e.closure(x, CW, SW, TVW)
    m = e.xcorr_losses().cpu().numpy()
    g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
    gs, ls, ms = np.zeros_like(g), np.zeros_like(l), np.zeros_like(m)
    for mask in (1, 2):
        gm, lm = e.closure_levels(x, CW, SW, TVW, mask)
        mm = e.xcorr_losses().cpu().numpy()
        assert not mm[[lv for lv in range(2) if not (mask >> lv) & 1]].any()          # zeros for levels outside the mask
        gs += gm.cpu().numpy()
        ls += lm.cpu().numpy()
        ms += mm
    np.testing.assert_allclose(ls, l, rtol=1e-6)
    assert np.array_equal(ms, m)
    err = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
    report(f"xcorr level masks [{which}]: |sum - unsharded| / |.| = {err:.1e}")
    assert err <= 1e-6


def test_lbfgs_is_the_same_with_reuse_and_lazy_backward_on_or_off(eng):
    """Five L-BFGS steps with closure reuse and the lazy backward off, and with both on: the same closures, decisions and
    history, and the same image bit for bit after every step.  The loss rows agree to 1e-6 and not bit for bit: the row of a
    rejected trial point comes from the forward half with the lazy backward and from a whole closure without it, and those two
    differ by one ulp in a content entry now and then whether a level carries the term or not (measured on this job from six
    start images, six steps each: one row entry with no term set, one with the term, none with 20 x the weights; the halves
    of a closure at one image are equal bit for bit, test_halves_equal_the_whole_and_run_to_run_bitwise).  The first step is
    taken and moves the image."""
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
                out.append((info.closures, info.total_closures, info.accepted, info.history, rows.copy(), _bits(x)))
            runs[(reuse, lazy)] = (out, opt.closure_stats(), opt.backward_stats())
        finally:
            opt.close()
    base = runs[(False, False)][0]
    out, stats, bw = runs[(True, True)]
    for k, (a, b) in enumerate(zip(out, base)):
        assert a[:4] == b[:4], (k, a[:4], b[:4])
        assert np.array_equal(a[5], b[5]), k
        np.testing.assert_allclose(a[4], b[4], rtol=1e-6)
    assert np.isfinite(base[-1][4]).all()
    assert sum(stats) == base[-1][1], (stats, bw)
    assert base[0][2] and not np.array_equal(base[0][5], _bits(x0))


def test_xcorr_losses_times_the_weights_plus_the_other_terms_are_the_row_totals(eng):
    """total = ((cw content + sw style) + tvw tv) + w_1 xcorr_1 + w_2 xcorr_2 ... in ascending map order, every product and sum
    rounded to fp32: bitwise from what the closure returns; the row has four entries; zeros for the maps without the term."""
    x, _, _ = _mixed_job(eng)
    _, l = eng.closure(x, CW, SW, TVW)
    assert l.numel() == 4 * 2 + 1
    rows = l.cpu().numpy()[:-1].reshape(2, 4)
    m = eng.xcorr_losses().cpu().numpy()
    on = [i for i in range(6) if MIXED_W[i] > 0]
    assert m.shape == (2, 6) and not m[:, [0, 4, 5]].any() and (m[:, on] > 0).all()
    f32 = np.float32
    for lv in range(2):
        total = (f32(CW) * rows[lv, 1] + f32(SW) * rows[lv, 2]) + f32(TVW) * rows[lv, 3]
        for i in on:
            total = f32(total + f32(MIXED_W[i]) * m[lv, i])
        assert total == rows[lv, 0], (lv, total, rows[lv, 0])
        assert rows[lv, 0] > 1.1 * float((f32(CW) * rows[lv, 1] + f32(SW) * rows[lv, 2]) + f32(TVW) * rows[lv, 3])


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
                _set_xcorr(e, s, MIXED_W)
                assert e.bytes() > before
                e.closure(dev(xt), CW, SW, TVW)
                e.clear_xcorr()
                assert e.bytes() == before
                assert all(e.xcorr_setting(i) is None for i in range(2))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            assert not e.xcorr_losses().cpu().numpy().any()
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
    before = [eng.xcorr_setting(i) for i in range(2)]
    assert before[0] == (MIXED_W, SHIFTS, (70, 110)) and before[1][2] == (35, 55)
    style = dev(cpu_ref.prepare_img(s[0]))
    hs, ws = style.shape[-2:]

    def raw(level=0, w=MIXED_W, shifts=SHIFTS, n=None, img=style, e=eng, hs=hs, ws=ws):
        flat = [v for d in shifts for v in d]
        arr = (C.c_int * max(len(flat), 1))(*flat)
        return e.lib.nst_level_set_xcorr(e.ctx, level, _ptr(img), hs, ws, (C.c_float * 6)(*w), arr, len(shifts) if n is None else n,
                                         _stream(e.device))

    # NST_E_ARG, and a refusal leaves the level as it was
    assert raw(level=-1) == -1 and raw(level=2) == -1
    for bad in (-1.0, float("nan"), float("inf")):
        assert raw(w=(0.0, 0.0, bad, 1.0, 0.0, 0.0)) == -1
    assert raw(n=0) == -1 and raw(shifts=((1, 0),) * 17) == -1
    for bad in (((0, 0),), ((-1, 0),), ((0, 65),), ((1, 0), (1, 0)), ((0, 8),), ((12, 0),)):
        assert raw(shifts=bad) == -1, bad                                # ((0, 8), (12, 0): not smaller than relu4_1, 8 x 12)
    assert raw(level=1, shifts=((0, 4),)) == -1                          # (relu4_1 of level 1 is 4 x 6)
    assert raw(w=(0.0, 0.0, 0.0, 0.0, 1.0, 0.0)) == -1                 # conv4_2 is no style map under the default taps
    assert raw(hs=8, ws=8) == -1
    assert [eng.xcorr_setting(i) for i in range(2)] == before
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # the Python setter refuses before the library is called
    for bad, text in (([(0, 0)], "xcorr_shifts"), ([65], "xcorr_shifts"), ([(0, 8)], "not smaller"), (list(range(1, 10)), "xcorr_shifts")):
        with pytest.raises(ValueError, match=text):
            eng.set_xcorr(0, style, MIXED_W, bad)
    with pytest.raises(ValueError, match="not a style map"):
        eng.set_xcorr(0, style, {4: 1.0})
    assert [eng.xcorr_setting(i) for i in range(2)] == before
    # a guided level, in either order of the two calls
    planes = torch.ones((2, 64, 96), device="cuda:0") * 0.5
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_guidance(0, planes)
    eng.clear_xcorr(0)
    eng.set_guidance(0, planes)
    assert raw() == -2 and eng.xcorr_setting(0) is None
    eng.clear_guidance()
    # a pending backward half goes with a new term
    _mixed_job(eng)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_xcorr(0, style, W_12)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure_backward(x, CW, SW, TVW)
    # configure, set_taps, set_pooling and set_color drop the term, and the bytes come back
    for drop, undo in ((lambda: eng.configure(2, 64, 96), None), (lambda: eng.set_taps(4, [0, 1, 2, 3]), eng.reset_taps),
                       (lambda: eng.set_pooling("avg"), eng.reset_pooling), (lambda: eng.set_color("luminance"), eng.reset_color)):
        _mixed_job(eng)
        assert eng.xcorr_setting(0) is not None
        drop()
        try:
            assert all(eng.xcorr_setting(i) is None for i in range(2))
            assert not eng.xcorr_losses().cpu().numpy().any()
        finally:
            if undo:
                undo()
    # the stripe closure, and the stripe sharding of the optimiser before any stripe engine is made
    e1 = StyleEngine(vgg_weights, 0)
    try:
        xs = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        assert raw(e=e1, img=xs, hs=64, ws=96, w=W_12) == -2                           # no configured job
        e1.configure(1, 64, 96)
        e1.set_targets(0, xs, xs)
        before = e1.bytes()
        e1.set_xcorr(0, xs, W_12)
        assert e1.bytes() > before
        with pytest.raises(NstError, match=r"\(-2\)"):
            e1.window_begin(xs, 0, 64, 64)
        opt = PixelOptimizer(e1, "lbfgs")
        try:
            with pytest.raises(ValueError, match="xcorr_weight cannot be combined with stripe sharding"):
                opt.shard_stripes(0, 2, None, None, None, dist_mod=object())
        finally:
            opt.close()
        # the readers name a level out of range the same way, and a map without the term
        assert e1.lib.nst_level_xcorr(e1.ctx, 1, None, None, None, None, None) == -1
        assert e1.lib.nst_level_xcorr_matrices(e1.ctx, 1, 2, _ptr(xs), _stream(e1.device)) == -1
        assert e1.lib.nst_level_xcorr_matrices(e1.ctx, 0, 0, _ptr(xs), _stream(e1.device)) == -2
        with pytest.raises(NstError):
            e1.xcorr_matrices(0, 3)
        e1.clear_xcorr()
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
        arr = (C.c_int * 2)(1, 0)
        assert e.lib.nst_level_set_xcorr(e.ctx, 0, _ptr(xs), 64, 96, (C.c_float * 6)(*W_12), arr, 1, _stream(e.device)) == -2
        e.clear_xcorr()                                            # clearing is no setting
        assert e.xcorr_setting(0) is None
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
    return asyncio.run(run())


def test_whole_job_through_the_driver():
    """neural_style_transfer_xcorr with xcorr_weight=None is neural_style_transfer_selfsim(), bitwise; with a weight every
    yielded image is finite and the result differs."""
    from artstyletransfer_amd.selfsim_loss import neural_style_transfer_selfsim
    from artstyletransfer_amd.xcorr_loss import neural_style_transfer_xcorr
    off = _run_job(neural_style_transfer_xcorr, xcorr_weight=None)
    base = _run_job(neural_style_transfer_selfsim)
    assert len(off) == len(base) >= 1 and all(np.array_equal(a, b) for a, b in zip(off, base))
    on = _run_job(neural_style_transfer_xcorr, xcorr_weight=1e7, xcorr_shifts=(2, (3, 1)), xcorr_levels=[0])
    assert len(on) >= 1 and all(np.isfinite(o).all() for o in on)
    assert not np.array_equal(on[-1], base[-1])


def test_ten_lbfgs_steps_lower_the_term(eng):
    """A 64 x 96, two-level job whose weights put the term at 90 % or more of the first level total (read from the first loss
    row): after 10 L-BFGS steps the weighted term is below the first closure's, and the image is finite."""
    from artstyletransfer_amd.engine import PixelOptimizer
    c, s, xt = _job("64x96_L1")
    w = tuple(20.0 * v for v in MIXED_W)          # (MIXED_W is about a third of the totals: 20 x that is above 90 %)
    _setup(eng, c, s, w)
    x = dev(xt).clone()
    _, l = eng.closure(x, CW, SW, TVW)
    row = l.cpu().numpy()[:4].astype(np.float64)
    first = eng.xcorr_losses().cpu().numpy().astype(np.float64) @ np.asarray(w)
    rest = CW * row[1] + SW * row[2] + TVW * row[3]
    share = (row[0] - rest) / row[0]
    assert share >= 0.90 and first[0] == pytest.approx(row[0] - rest, rel=1e-4), (share, first, row)
    opt = PixelOptimizer(eng, "lbfgs")
    try:
        for _ in range(10):
            opt.step(x, CW, SW, TVW)
    finally:
        opt.close()
    eng.closure(x, CW, SW, TVW)
    last = eng.xcorr_losses().cpu().numpy().astype(np.float64) @ np.asarray(w)
    report(f"xcorr whole job: share of the first level total {share:.1%}; weighted term per level {first} -> {last} after 10 L-BFGS steps")
    assert bool(torch.isfinite(x).all()) and last.sum() < first.sum(), (first, last)
