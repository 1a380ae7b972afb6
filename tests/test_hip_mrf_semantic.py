"""GPU: the MRF term under semantic maps (nst_level_set_patch_guidance; Champandard 2016, neural-doodle) - the patch search
steered by T(i,j) = cos(i,j) + gamma <d_i, e_j>.
1. the descriptors alone (nst_patch_descriptors) against numpy in float64;
2. the decisions of the guided match alone (nst_patch_match_guided) against fp64, held to torch-fp32's own error of the same T;
3. regions separate, exactly, at gamma = 2 - and the unguided match does cross them;
4. ties, bitwise: constant features, so the descriptors alone decide, and the lowest index wins;
5. the closure: its matches are nst_patch_match_guided's on its own maps, bitwise; under those decisions it is held to the
   patched oracle of test_hip_mrf.py (no oracle edit) on both walkers; halves, run to run;
6. off means off, bitwise, and the bytes come back; 7. life cycle and refusals; 8. a whole job."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch

from artstyletransfer_amd import regions as rg
from hip_helpers import CW, SW, TVW, dev, oracle_targets, report
from oracle import cpu_ref
from test_hip_gram_shift import _bits, _job
from test_hip_mrf import (EPS, MATCH_SHAPES, MIXED_W, W_34, PatchedOracle, _hand_over_matches, _held_to_patched_oracle, _setup,
                          _the_term_counts, dictionary, feature_like, nhwc, patches)

pytestmark = pytest.mark.gpu

MAP_SCALE = (0, 1, 2, 3, 3, 4)
TAP_LAYER = (0, 2, 4, 8, 9, 12)          # index of each tapped map among the 13 conv outputs
ONE_HOT = 0.9999


# ---- the term restated ---------------------------------------------------------------------------------------------------
def hard_planes(r, h, w):
    """Vertical bands: label(y, x) = x * R // w, as one-hot planes (R,h,w)."""
    label = np.arange(w) * r // w
    return np.ascontiguousarray(np.broadcast_to((label[None, None, :] == np.arange(r)[:, None, None]), (r, h, w)), dtype=np.float32)


def soft_planes(r, h, w, seed):
    return np.random.default_rng(seed).random((r, h, w)).astype(np.float32)


def planes_of(kind, r, h, w, seed):
    return hard_planes(r, h, w) if kind == "hard" else soft_planes(r, h, w, seed)


def descriptors64(planes, stride=1, eps=EPS):
    """(count, 4) float64: a[r] = the nine taps of plane r in row-major order, a / sqrt(sum_r a[r]^2 + eps), entries r >= R
    zero, at the centres (1 + a s, 1 + b s) - the definition in double, not yet rounded to float."""
    r, hm, wm = planes.shape
    p = planes.astype(np.float64)
    a = np.zeros((r, hm - 2, wm - 2))
    for ty in range(3):
        for tx in range(3):
            a = a + p[:, ty:ty + hm - 2, tx:tx + wm - 2]
    a = a[:, ::stride, ::stride].reshape(r, -1)
    d = a / np.sqrt((a * a).sum(axis=0) + eps)[None, :]
    out = np.zeros((d.shape[1], 4))
    out[:, :r] = d.T
    return out


def descriptors32(planes, stride=1, eps=EPS):
    """The definition's descriptors: the double results rounded once to float."""
    return descriptors64(planes, stride, eps).astype(np.float32)


def guided_scores(f, fs, d, e, gamma, stride, eps=EPS):
    """(n, m) T(i,j) = <P_i,Q_j> rq_j rp_i + gamma <d_i, e_j> in f's dtype (d, e: the float descriptors, converted)."""
    p, q = patches(f), dictionary(fs, stride)
    rq = 1.0 / torch.sqrt((q * q).sum(dim=1) + eps)
    rp = 1.0 / torch.sqrt((p * p).sum(dim=1) + eps)
    dd, ee = torch.from_numpy(d).to(f.dtype), torch.from_numpy(e).to(f.dtype)
    return (p @ q.t()) * rq[None, :] * rp[:, None] + gamma * (dd @ ee.t())


def region_of(desc):
    """Per descriptor: its region when it is one-hot (largest component > 0.9999), else -1; and the arg-max component."""
    top = desc.argmax(axis=1)
    return np.where(desc.max(axis=1) > ONE_HOT, top, -1), top


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


_MAPS = {}


def _maps(shape):
    """(f, fs, f on the device, fs on the device) of one of MATCH_SHAPES, made once (test_hip_mrf's seeds)."""
    if shape not in _MAPS:
        c, h, w, hs, ws, _ = shape
        f, fs = feature_like(c, h, w, seed=c + h), feature_like(c, hs, ws, seed=c + hs + 100)
        _MAPS[shape] = (f, fs, nhwc(f), nhwc(fs))
    return _MAPS[shape]


# ---- 1. descriptors against numpy -------------------------------------------------------------------------------------------
DESC_ULP = 2.0 * 2.0 ** -23            # 2 ulp of a float at 1: |d| <= 1, double results rounded once


@pytest.mark.parametrize("kind", ["hard", "soft"])
@pytest.mark.parametrize("r", [1, 2, 4])
def test_descriptors_vs_numpy(eng, kind, r):
    """Planes of a 45x37 image (pooling floors both sizes at every step: 22x18, 11x9, 5x4) through regions.pool_chain, then
    the definition in float64, at strides 1 and 2 and every scale that still has a patch: every component within 2 ulp of a
    float at 1 (2.4e-7) - the values are double results rounded once, and the only freedom is the last bit of the double
    square root and quotient.  Entries r >= R are exactly zero.

    Measured on the GPU (profiles/r22_mrf_semantic.txt): the largest difference is 2.1e-9 (hard planes, R = 1) ... 2.98e-8, half a
    float ulp below 1: the device's values are the float64 results rounded once."""
    chain = rg.pool_chain(planes_of(kind, r, 45, 37, seed=7 + r))
    worst = 0.0
    for scale, pl in enumerate(chain):
        if pl.shape[1] < 3 or pl.shape[2] < 3:
            continue
        for stride in (1, 2):
            got = eng.patch_descriptors(dev(torch.from_numpy(pl)), stride, EPS).cpu().numpy()
            want = descriptors64(pl, stride)
            assert got.shape == want.shape and got.dtype == np.float32
            assert not got[:, r:].any()
            err = float(np.abs(got.astype(np.float64) - want).max())
            worst = max(worst, err)
            assert err <= DESC_ULP, (kind, r, scale, stride, err)
    assert len(chain) == 5 and chain[3].shape[1:] == (5, 4)
    report(f"mrf semantic descriptors {kind} R={r}: largest |device - float64| over scales 0..3 and strides 1, 2 = {worst:.2e}")


def test_descriptors_of_an_empty_band_are_zero_and_the_call_refuses_what_it_cannot_read(eng):
    from artstyletransfer_amd._lib import NstError
    pl = hard_planes(2, 6, 12)
    pl[:, :, 4:8] = 0.0
    got = eng.patch_descriptors(dev(torch.from_numpy(pl))).cpu().numpy().reshape(4, 10, 4)
    assert not got[:, 4:6].any() and (got[:, :2, 0] > ONE_HOT).all() and (got[:, 8:, 1] > ONE_HOT).all()
    with pytest.raises(ValueError):
        eng.patch_descriptors(dev(torch.zeros((5, 6, 6))))
    with pytest.raises(ValueError):
        eng.patch_descriptors(dev(torch.zeros((2, 2, 6))))
    with pytest.raises(ValueError):
        eng.patch_descriptors(dev(torch.zeros((2, 6, 6))).double())
    with pytest.raises(NstError):
        eng.patch_descriptors(torch.zeros((2, 6, 6)))
    d, e = dev(torch.zeros((4 * 5, 4))), dev(torch.zeros((9, 4)))
    f, fs = nhwc(feature_like(64, 6, 7, seed=1)), nhwc(feature_like(64, 5, 5, seed=2))
    eng.patch_match_guided(f, fs, d, e, 1.0)
    for bad_d, bad_e in ((d[:-1].contiguous(), e), (d, e[:, :3].contiguous()), (d.cpu(), e)):
        with pytest.raises(NstError):
            eng.patch_match_guided(f, fs, bad_d, bad_e, 1.0)
    for gamma in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            eng.patch_match_guided(f, fs, d, e, gamma)


# ---- 2. decisions against fp64 ---------------------------------------------------------------------------------------------
GAMMAS = (0.25, 1.0, 2.0)


@pytest.mark.parametrize("shape", MATCH_SHAPES)
def test_guided_decisions_vs_fp64(eng, shape):
    """For R = 1, 2, 4, hard and soft planes and gamma = 0.25, 1, 2: the fp64 T of every device choice is within delta of the
    fp64 best, delta = 4 x the largest error of a torch-fp32 evaluation of the same T against fp64 on this input (measured
    here, never taken from the device); at most 1 % of the patches differ from the fp64 arg-max at all.  The device is handed
    the definition's descriptors (float64 rounded once), so this holds the search alone.

    Measured on the GPU (profiles/r22_mrf_semantic.txt), over the 18 inputs of each shape: no patch off the fp64 arg-max and a
    worst shortfall of 0 on every shape; delta 6.6e-9 ... 1.5e-6; |T - fp64 T| of the device's choice 1.7e-7 ... 3.5e-7, torch
    fp32's 1.7e-7 ... 2.9e-7."""
    c, h, w, hs, ws, stride = shape
    f, fs, fd, fsd = _maps(shape)
    f64, fs64 = f.double(), fs.double()
    worst = dict(short=0.0, differ=0.0, dev=0.0, f32=0.0, delta_lo=np.inf, delta_hi=0.0)
    for r in (1, 2, 4):
        for kind in ("hard", "soft"):
            d = descriptors32(planes_of(kind, r, h, w, seed=31 + r))
            e = descriptors32(planes_of(kind, r, hs, ws, seed=57 + r), stride)
            dd, ed = dev(torch.from_numpy(d)), dev(torch.from_numpy(e))
            for gamma in GAMMAS:
                t64 = guided_scores(f64, fs64, d, e, gamma, stride)
                t32 = guided_scores(f, fs, d, e, gamma, stride).double()
                delta = 4.0 * float((t32 - t64).abs().max())
                nn, score = eng.patch_match_guided(fd, fsd, dd, ed, gamma, stride, EPS)
                nn, score = nn.cpu(), score.cpu()
                n, m = t64.shape
                assert tuple(nn.shape) == (h - 2, w - 2) and torch.isfinite(score).all()
                idx = nn.reshape(-1).long()
                assert int(idx.min()) >= 0 and int(idx.max()) < m
                best, arg = t64.max(dim=1)
                chosen = t64.gather(1, idx[:, None]).squeeze(1)
                differ = float((idx != arg).double().mean())
                e_dev = float((score.reshape(-1).double() - chosen).abs().max())
                e_32 = float((t32.gather(1, idx[:, None]).squeeze(1) - chosen).abs().max())
                short = float((best - chosen).max())
                for k, v in (("short", short), ("differ", differ), ("dev", e_dev), ("f32", e_32), ("delta_hi", delta)):
                    worst[k] = max(worst[k], v)
                worst["delta_lo"] = min(worst["delta_lo"], delta)
                assert bool((chosen >= best - delta).all()), (r, kind, gamma, short, delta)
                assert differ <= 0.01, (r, kind, gamma, differ)
    report(f"mrf semantic match C={c} {h}x{w} vs {hs}x{ws} stride {stride}, R 1/2/4 x hard/soft x gamma 0.25/1/2: delta "
           f"{worst['delta_lo']:.2e} .. {worst['delta_hi']:.2e}, worst shortfall {worst['short']:.2e}, patches off the fp64 arg-max "
           f"{worst['differ']:.2%}; |T - fp64 T| of the choice: device {worst['dev']:.2e}, torch fp32 {worst['f32']:.2e}")


# ---- 3. regions separate, exactly --------------------------------------------------------------------------------------------
# (shape, R) with at least one interior patch - an image patch whose descriptor is one-hot and whose region has a one-hot
# dictionary entry - and how many there are.  Left out, for having none: every R = 1 (one region: nothing to separate), R = 4
# of (128,9,10,14,7,2) and of (512,5,6,6,5,1) (bands narrower than a patch on one side), and (64,3,3,3,3,1) (one patch that
# spans every band).
INTERIOR = {((64, 12, 13, 11, 9, 1), 2): 90, ((64, 12, 13, 11, 9, 1), 4): 20, ((128, 9, 10, 14, 7, 2), 2): 42,
            ((256, 7, 33, 8, 19, 1), 2): 145, ((256, 7, 33, 8, 19, 1), 4): 125, ((512, 5, 6, 6, 5, 1), 2): 3,
            ((64, 40, 37, 33, 45, 1), 2): 1254, ((64, 40, 37, 33, 45, 1), 4): 1102}


def _interior(shape, r):
    c, h, w, hs, ws, stride = shape
    d, e = descriptors32(hard_planes(r, h, w)), descriptors32(hard_planes(r, hs, ws), stride)
    reg_d, _ = region_of(d)
    reg_e, top_e = region_of(e)
    ok = (reg_d >= 0) & np.isin(reg_d, reg_e[reg_e >= 0])
    return d, e, reg_d, top_e, ok


def test_the_interior_patches_are_the_ones_listed():
    """(No GPU work: the table above against the definition.)"""
    for shape in MATCH_SHAPES:
        for r in (2, 4):
            count = int(_interior(shape, r)[4].sum())
            assert count == INTERIOR.get((shape, r), 0), (shape, r, count)


def test_regions_separate_exactly_and_the_unguided_match_crosses_them(eng):
    """Hard planes, gamma = 2: every interior patch is matched inside its region - the arg-max component of its match's
    descriptor is the patch's region.  (The cosines of these non-negative maps lie in [0,1]; an entry whose larger part lies
    in another band has <d, e> <= 3 / sqrt(45) = 0.4473, so its T is at most 1 + 2 x 0.4473 = 1.895, below the 2 x 0.99999 a
    one-hot entry of the patch's own region has before its cosine.)  With the same inputs and no guidance the match does
    cross regions, so the test cannot pass vacuously.

    Measured on the GPU (profiles/r22_mrf_semantic.txt): guided 0 of 90 / 20 / 42 / 145 / 125 / 3 / 1254 / 1102 interior patches
    cross, unguided 41 / 16 / 20 / 77 / 95 / 0 / 563 / 802."""
    crossed_unguided = 0
    for (shape, r), count in INTERIOR.items():
        f, fs, fd, fsd = _maps(shape)
        stride = shape[5]
        d, e, reg_d, top_e, ok = _interior(shape, r)
        nn, _ = eng.patch_match_guided(fd, fsd, dev(torch.from_numpy(d)), dev(torch.from_numpy(e)), 2.0, stride, EPS)
        idx = nn.cpu().numpy().reshape(-1)
        cross = int((top_e[idx[ok]] != reg_d[ok]).sum())
        plain, _ = eng.patch_match(fd, fsd, stride, EPS)
        pidx = plain.cpu().numpy().reshape(-1)
        pcross = int((top_e[pidx[ok]] != reg_d[ok]).sum())
        crossed_unguided += pcross
        report(f"mrf semantic regions C={shape[0]} {shape[1]}x{shape[2]} R={r}: {count} interior patches, matched across regions: "
               f"guided {cross}, unguided {pcross}")
        assert int(ok.sum()) == count and cross == 0, (shape, r, cross)
    assert crossed_unguided > 0


# ---- 4. ties, bitwise ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,h,w,hs,ws,stride", [(64, 9, 14, 8, 17, 1), (256, 6, 41, 9, 23, 2), (512, 7, 12, 7, 13, 1)])
def test_ties_the_descriptors_decide_and_the_lowest_index_wins(eng, c, h, w, hs, ws, stride):
    """Constant feature maps on both sides: every feat of a column is the same float, so T differs by the descriptors alone.
    Every one-hot image patch gets the LOWEST j whose descriptor is the same one-hot vector, bitwise; a patch with an
    all-zero descriptor (the content planes have an empty band) gets j = 0.  Run to run the same bits."""
    f, fs = torch.full((1, c, h, w), 0.75), torch.full((1, c, hs, ws), 1.25)
    for r in (2, 4):
        cp = hard_planes(r, h, w)
        cp[:, :, w // 2 - 2:w // 2 + 2] = 0.0                           # an empty band of four columns: two all-zero patch columns
        d = eng.patch_descriptors(dev(torch.from_numpy(cp)), 1, EPS)
        e = eng.patch_descriptors(dev(torch.from_numpy(hard_planes(r, hs, ws))), stride, EPS)
        nn, score = eng.patch_match_guided(nhwc(f), nhwc(fs), d, e, 2.0, stride, EPS)
        idx, dn, en = nn.cpu().numpy().reshape(-1), d.cpu().numpy(), e.cpu().numpy()
        reg_d, _ = region_of(dn)
        zero = ~dn.any(axis=1)
        assert zero.sum() == 2 * (h - 2) and (reg_d >= 0).sum() > 0
        assert not idx[zero].any()
        checked = 0
        for i in np.nonzero(reg_d >= 0)[0]:
            same = np.nonzero((en.view(np.uint32) == dn[i].view(np.uint32)[None, :]).all(axis=1))[0]
            if len(same):
                assert idx[i] == same[0], (r, i, idx[i], same[0])
                checked += 1
        assert checked > 0
        nn2, score2 = eng.patch_match_guided(nhwc(f), nhwc(fs), d, e, 2.0, stride, EPS)
        assert torch.equal(nn, nn2) and np.array_equal(_bits(score), _bits(score2))


# ---- 5. the closure ----------------------------------------------------------------------------------------------------------
GAMMA = 2.0


def _level_planes(c, s, r=2):
    """Per level (content planes, style planes): vertical bands at the level's own sizes."""
    return [(hard_planes(r, *ci.shape[:2]), hard_planes(r, *si.shape[:2])) for ci, si in zip(c, s)]


def _set_guidance(e, planes, gamma=GAMMA):
    for l, (cp, sp) in enumerate(planes):
        e.set_patch_guidance(l, dev(torch.from_numpy(cp)), dev(torch.from_numpy(sp)), gamma)


def _guided_job(e, w=W_34, r=2):
    c, s, xt = _job("64x96_L1")
    _setup(e, c, s, w)
    planes = _level_planes(c, s, r)
    _set_guidance(e, planes)
    return dev(xt), c, s, planes


def _closure_case(e, monkeypatch, vgg_weights, what):
    c, s, xt = _job("64x96_L1")
    patched = PatchedOracle(monkeypatch, W_34)
    tg = oracle_targets(c, s, vgg_weights)
    _setup(e, c, s, W_34)
    planes = _level_planes(c, s)
    _set_guidance(e, planes)
    assert all(e.patch_guidance(l) == (2, GAMMA) for l in range(2))
    _hand_over_matches(e, patched, dev(xt), W_34)
    # the closure's matches are the guided match of its own maps under the descriptors of the pooled planes, bitwise
    crossed = 0
    for l in range(2):
        acts = e.level_activations(l)
        style_maps = e.vgg_features(dev(cpu_ref.prepare_img(s[l])))
        cchain, schain = rg.pool_chain(planes[l][0]), rg.pool_chain(planes[l][1])
        for i in (2, 3):
            d = e.patch_descriptors(dev(torch.from_numpy(cchain[MAP_SCALE[i]])), 1, EPS)
            ee = e.patch_descriptors(dev(torch.from_numpy(schain[MAP_SCALE[i]])), 1, EPS)
            fmap = acts[TAP_LAYER[i]].squeeze(0).permute(1, 2, 0).contiguous()
            smap = style_maps[i].squeeze(0).permute(1, 2, 0).contiguous()
            nn, _ = e.patch_match_guided(fmap, smap, d, ee, GAMMA, 1, EPS)
            assert torch.equal(nn.cpu(), patched.nn[l][i]), (what, l, i)
            plain, _ = e.patch_match(fmap, smap, 1, EPS)
            crossed += int((plain.cpu() != nn.cpu()).sum())
    assert crossed > 0, "the guidance moved no match: the case shows nothing"
    cache = {}
    _the_term_counts(patched, xt, tg, vgg_weights, what, cache)
    _held_to_patched_oracle(e, xt, tg, vgg_weights, what, cache)


def test_closure_batched_walker(eng, vgg_weights, monkeypatch):
    _closure_case(eng, monkeypatch, vgg_weights, "semantic, batched walker")


def test_closure_per_level_walker(eng_per_level, vgg_weights, monkeypatch):
    _closure_case(eng_per_level, monkeypatch, vgg_weights, "semantic, per-level walker")


def test_halves_equal_the_whole_and_run_to_run_bitwise(eng):
    x, _, _, _ = _guided_job(eng, MIXED_W)
    g, l = eng.closure(x, CW, SW, TVW)
    m = eng.patch_losses()
    nn = [eng.patch_matches(lv, 3).clone() for lv in range(2)]
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(l), _bits(l2))
    assert np.array_equal(_bits(m), _bits(eng.patch_losses()))
    assert all(torch.equal(a, eng.patch_matches(lv, 3)) for lv, a in enumerate(nn))
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


# ---- 6. off means off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["gamma 0", "cleared"])
def test_off_is_bitwise_an_engine_that_never_called_the_setter(vgg_weights, how):
    from artstyletransfer_amd.engine import StyleEngine
    c, s, xt = _job("64x96_L1")
    out = []
    for call in (False, True):
        e = StyleEngine(vgg_weights, 0)
        try:
            _setup(e, c, s, MIXED_W)
            if call:
                before = e.bytes()
                planes = _level_planes(c, s)
                _set_guidance(e, planes)
                assert e.bytes() > before and e.patch_guidance(0) == (2, GAMMA)
                g1, _ = e.closure(dev(xt), CW, SW, TVW)
                if how == "gamma 0":
                    _set_guidance(e, planes, gamma=0.0)
                else:
                    e.clear_patch_guidance()
                assert e.bytes() == before
                assert all(e.patch_guidance(i) is None for i in range(2))
            g, l = e.closure(dev(xt), CW, SW, TVW)
            nn = [e.patch_matches(lv, i).cpu() for lv in range(2) for i in (1, 2, 3)]
            out.append((_bits(g), _bits(l), _bits(e.patch_losses()), nn))
            if call:
                assert not np.array_equal(_bits(g1), out[-1][0])          # (the guidance had moved the gradient)
        finally:
            e.close()
    for k in range(3):
        assert np.array_equal(out[0][k], out[1][k]), k
    assert all(torch.equal(a, b) for a, b in zip(out[0][3], out[1][3]))


# ---- 7. life cycle and refusals ------------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(eng):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import _ptr, _stream
    c, s, xt = _job("64x96_L1")
    planes = _level_planes(c, s)
    cp, sp = (dev(torch.from_numpy(a)) for a in planes[0])

    def raw(level=0, r=2, gamma=2.0, a=cp, b=sp):
        return eng.lib.nst_level_set_patch_guidance(eng.ctx, level, r, _ptr(a), _ptr(b), C.c_float(gamma), _stream(eng.device))

    # guidance before patches: NST_E_STATE; clearing such a level is no setting
    eng.configure(2, 64, 96)
    for i in range(2):
        eng.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))
    assert raw() == -2
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.set_patch_guidance(0, cp, sp)
    eng.clear_patch_guidance()
    # NST_E_ARG, and a refusal leaves the level as it was
    x, _, _, _ = _guided_job(eng, MIXED_W)
    g0, l0 = eng.closure(x, CW, SW, TVW)
    assert raw(level=-1) == -1 and raw(level=2) == -1
    assert raw(r=5) == -1 and raw(r=-1) == -1
    for bad in (-1.0, float("nan"), float("inf")):
        assert raw(gamma=bad) == -1
    for side in (0, 1):
        spoiled = [cp.clone(), sp.clone()]
        spoiled[side][1, 5, 7] = 1.5
        assert raw(a=spoiled[0], b=spoiled[1]) == -1
        spoiled[side][1, 5, 7] = float("nan")
        assert raw(a=spoiled[0], b=spoiled[1]) == -1
    assert eng.patch_guidance(0) == (2, GAMMA)
    g1, l1 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    # an empty region on either side is no refusal (the mass rule of the guided Gram does not apply)
    empty = [cp.clone(), sp.clone()]
    empty[0][1] = 0.0
    empty[1][0] = 0.0
    assert raw(a=empty[0], b=empty[1]) == 0
    # engine.py, before the call: planes of the wrong size, dtype or R, a bad gamma
    for a, b in ((cp[:, :-1].contiguous(), sp), (cp, sp[:, :, :-1].contiguous()), (cp[:1].contiguous(), sp), (cp.double(), sp),
                 (cp[0], sp), (dev(torch.zeros((5, 64, 96))), dev(torch.zeros((5, 70, 110))))):
        with pytest.raises(ValueError):
            eng.set_patch_guidance(0, a, b)
    for gamma in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            eng.set_patch_guidance(0, cp, sp, gamma)
    # a pending backward half goes with new guidance
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_patch_guidance(0, cp, sp, 1.0)
    with pytest.raises(NstError, match=r"\(-2\)"):
        eng.closure_backward(x, CW, SW, TVW)
    # whatever drops the term drops its guidance, and the bytes with it
    style0 = dev(cpu_ref.prepare_img(s[0]))
    for drop, undo in ((lambda: eng.set_patches(0, style0, W_34), None), (lambda: eng.clear_patches(0), None),
                       (lambda: eng.configure(2, 64, 96), None), (lambda: eng.set_taps(4, [0, 1, 2, 3]), eng.reset_taps),
                       (lambda: eng.set_pooling("avg"), eng.reset_pooling), (lambda: eng.set_color("luminance"), eng.reset_color)):
        _guided_job(eng, MIXED_W)
        assert eng.patch_guidance(0) == (2, GAMMA)
        drop()
        try:
            assert eng.patch_guidance(0) is None
        finally:
            if undo:
                undo()
    # the reader names a level out of range as the other readers of the term do
    assert eng.lib.nst_level_patch_guidance(eng.ctx, 7, None, None, None, None) == -1


# ---- 8. a whole job ----------------------------------------------------------------------------------------------------------
def _run_job(fn, capture=None, **kw):
    import neural_style_transfer as nst
    content = cpu_ref.synthetic_image(64, 96, seed=1)
    style = cpu_ref.synthetic_image(70, 110, seed=2)
    pair = nst.ContentStylePair(("c", content), ("s", style))
    np.random.seed(1234)

    async def run():
        return [img async for _, img in fn(pair, CW, SW, TVW, "lbfgs", "vgg19", "content+noise", 3, 1, 0.95, (9, 18, 36, -1, 0),
                                           (0.3, 0.2, 0.1, 0.2, 0.2), (0.2, 0.3, 0.4, 0.1, 0.0), (0.2, 0.3, 0.4, 0.6, 0.3),
                                           device=torch.device("cuda", 0), **kw)]
    return asyncio.run(run())


def test_whole_job(monkeypatch):
    """neural_style_transfer_mrf_semantic on a 64x96 pair (one level, which the driver resizes to a short edge of 256), three
    L-BFGS steps, two vertical bands, gamma = 2: finite images that differ from the same job without the maps, and after the
    last closure no interior patch of relu3_1 is matched across the bands."""
    from artstyletransfer_amd import neural_style_transfer as impl
    from artstyletransfer_amd.patch_match import neural_style_transfer_mrf, neural_style_transfer_mrf_semantic
    seen = {}
    close0 = impl._DeviceJob.close

    def close(self):
        with torch.cuda.device(self.dev), torch.cuda.stream(self.job_stream):
            if self.optimizer is not None and "nn" not in seen and self.engine.patch_guidance(0) is not None:
                seen["nn"] = self.engine.patch_matches(0, 2).cpu().numpy().reshape(-1)
                seen["losses"] = self.engine.patch_losses().cpu().numpy()
                seen["shape"] = self.engine.level_shape(0)
        close0(self)

    monkeypatch.setattr(impl._DeviceJob, "close", close)
    labels, slabels = hard_planes(2, 64, 96).argmax(axis=0), hard_planes(2, 70, 110).argmax(axis=0)
    out = _run_job(neural_style_transfer_mrf_semantic, mrf_weight=300.0, semantic_content=labels, semantic_style=slabels, semantic_weight=2.0)
    assert len(out) >= 1 and all(np.isfinite(o).all() for o in out)
    assert "nn" in seen and np.isfinite(seen["losses"]).all() and (seen["losses"][0, [2, 3]] > 0).all()
    plain = _run_job(neural_style_transfer_mrf, mrf_weight=300.0)
    assert len(plain) >= 1 and not np.array_equal(plain[-1], out[-1])
    none = _run_job(neural_style_transfer_mrf_semantic, mrf_weight=300.0)
    assert len(none) == len(plain) and all(np.array_equal(a, b) for a, b in zip(plain, none))         # (no map: neural_style_transfer_mrf, bitwise)
    # the bands at relu3_1 of the level, as the job made them: resized, then pooled twice
    from artstyletransfer_amd import host_image
    h, w = seen["shape"]
    hs, ws = host_image.level_size(70, 110, 0)
    d = descriptors32(rg.pool_chain(rg.resize_nearest(hard_planes(2, 64, 96), h, w))[2])
    e = descriptors32(rg.pool_chain(rg.resize_nearest(hard_planes(2, 70, 110), hs, ws))[2])
    reg_d, _ = region_of(d)
    _, top_e = region_of(e)
    ok = reg_d >= 0
    assert len(seen["nn"]) == len(d) and ok.sum() > 0.9 * len(d)
    assert int((top_e[seen["nn"][ok]] != reg_d[ok]).sum()) == 0
