"""GPU: the matting term (nst_job_set_matting, StyleEngine.set_matting; Luan, Paris, Shechtman & Bala 2017) against a torch
restatement of the definition in include/nst_hip.h, written here: F.unfold for the 3x3 windows, torch.linalg.solve per window,
autograd, and cpu_ref.bicubic_half for the pyramid.  tests/test_matting_host.py holds the restatement to a dense Levin matrix.

Bounds.  "Bound 1" of a quantity = max(3 x the distance of the same restatement in torch fp32 from fp64, 5e-6), rel-L2 for a
gradient and relative for a value (test_hip_laplacian.py's rule).  Loss rows: check_rows at 2e-5, totals 1e-5; additivity 2e-6 -
hip_helpers' own bounds.

The kernels' tile is 32 x 8 (matting.hip: MAT_TW x MAT_TH; windows in the value pass, pixels in the gradient pass).  Geometries
of the piece: 3x3 (one window), 5x7, 50x76 (odd, w % 4 != 0), 9x33 (one pixel more than the tile of pixels), 11x35 (one window
more than the tile of windows), 32x48."""
import asyncio
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, check_rows, dev, device_decisions, oracle_targets, rel_l2, report

pytestmark = pytest.mark.gpu

MODES = {"f16x2": {}, "per_level": {"batched": False}, "bf16x3": {"conv_mode": "bf16x3"}, "f32": {"conv_mode": "f32"}}
FLOOR = 5e-6
TILE_H, TILE_W = 8, 32
MEAN = torch.tensor(cpu_ref.IMAGENET_MEAN_255, dtype=torch.float64).view(1, 3, 1, 1)


# ---- the restatement --------------------------------------------------------------------------------------------------------
def windows(t):
    """(1,C,h,w) -> (L, 9, C): the nine pixels of every 3x3 window that lies inside the image, L = (h-2)(w-2)."""
    c = t.shape[1]
    return F.unfold(t, 3).view(c, 9, -1).permute(2, 1, 0)


def mat_term(y, guide, eps):
    """mat of the prepared image y (1,3,h,w) under the guide I (1,3,h,w): (1/n) sum_k sum_c E_kc, n = 3 (h-2)(w-2)."""
    iw = windows(guide)
    ic = iw - iw.mean(dim=1, keepdim=True)
    m = ic.transpose(1, 2) @ ic / 9.0 + (eps / 9.0) * torch.eye(3, dtype=y.dtype)
    vw = windows(y / 255.0)
    vc = vw - vw.mean(dim=1, keepdim=True)
    v = ic.transpose(1, 2) @ vc                      # (L, 3, C): column c is v of output channel c
    a = torch.linalg.solve(m, v) / 9.0
    e = (vc * vc).sum(dim=1) - (v * a).sum(dim=1)    # (L, C)
    return e.sum() / (3.0 * e.shape[0])


def mat_piece(y, guide, eps, dtype):
    """(value, gradient) in `dtype`."""
    y = y.detach().to(dtype).clone().requires_grad_(True)
    v = mat_term(y, guide.to(dtype), eps)
    v.backward()
    return float(v.detach()), y.grad.detach()


def guide_of(content_prepared, dtype):
    """I = (content_l + IMAGENET_MEAN_255) / 255 of a prepared (1,3,h,w) content level."""
    return ((content_prepared.double() + MEAN) / 255.0).to(dtype)


def mat_closure(x, contents, gamma, eps, dtype):
    """The term of a whole job: sum over the levels of gamma mat on the bicubic 1/2 chain of x.  Returns (grad, per-level
    gamma mat, per-level mat)."""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    lv, total, vals = [x], 0.0, []
    for l, c in enumerate(contents):
        if l > 0:
            lv.append(cpu_ref.bicubic_half(lv[-1]))
        v = mat_term(lv[l], guide_of(c, dtype), eps)
        total = total + gamma * v
        vals.append(float(v.detach()))
    total.backward()
    vals = np.array(vals)
    return x.grad.detach(), gamma * vals, vals


def bound1(fp32, fp64):
    return max(3.0 * rel_l2(np.asarray(fp32), np.asarray(fp64)), FLOOR)


def bound1_value(v32, v64):
    return max(3.0 * abs(v32 - v64) / abs(v64), FLOOR)


# ---- jobs ---------------------------------------------------------------------------------------------------------------------
# gamma: chosen on the CPU with the oracle and the restatement alone, so that under (CW, SW, TVW) the term is 10-50 % of every
# level total.  At the fixtures' x: L0 (50x76) mat = 5.647e-6 against an oracle level total of 1.019e5: gamma = 5e9 gives the
# term 22 %.  L1 (64x96 + 32x48) mat = 1.286e-5 and 1.200e-4 against 3.040e4 and 3.638e4: the two levels' ratios differ by 8, so
# one gamma for both levels (the term has no per-level weight) has to lie in 2.63e8 .. 3.03e8; 2.8e8 gives 10.6 % and 48 %.
# At these x the restatement in torch fp32 sits 1.3e-4 (L0) and 8.9e-5 (L1) from fp64 in the gradient and 6.8e-6 / 1.4e-5 /
# 7.2e-7 in the values (the fixtures' guides are smooth: near rank 1 in most windows).
EPS = 1e-7
JOBS = {"L0": ("closure_50x76_L0", 1, 5.0e9), "L1": ("closure_64x96_L1", 2, 2.8e8)}
GAMMA = JOBS["L1"][2]


def cpu_ref_golden(name):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _job(name):
    fx = cpu_ref_golden(JOBS[name][0])
    nlev = JOBS[name][1]
    contents = [fx[f"content{i}"] for i in range(nlev)]
    styles = [fx[f"style{i}"] for i in range(nlev)]
    return contents, styles, cpu_ref.prepare_img(fx["x_img"])


@functools.lru_cache(maxsize=None)
def _restated(name):
    """fp64 and fp32 restatement of the term of job `name` at the job's x: shared by the tests, never changed."""
    contents, _, xt = _job(name)
    cp = [cpu_ref.prepare_img(c) for c in contents]
    g64, rows64, vals64 = mat_closure(xt, cp, JOBS[name][2], EPS, torch.float64)
    g32, rows32, vals32 = mat_closure(xt, cp, JOBS[name][2], EPS, torch.float32)
    return g64, rows64, vals64, g32, rows32, vals32


@pytest.fixture(scope="module")
def engines(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = StyleEngine(vgg_weights, 0, **MODES[mode])
        return made[mode]
    yield get
    for e in made.values():
        e.close()


def _targets(eng, contents, styles):
    for i in range(len(contents)):
        eng.set_targets(i, dev(cpu_ref.prepare_img(contents[i])), dev(cpu_ref.prepare_img(styles[i])))


def _setup(eng, name, gamma=None, eps=EPS):
    """Configure (which clears any matting setting), set the term, make the targets."""
    contents, styles, xt = _job(name)
    h, w = contents[0].shape[:2]
    eng.configure(len(contents), h, w)
    if gamma:
        eng.set_matting(gamma, eps)
        assert eng.matting == (float(np.float32(gamma)), eps)
    _targets(eng, contents, styles)
    return dev(xt)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ---- 1. the piece alone -------------------------------------------------------------------------------------------------------
GEOMETRIES = [(3, 3), (5, 7), (50, 76), (TILE_H + 1, TILE_W + 1), (TILE_H + 3, TILE_W + 3), (32, 48)]
GUIDES = ["noise", "ramp", "constant", "quantised"]


def _guide(kind, h, w, seed):
    """(h,w,3) float32 guide I in [0,1]."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        g = rng.random((h, w, 3))
    elif kind == "ramp":            # a coloured ramp plus a little noise: near rank 1 in every window
        t = (np.arange(w)[None, :] / max(w - 1, 1) + np.arange(h)[:, None] / max(h - 1, 1)) / 2.0
        g = 0.1 + t[:, :, None] * np.array([0.7, 0.5, 0.2])[None, None, :] + 1e-3 * rng.standard_normal((h, w, 3))
    elif kind == "constant":
        g = np.broadcast_to(np.array([0.3, 0.5, 0.7]), (h, w, 3))
    else:                           # 8-bit quantised, near constant: the worst conditioning
        g = np.round(rng.random((h, w, 3)) * 3.0 + 100.0) / 255.0
    return np.ascontiguousarray(np.clip(g, 0.0, 1.0), dtype=np.float32)


def _image(kind, guide, seed):
    """Prepared (1,3,h,w) image: uniform noise, or the prepared guide plus noise of rms 5."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return cpu_ref.prepare_img(rng.random(guide.shape).astype(np.float32))
    y = cpu_ref.prepare_img(guide)
    return y + torch.from_numpy((5.0 * rng.standard_normal(tuple(y.shape))).astype(np.float32))


def _chw(guide):
    return torch.from_numpy(guide).permute(2, 0, 1).unsqueeze(0).contiguous()


@pytest.mark.parametrize("kind", GUIDES)
@pytest.mark.parametrize("h,w", GEOMETRIES)
def test_piece_vs_restatement(engines, h, w, kind):
    """nst_matting_loss against the fp64 restatement under bound 1, value and gradient, for two images and two epsilons; the
    value-only call gives bitwise the value of the value-and-gradient call."""
    eng = engines("f16x2")
    guide = _guide(kind, h, w, 31)
    gt = _chw(guide)
    for image in ("noise", "near"):
        y = _image(image, guide, 32)
        for eps in (1e-7, 1e-4):
            v64, g64 = mat_piece(y, gt, eps, torch.float64)
            v32, g32 = mat_piece(y, gt, eps, torch.float32)
            bv, bg = bound1_value(v32, v64), bound1(g32, g64)
            val, grad = eng.matting_loss(dev(y), dev(gt), eps, want_grad=True)
            only = eng.matting_loss(dev(y), dev(gt), eps)
            val, grad = float(val.cpu()), grad.cpu()
            ev, eg = abs(val - v64) / abs(v64), rel_l2(grad.numpy(), g64.numpy())
            report(f"matting piece {h}x{w} guide={kind} image={image} eps={eps:g}: value rel {ev:.2e} (bound {bv:.2e}, torch fp32 "
                   f"{abs(v32 - v64) / abs(v64):.1e}), gradient rel-L2 {eg:.2e} (bound {bg:.2e}, torch fp32 {rel_l2(g32.numpy(), g64.numpy()):.1e})")
            assert float(only.cpu()) == val
            assert tuple(grad.shape) == (1, 3, h, w) and torch.isfinite(grad).all()
            assert ev <= bv and eg <= bg


@pytest.mark.parametrize("h,w", [(50, 76), (32, 48)])
def test_piece_luminance_vs_restatement_on_three_channels(engines, h, w):
    """C = 1: the term of the plane u under the one-plane guide is the three-channel term at E(u) with three equal guide
    channels, its gradient the sum over the three channels."""
    eng = engines("f16x2")
    rng = np.random.default_rng(41)
    u = torch.from_numpy((rng.random((1, 1, h, w)) * 255.0).astype(np.float32))
    gu = torch.from_numpy(rng.random((1, 1, h, w)).astype(np.float32))

    def piece(dtype, eps):
        x = u.to(dtype).clone().requires_grad_(True)
        v = mat_term(x.expand(-1, 3, -1, -1) - MEAN.to(dtype), gu.to(dtype).expand(-1, 3, -1, -1), eps)
        v.backward()
        return float(v.detach()), x.grad.detach()

    for eps in (1e-7, 1e-4):
        (v64, g64), (v32, g32) = piece(torch.float64, eps), piece(torch.float32, eps)
        bv, bg = bound1_value(v32, v64), bound1(g32, g64)
        val, grad = eng.matting_loss(dev(u), dev(gu), eps, want_grad=True)
        ev, eg = abs(float(val.cpu()) - v64) / abs(v64), rel_l2(grad.cpu().numpy(), g64.numpy())
        report(f"matting piece C=1 {h}x{w} eps={eps:g}: value rel {ev:.2e} (bound {bv:.2e}), gradient rel-L2 {eg:.2e} (bound {bg:.2e})")
        assert tuple(grad.shape) == (1, 1, h, w)
        assert ev <= bv and eg <= bg


# ---- 3. the term inside the closure ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,name", [("f16x2", "L0"), ("f16x2", "L1"), ("per_level", "L0"), ("per_level", "L1"),
                                       ("bf16x3", "L0"), ("bf16x3", "L1"), ("f32", "L0"), ("f32", "L1")])
def test_term_inside_the_closure(engines, vgg_weights, mode, name):
    """matting_losses() and the change of the level totals against fp64; g(closure with the term) - g(closure without) against
    the restated term's gradient under bound 1 and the additivity bound; the full row against oracle + restatement."""
    eng = engines(mode)
    nlev = JOBS[name][1]
    contents, styles, xt = _job(name)
    g64, rows64, vals64, g32, _, vals32 = _restated(name)
    x = _setup(eng, name)
    g_off, l_off = eng.closure(x, CW, SW, TVW)
    assert eng.matting is None and torch.count_nonzero(eng.matting_losses()) == 0
    rows_off = l_off.cpu().numpy()[:-1].reshape(nlev, 4).astype(np.float64)
    g_off, l_off = g_off.clone(), l_off.clone()
    x = _setup(eng, name, JOBS[name][2])
    g_on, l_on = eng.closure(x, CW, SW, TVW)
    g_on, l_on = g_on.clone(), l_on.clone()
    per = eng.matting_losses().cpu().numpy().astype(np.float64)
    g_alone, l_alone = eng.closure(x, 0.0, 0.0, 0.0)
    rows_on = l_on.cpu().numpy()[:-1].reshape(nlev, 4).astype(np.float64)
    rows_alone = l_alone.cpu().numpy()[:-1].reshape(nlev, 4).astype(np.float64)
    share = rows64 / (rows_off[:, 0] + rows64)
    ev = float(np.max(np.abs(per - vals64) / vals64))
    bv = max(bound1_value(a, b) for a, b in zip(vals32, vals64))
    diff = g_on.cpu().numpy().astype(np.float64) - g_off.cpu().numpy().astype(np.float64)
    # bound 1 holds the difference of the two closures' gradients and the term's own gradient (weights 0); the additivity bound
    # holds g(on) against g(off) + g(term alone)
    eg, bg = rel_l2(g_alone.cpu().numpy(), g64.numpy()), bound1(g32, g64)
    ed = rel_l2(diff, g64.numpy())
    s = g_off.cpu().numpy().astype(np.float64) + g_alone.cpu().numpy().astype(np.float64)
    add = float(np.linalg.norm(g_on.cpu().numpy().astype(np.float64) - s) / np.linalg.norm(s))
    report(f"matting in the closure {name} [{mode}]: term share of the level totals {np.array2string(share, precision=2)}, mat rel {ev:.2e} "
           f"(bound {bv:.2e}), term gradient rel-L2 {eg:.2e}, g(on) - g(off) rel-L2 {ed:.2e} (bound {bg:.2e}), "
           f"additivity {add:.1e}; |g(mat)| / |g(off)| = {np.linalg.norm(g64.numpy()) / np.linalg.norm(g_off.cpu().numpy()):.2f}")
    assert np.all(share >= 0.10) and np.all(share <= 0.50), share
    assert ev <= bv
    np.testing.assert_allclose(rows_alone[:, 0], rows64, rtol=1e-5)
    np.testing.assert_allclose(rows_on[:, 0] - rows_off[:, 0], rows64, rtol=1e-5, atol=2e-6 * float(rows_on[:, 0].max()))
    assert np.array_equal(_bits(l_on)[:-1].reshape(nlev, 4)[:, 1:], _bits(l_off)[:-1].reshape(nlev, 4)[:, 1:])
    assert eg <= bg and ed <= bg
    assert add <= 2e-6
    if mode in ("f16x2", "per_level"):
        dec = device_decisions(eng, x)
        tg = oracle_targets(contents, styles, vgg_weights)
        loss_o, _, rows_o = cpu_ref.closure_eval(xt, tg, vgg_weights, CW, SW, TVW, decisions=dec)
        ref_rows = np.array(rows_o, dtype=np.float64)
        ref_rows[:, 0] += rows64
        check_rows(rows_on, ref_rows, 2e-5)
        assert abs(float(l_on[-1].cpu()) - (float(loss_o) + rows64.sum())) <= 1e-5 * (float(loss_o) + rows64.sum())


# ---- 4. off is off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
def test_off_is_off(vgg_weights, mode):
    """set_matting(0) and never calling it: bitwise equal loss rows and gradient, the same launch count and context bytes; with
    the term a closure has two more launches per level."""
    from artstyletransfer_amd.engine import StyleEngine
    out = []
    for call in (False, True):
        e = StyleEngine(vgg_weights, 0, **MODES[mode])
        try:
            e.set_timing(2)
            x = _setup(e, "L1")
            if call:
                before = e.bytes()
                assert e.lib.nst_job_set_matting(e.ctx, 0.0, 1e-7) == 0
                assert e.matting_setting() is None and e.bytes() == before
            _targets(e, *_job("L1")[:2])
            g, l = e.closure(x, CW, SW, TVW)
            out.append((_bits(g), _bits(l), len(e.last_closure_launches()), e.bytes()))
            assert torch.count_nonzero(e.matting_losses()) == 0
            if call:
                e.set_matting(GAMMA)
                _targets(e, *_job("L1")[:2])
                e.closure(x, CW, SW, TVW)
                with_term = len(e.last_closure_launches())
        finally:
            e.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][2] > 0
    assert out[0][3] == out[1][3]
    assert with_term == out[0][2] + 2 * 2


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------
def test_two_closures_and_the_halves_are_bitwise_equal(engines):
    eng = engines("f16x2")
    x = _setup(eng, "L1", GAMMA)
    g, l = eng.closure(x, CW, SW, TVW)
    g, l = g.clone(), l.clone()
    per = eng.matting_losses().clone()
    g2, l2 = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g2), _bits(g)) and np.array_equal(_bits(l2), _bits(l))
    g3, l3 = eng.closure_levels(x, CW, SW, TVW, 3)
    assert np.array_equal(_bits(g3), _bits(g)) and np.array_equal(_bits(l3), _bits(l))
    lf = eng.closure_forward(x, CW, SW, TVW)
    assert np.array_equal(_bits(lf), _bits(l))
    assert torch.equal(eng.matting_losses(), per)
    gb = eng.closure_backward(x, CW, SW, TVW)
    assert np.array_equal(_bits(gb), _bits(g))


def test_lbfgs_is_the_same_with_reuse_and_lazy_backward_on_or_off(engines):
    from artstyletransfer_amd.engine import PixelOptimizer
    eng = engines("f16x2")
    x0 = _setup(eng, "L1", GAMMA)
    runs = {}
    for reuse, lazy in ((False, False), (True, True)):
        opt = PixelOptimizer(eng, "lbfgs")
        try:
            opt.set_closure_reuse(reuse)
            opt.set_lazy_backward(lazy)
            x = x0.clone()
            out = []
            for _ in range(6):
                info, rows = opt.step(x, CW, SW, TVW)
                out.append((info.closures, info.total_closures, info.accepted, info.history,
                            int(np.float32(info.loss).view(np.uint32)), rows.view(np.uint32).copy(), _bits(x)))
            runs[(reuse, lazy)] = out
        finally:
            opt.close()
    for k, (a, b) in enumerate(zip(runs[(True, True)], runs[(False, False)])):
        assert a[:5] == b[:5], (k, a[:5], b[:5])
        assert np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6]), k
    assert np.isfinite(runs[(False, False)][-1][5].view(np.float32)).all()


def test_graph_replay_captures_the_term(vgg_weights):
    """use_graph = 1: the closure with the term, replayed as a hipGraph, writes the bits the plain launches write."""
    from artstyletransfer_amd.engine import StyleEngine
    out = []
    for graph in (False, True):
        e = StyleEngine(vgg_weights, 0, use_graph=graph)
        try:
            x = _setup(e, "L1", GAMMA)
            g = torch.empty_like(x)
            l = torch.empty(9, dtype=torch.float32, device=x.device)
            for _ in range(3):                                # (captured the second time the same buffers are passed)
                e.closure(x, CW, SW, TVW, grad=g, losses=l)
            out.append((_bits(g), _bits(l), _bits(e.matting_losses())))
        finally:
            e.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


# ---- 6. life cycle and refusals ---------------------------------------------------------------------------------------------------
def test_life_cycle_and_refusals(engines):
    from artstyletransfer_amd._lib import NstError
    eng = engines("f16x2")
    contents, styles, _ = _job("L1")
    x = _setup(eng, "L1")
    eng.closure(x, CW, SW, TVW)
    for step in ("set", "set", "off"):          # setting the term, even the same one, and switching it off drop the targets
        if step == "set":
            eng.set_matting(GAMMA, 1e-4)
        else:
            eng.reset_matting()
        with pytest.raises(NstError, match=r"\(-2\)"):
            eng.closure(x, CW, SW, TVW)
        _targets(eng, contents, styles)
        eng.closure(x, CW, SW, TVW)
    assert eng.matting is None
    eng.set_matting(GAMMA, 1e-4)
    _targets(eng, contents, styles)
    g0, l0 = eng.closure(x, CW, SW, TVW)
    before = eng.matting_setting()
    assert before == (GAMMA, 1e-4)
    for gamma, eps in ((-1.0, 1e-7), (float("nan"), 1e-7), (float("inf"), 1e-7), (1.0, 0.0), (1.0, -1e-7), (1.0, float("nan")),
                       (1.0, float("inf"))):
        assert eng.lib.nst_job_set_matting(eng.ctx, gamma, eps) == -1, (gamma, eps)
        with pytest.raises(ValueError):
            eng.set_matting(gamma, eps)
    assert eng.matting_setting() == before and eng.matting == before      # every refusal left the setting ...
    g1, l1 = eng.closure(x, CW, SW, TVW)                                   # ... the targets and the context as they were
    assert np.array_equal(_bits(g1), _bits(g0)) and np.array_equal(_bits(l1), _bits(l0))
    eng.configure(2, 64, 96)                                               # configure clears the setting
    assert eng.matting is None and eng.matting_setting() is None


def test_setter_needs_a_configured_job_and_the_stripe_closure_refuses_the_term(vgg_weights):
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    try:
        assert e.lib.nst_job_set_matting(e.ctx, 1.0, 1e-7) == -2
        x = dev(cpu_ref.prepare_img(cpu_ref.synthetic_image(64, 96, 1)))
        e.configure(1, 64, 96)
        e.set_matting(1.0)
        assert e.matting_setting() == (1.0, 1e-7)
        e.set_targets(0, x, x)
        with pytest.raises(NstError, match=r"\(-2\).*matting"):
            e.window_begin(x, 0, 64, 64)
        e.reset_matting()
        e.set_targets(0, x, x)
        e.window_begin(x, 0, 64, 64)
    finally:
        e.close()


def test_pooled_engine_comes_back_without_the_setting(vgg_weights):
    from artstyletransfer_amd import neural_nets
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 64, 96)
    e.set_matting(3.0)
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.matting is None and again.matting_setting() is None
    finally:
        neural_nets.return_engine(again)


# ---- 7. composition ----------------------------------------------------------------------------------------------------------------
def test_composition_with_laplacian_regions_avg_pooling_and_luminance(engines):
    """One two-level job with the Laplacian loss, two regions, pooling="avg" and the luminance closure: the loss row is the row
    without the term plus gamma mat, added last (bitwise: the same float sum), the gradient is additive, and the level-sharded
    closures (masks {0} and {1}) add up to the unsharded one."""
    eng = engines("f16x2")
    contents, styles, xt = _job("L1")
    h, w = contents[0].shape[:2]
    gamma = 3.0e7

    def planes(hh, ww):
        m = np.zeros((2, hh, ww), np.float32)
        m[0, :, : ww // 2] = 1.0
        m[1, :, ww // 2:] = 1.0
        return torch.from_numpy(m)

    def setup(with_term):
        eng.configure(2, h, w)
        eng.set_pooling("avg")
        eng.set_color("luminance")
        eng.set_laplacian((4,), (50.0,))
        if with_term:
            eng.set_matting(gamma)
        for i in range(2):
            c = eng.luminance(dev(torch.from_numpy(contents[i])))
            s = eng.luminance(dev(torch.from_numpy(styles[i])))
            hh, ww = contents[i].shape[:2]
            sh, sw_ = styles[i].shape[:2]
            eng.set_guidance(i, dev(planes(hh, ww)))
            eng.set_targets_guided(i, c, s, dev(planes(sh, sw_)))
        return eng.luminance(dev(torch.from_numpy(cpu_ref_golden(JOBS["L1"][0])["x_img"])))

    try:
        u = setup(False)
        g_off, l_off = eng.closure(u, CW, SW, TVW)
        g_off, l_off = g_off.clone(), l_off.clone()
        u = setup(True)
        g_on, l_on = eng.closure(u, CW, SW, TVW)
        g_on, l_on = g_on.clone(), l_on.clone()
        per = eng.matting_losses().cpu().numpy()
        g_alone, _ = eng.closure(u, 0.0, 0.0, 0.0)      # (the Laplacian entry keeps its own weight: taken out below)
        rows_on = l_on.cpu().numpy()[:-1].reshape(2, 4)
        rows_off = l_off.cpu().numpy()[:-1].reshape(2, 4)
        assert np.all(per > 0) and np.isfinite(per).all()
        # the stated order: (row without the term) + gamma * mat, product and sum each rounded in float
        want = (rows_off[:, 0] + np.float32(gamma) * per.astype(np.float32)).astype(np.float32)
        assert np.array_equal(rows_on[:, 0].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(rows_on[:, 1:].view(np.uint32), rows_off[:, 1:].view(np.uint32))
        # one-plane value = the three-channel restatement at E(u)
        um = u.cpu().double()
        cu = eng.luminance(dev(torch.from_numpy(contents[0]))).cpu().double()
        v64 = float(mat_term(um.expand(-1, 3, -1, -1), (cu / 255.0).expand(-1, 3, -1, -1), EPS))
        assert abs(per[0] - v64) <= FLOOR * v64
        # additivity: g(on) = g(off) + g(mat alone); g(mat alone) = g(weights 0 with both pixel terms) - g(weights 0, Laplacian only)
        u2 = setup(False)
        g_lap, _ = eng.closure(u2, 0.0, 0.0, 0.0)
        s = g_off.cpu().numpy().astype(np.float64) + g_alone.cpu().numpy().astype(np.float64) - g_lap.cpu().numpy().astype(np.float64)
        add = float(np.linalg.norm(g_on.cpu().numpy().astype(np.float64) - s) / np.linalg.norm(s))
        # level sharding
        u = setup(True)
        g, l = eng.closure(u, CW, SW, TVW)
        g, l = g.cpu().numpy().astype(np.float64), l.cpu().numpy().astype(np.float64)
        gs, ls = np.zeros_like(g), np.zeros_like(l)
        for mask in (1, 2):
            gm, lm = eng.closure_levels(u, CW, SW, TVW, mask)
            pm = eng.matting_losses().cpu().numpy()
            own = 0 if mask == 1 else 1
            assert pm[own] == per[own] and pm[1 - own] == 0
            gs += gm.cpu().numpy()
            ls += lm.cpu().numpy()
        e = float(np.linalg.norm(gs - g) / np.linalg.norm(g))
        report(f"matting composition: mat {per}, term share {gamma * per / rows_on[:, 0]}, additivity {add:.1e}, "
               f"|sum of the ranks' gradients - unsharded| / |.| = {e:.1e}")
        assert add <= 2e-6
        np.testing.assert_allclose(ls, l, rtol=1e-6)
        assert e <= 2e-6
    finally:
        eng.configure(2, h, w)
        eng.reset_color()
        eng.reset_pooling()


# ---- 8. the public path ------------------------------------------------------------------------------------------------------------
def test_job_driver_with_the_matting_term(vgg_weights):
    """neural_style_transfer(..., matting_weight=g) on a 64x96 pair, two levels, three Adam steps: it yields images,
    matting_losses() is finite and positive, and the first yielded image differs from that of the same job without the term."""
    from artstyletransfer_amd import config, neural_nets
    from artstyletransfer_amd import neural_style_transfer as impl
    import neural_style_transfer as nst
    neural_nets.set_weights(vgg_weights)
    content = cpu_ref.synthetic_image(64, 96, seed=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=2, iters_num=3, optimizer="adam")
    real_step = impl._DeviceJob.step

    def run(**kw):
        first = {}

        def step(self, cw, sw, tvw):
            out = real_step(self, cw, sw, tvw)
            if "mat" not in first:
                with torch.cuda.stream(self.job_stream):
                    first["mat"] = self.engine.matting_losses().cpu().numpy()
                first["setting"] = self.engine.matting
            return out

        impl._DeviceJob.step = step

        async def go():
            out = []
            async for percent, img in nst.neural_style_transfer(
                    nst.ContentStylePair(("c", content), ("s", style)), cfg.content_weight, cfg.style_weight, cfg.tv_weight,
                    cfg.optimizer, cfg.model, "content", cfg.iters_num, cfg.levels_num, cfg.noise_factor,
                    cfg.noise_levels, cfg.noise_levels_central_amplitude, cfg.noise_levels_peripheral_amplitude,
                    cfg.noise_levels_dispersion, **kw):
                out.append((percent, img))
            return out

        try:
            return asyncio.run(go()), first
        finally:
            impl._DeviceJob.step = real_step

    out_mat, first = run(matting_weight=GAMMA)
    assert len(out_mat) == 3
    for _, img in out_mat:
        assert np.isfinite(img).all()
    assert first["setting"] == (GAMMA, 1e-7)
    assert first["mat"].shape == (2,) and np.isfinite(first["mat"]).all() and np.all(first["mat"] > 0)
    out_plain, first_plain = run()
    assert first_plain["setting"] is None and np.count_nonzero(first_plain["mat"]) == 0
    assert out_mat[0][1].shape == out_plain[0][1].shape
    assert not np.array_equal(out_mat[0][1], out_plain[0][1])
