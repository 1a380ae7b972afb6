"""GPU: spatial control - per-region styles through guided Gram matrices (nst_level_set_guidance,
nst_level_set_targets_guided), as include/nst_hip.h defines them:

    guidance of a map at network scale s = the level plane t_r passed s times through the 2x2/2 mean pool
    n_r = sum_p t_r(p)^2,   G_r = sum_p t_r(p)^2 F(p) F(p)^T / (C n_r)
    style term of a level = (sum_i w_i sum_r lambda_r MSE(G_ri, Gt_ri)) / nstyle

The reference is a torch restatement of those lines (`guided_targets`, `guided_closure`) on the CPU oracle's pieces
(vgg19_features, total_variation, bicubic_half), evaluated under the device pass's ReLU / pooling / TV-sign decisions, with
the Gram matrices formed in fp64.

Bounds (none taken from what the code under test gives): loss totals and rows 1e-5 relative (check_rows), gradient rel-L2
2e-5 under equal decisions (hip_helpers.BULK_RTOL); two DEVICE evaluations that must agree to rounding: rows 1e-6, gradient
1e-6 (test_hip_style_blend's level-sharding bound); guidance planes 1 ulp, masses 1e-6; what must be the same bits is
compared as bits.
Jobs: 50x76 one level; 64x96 two levels (a 2x3-pixel relu5_1 map on level 1); 68x260 three levels with style images of
other sizes (maps of 17x65, 34x130 ... pixels: pixel counts off the staging width of the Gram kernels, odd pooling sources)."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from hip_helpers import BULK_RTOL, CW, SW, TVW, check_rows, dev, levels as _levels, rel_l2, report
from test_hip_style_blend import _same_bits, avg_features, device_decisions

pytestmark = pytest.mark.gpu

MODES = {"f16x2": {}, "per_level": {"batched": False}, "bf16x3": {"conv_mode": "bf16x3"}, "f32": {"conv_mode": "f32"}}
DEFAULT = (4, (0, 1, 2, 3, 5))
TAPS_SHARED = (2, (2, 3))                # map 2 is the content map and a style map
MAP_SCALE = (0, 1, 2, 3, 3, 4)
ONES = (1.0,) * 6
W_MIXED = (1.0, 0.5, 0.0, 2.0, 1.0, 0.25)
GRAD_TOL = BULK_RTOL                     # 2e-5
LOSS_TOL = 1e-5
WEIGHTINGS = (("style", (0.0, SW, 0.0)), ("all", (CW, SW, TVW)))


# ---- engines and jobs, made once -------------------------------------------------------------------------------------
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


@pytest.fixture()
def eng(engines):
    e = engines("f16x2")
    yield e
    e.reset_style_weights()
    e.reset_taps()
    e.reset_color()
    e.reset_pooling()


class Job:
    def __init__(self, name, h, w, nlev, style_hw, seed):
        self.name, self.nlev = name, nlev
        self.c = _levels(h, w, nlev, seed)
        # (a style image per level, each of a size of its own whose relu5_1 map still has 3 x 4 pixels or more)
        self.s = [cpu_ref.synthetic_image(sh, sw, seed + 20 + k) for k, (sh, sw) in enumerate(style_hw)]
        self.x = cpu_ref.prepare_img((0.6 * self.c[0] + 0.4 * cpu_ref.synthetic_image(h, w, seed=seed + 7)).astype(np.float32))
        self.shapes = [tuple(c.shape[:2]) for c in self.c]
        self.style_shapes = [tuple(s.shape[:2]) for s in self.s]


@pytest.fixture(scope="module")
def jobs():
    made = {"50x76_L0": Job("50x76_L0", 50, 76, 1, [(48, 80)], 3),
            "64x96_L1": Job("64x96_L1", 64, 96, 2, [(64, 80), (48, 80)], 1),
            "68x260_L2": Job("68x260_L2", 68, 260, 3, [(100, 152), (50, 76), (48, 80)], 5)}
    return made


def mask_set(name, h, w):
    """(R,h,w) float32 planes at a master resolution; resized to every level by regions.resize_nearest."""
    xs = (np.arange(w, dtype=np.float32) + 0.5) / w
    ramp = np.broadcast_to(xs, (h, w)).astype(np.float32)
    rows = np.broadcast_to(((np.arange(h, dtype=np.float32) + 0.5) / h)[:, None], (h, w))
    if name == "halves":
        left = (ramp < 0.5).astype(np.float32)
        return np.stack([left, 1 - left])
    if name == "bands3":
        # thirds, but where the coarsest relu5_1 map is 1 x 4 pixels (68x260: level 2 is 17x65) or cuts the width off at 64
        # (50x76) the boundaries sit where every band still holds one whole pixel of that map: mass >= 1 everywhere
        f0, f2 = {260: (64 / 260, 192 / 260), 76: (0.3, 0.6)}.get(w, (1 / 3, 2 / 3))
        b0, b2 = ramp < f0, ramp >= f2
        return np.stack([b0, ~(b0 | b2), b2]).astype(np.float32)
    if name == "soft":
        return np.stack([ramp, 1 - ramp]).astype(np.float32)
    if name == "overlap":            # does not sum to 1
        return np.stack([0.5 + 0.5 * ramp, 0.9 - 0.6 * ramp]).astype(np.float32)
    if name == "zero_tiles":         # hard, each region zero over the other half of the (row-major) pixel range: whole staging chunks
        top = (rows < 0.5).astype(np.float32)
        return np.stack([top, 1 - top])
    raise KeyError(name)


MASK_SETS = ("halves", "bands3", "soft", "overlap", "zero_tiles")


def level_planes(job, name, style_indices):
    """Per-level content and style planes of a mask set, with the CPU assertion that every mass on every map in use is >= 1."""
    from artstyletransfer_amd import regions
    cm = mask_set(name, *job.shapes[0])
    sm = mask_set(name, *job.style_shapes[0])
    cp = [regions.resize_nearest(cm, *hw) for hw in job.shapes]
    sp = [regions.resize_nearest(sm, *hw) for hw in job.style_shapes]
    for t in cp + sp:
        m = regions.masses(t)
        for i in style_indices:
            assert (m[MAP_SCALE[i]] >= 1.0).all(), (job.name, name, t.shape, MAP_SCALE[i], m[MAP_SCALE[i]])
    return cp, sp


def _prep(img):
    return dev(cpu_ref.prepare_img(img))


def set_guided(e, job, cp, sp, lam=None):
    for l in range(job.nlev):
        e.set_guidance(l, dev(torch.from_numpy(cp[l])), lam)
        e.set_targets_guided(l, _prep(job.c[l]), _prep(job.s[l]), dev(torch.from_numpy(sp[l])))


def set_plain(e, job):
    for l in range(job.nlev):
        e.set_targets(l, _prep(job.c[l]), _prep(job.s[l]))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def pool_chain(t):
    """(R,h,w) torch -> the planes of the five network scales (F.avg_pool2d chain, floor sizes)."""
    out = [t]
    for _ in range(4):
        if min(out[-1].shape[1:]) < 2:
            break
        out.append(F.avg_pool2d(out[-1].unsqueeze(0), kernel_size=2, stride=2).squeeze(0))
    return out


def guided_gram(f, t):
    """G = sum_p t(p)^2 F(p) F(p)^T / (C n), n = sum_p t(p)^2, in fp64.  f: (1,C,h,w), t: (h,w)."""
    c = f.shape[1]
    fm = f[0].reshape(c, -1).double()
    t2 = t.reshape(-1).double() ** 2
    return (fm * t2) @ fm.t() / (c * t2.sum())


class Targets:
    pass


def guided_targets(content_t, style_t, style_planes, weights, taps=DEFAULT, feats=cpu_ref.vgg19_features):
    t = Targets()
    chain = pool_chain(torch.from_numpy(style_planes))
    with torch.no_grad():
        t.content = feats(content_t, weights)[taps[0]].squeeze(0)
        sf = feats(style_t, weights)
        t.grams = {i: [guided_gram(sf[i], chain[MAP_SCALE[i]][r]) for r in range(style_planes.shape[0])] for i in taps[1]}
    return t


def guided_closure(x, targets, planes, lam, weights, cw, sw, tvw, w6=ONES, taps=DEFAULT, decisions=None, feats=cpu_ref.vgg19_features):
    """cpu_ref.closure_eval with style = (sum_i w_i sum_r lambda_r MSE(G_ri, Gt_ri)) / nstyle: (total, gradient, rows)."""
    content_i, style_set = taps
    x = x.detach().clone().requires_grad_(True)
    lv, total, rows = [x], None, []
    for l, tg in enumerate(targets):
        if l > 0:
            lv.append(cpu_ref.bicubic_half(lv[l - 1]))
        dec = decisions[l] if decisions is not None else None
        f = feats(lv[l], weights, dec)
        chain = pool_chain(torch.from_numpy(planes[l]))
        content = F.mse_loss(tg.content, f[content_i].squeeze(0), reduction="mean")
        style = 0.0
        for i in style_set:
            for r in range(planes[l].shape[0]):
                g = guided_gram(f[i], chain[MAP_SCALE[i]][r])
                style = style + float(w6[i]) * float(lam[r]) * ((g - tg.grams[i][r]) ** 2).mean()
        style = (style / len(style_set)).float()
        tv = cpu_ref.total_variation(lv[l], dec.tv if dec is not None else None)
        t = cw * content + sw * style + tvw * tv
        total = t if total is None else 1.0 * total + t
        rows.append((float(t.detach()), float(content.detach()), float(style.detach()), float(tv.detach())))
    total.backward()
    return total.detach(), x.grad.detach(), rows


def held_to_restatement(e, job, targets, planes, lam, weights, what, w6=ONES, taps=DEFAULT, feats=cpu_ref.vgg19_features,
                        weightings=WEIGHTINGS):
    xd = dev(job.x)
    for name, (cw, sw, tvw) in weightings:
        grad, losses = e.closure(xd, cw, sw, tvw)
        dec = device_decisions(e, xd, weights, taps, feats)
        losses = losses.cpu().numpy()
        loss, g_ref, rows = guided_closure(job.x, targets, planes, lam, weights, cw, sw, tvw, w6, taps, dec, feats)
        e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
        e_g = rel_l2(grad.cpu().numpy(), g_ref.numpy())
        report(f"regions {what} [{name}]: total rel {e_l:.2e}, gradient rel-L2 under equal decisions {e_g:.2e}")
        print(f"regions {what} [{name}]: total rel {e_l:.2e}, gradient rel-L2 {e_g:.2e}")
        assert np.isfinite(losses).all()
        assert e_l < LOSS_TOL, (what, name, e_l)
        check_rows(losses[:-1].reshape(job.nlev, 4), np.array(rows), LOSS_TOL, cw, sw, tvw)
        assert e_g < GRAD_TOL, (what, name, e_g)


_target_cache = {}


def cached_targets(job, name, sp, weights, taps):
    key = (job.name, name, taps)
    if key not in _target_cache:
        _target_cache[key] = [guided_targets(cpu_ref.prepare_img(job.c[l]), cpu_ref.prepare_img(job.s[l]), sp[l], weights, taps)
                              for l in range(job.nlev)]
    return _target_cache[key]


# ---- 1. every mask set on every job, both schedules, two tap choices ----------------------------------------------------
@pytest.mark.parametrize("taps", [DEFAULT, TAPS_SHARED], ids=["default_taps", "c2_s23"])
@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
@pytest.mark.parametrize("name", MASK_SETS)
@pytest.mark.parametrize("jobname", ["50x76_L0", "64x96_L1", "68x260_L2"])
def test_guided_closure_vs_restatement(engines, vgg_weights, jobs, jobname, name, mode, taps):
    job = jobs[jobname]
    cp, sp = level_planes(job, name, taps[1])
    lam = (1.0, 0.5, 2.0)[:cp[0].shape[0]] if name == "bands3" else None
    e = engines(mode)
    try:
        e.configure(job.nlev, *job.shapes[0])
        e.set_taps(*taps)
        set_guided(e, job, cp, sp, lam)
        tg = cached_targets(job, name, sp, vgg_weights, taps)
        held_to_restatement(e, job, tg, cp, lam or (1.0,) * cp[0].shape[0], vgg_weights, f"{jobname} {name} {mode}", taps=taps)
    finally:
        e.reset_taps()


# ---- 2, 3. guidance that is no guidance -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
@pytest.mark.parametrize("case", ["R1_ones", "R2_ones_halved"])
def test_all_ones_guidance_is_the_unguided_closure(engines, jobs, mode, case):
    job = jobs["64x96_L1"]
    e = engines(mode)
    x = dev(job.x)
    e.configure(job.nlev, *job.shapes[0])
    set_plain(e, job)
    g_ref, l_ref = (t.clone() for t in e.closure(x, CW, SW, TVW))
    r, lam = (1, None) if case == "R1_ones" else (2, (0.5, 0.5))
    cp = [np.ones((r, *hw), np.float32) for hw in job.shapes]
    sp = [np.ones((r, *hw), np.float32) for hw in job.style_shapes]
    set_guided(e, job, cp, sp, lam)
    g, l = e.closure(x, CW, SW, TVW)
    e_g = rel_l2(g.cpu().numpy(), g_ref.cpu().numpy())
    e_l = float(np.max(np.abs(l.cpu().numpy() - l_ref.cpu().numpy()) / np.abs(l_ref.cpu().numpy())))
    print(f"regions {case} {mode}: rows rel {e_l:.2e}, gradient rel-L2 {e_g:.2e}")
    np.testing.assert_allclose(l.cpu().numpy(), l_ref.cpu().numpy(), rtol=LOSS_TOL)
    assert e_g < GRAD_TOL


# ---- 4. pyramid and masses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jobname", ["50x76_L0", "68x260_L2"])
def test_guidance_pyramid_and_masses(eng, jobs, jobname):
    job = jobs[jobname]
    cp, _ = level_planes(job, "overlap", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    for l in range(job.nlev):
        eng.set_guidance(l, dev(torch.from_numpy(cp[l])), (1.0, 0.25))
        r, lam, mass = eng.guidance(l)
        assert r == 2 and lam == (1.0, 0.25)
        chain = pool_chain(torch.from_numpy(cp[l]))
        assert len(chain) == 5
        for s, ref in enumerate(chain):
            got = eng.guidance_planes(l, s).cpu()
            assert got.shape == ref.shape
            ulp = np.spacing(np.abs(ref.numpy()).astype(np.float32))
            assert (np.abs(got.numpy() - ref.numpy()) <= ulp).all(), (l, s)
            want = (got.double() ** 2).sum(dim=(1, 2)).numpy()
            np.testing.assert_allclose(mass[s], want, rtol=1e-6)
            np.testing.assert_allclose(mass[s], (ref.double() ** 2).sum(dim=(1, 2)).numpy(), rtol=1e-6)
    eng.clear_guidance()
    assert eng.guidance(0)[0] == 0


# ---- 5. set, then cleared: today's bits and today's launches -----------------------------------------------------------------
def _launch_list(e, x):
    e.set_timing(2)
    try:
        e.closure(x, CW, SW, TVW)
        torch.cuda.synchronize()
        return e.last_closure_launches()
    finally:
        e.set_timing(0)


@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
def test_cleared_guidance_is_bitwise_the_plain_closure(engines, jobs, mode):
    job = jobs["64x96_L1"]
    e = engines(mode)
    x = dev(job.x)
    e.configure(job.nlev, *job.shapes[0])
    set_plain(e, job)
    g_ref, l_ref = (t.clone() for t in e.closure(x, CW, SW, TVW))
    launches_ref = _launch_list(e, x)
    cp, sp = level_planes(job, "soft", DEFAULT[1])
    set_guided(e, job, cp, sp)
    launches_guided = _launch_list(e, x)
    assert len(launches_guided) > len(launches_ref)
    assert not any(la["h2_second"] for la in launches_guided)       # no conv launch of a guided job carries a second K source
    e.clear_guidance()
    g, l = e.closure(x, CW, SW, TVW)
    assert _same_bits(g, g_ref) and _same_bits(l, l_ref)
    assert _launch_list(e, x) == launches_ref


# ---- 6. run to run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x2", "per_level"])
def test_guided_closure_is_bitwise_reproducible(engines, jobs, mode):
    job = jobs["68x260_L2"]
    e = engines(mode)
    x = dev(job.x)
    cp, sp = level_planes(job, "overlap", DEFAULT[1])
    e.configure(job.nlev, *job.shapes[0])
    set_guided(e, job, cp, sp, (1.0, 0.5))
    g0, l0 = (t.clone() for t in e.closure(x, CW, SW, TVW))
    for _ in range(2):
        g, l = e.closure(x, CW, SW, TVW)
        assert _same_bits(g, g0) and _same_bits(l, l0)
    # the two halves are the whole
    if mode == "f16x2":
        lf = e.closure_forward(x, CW, SW, TVW).clone()
        gb = e.closure_backward(x, CW, SW, TVW)
        assert _same_bits(lf, l0) and _same_bits(gb, g0)


# ---- 7. composition ------------------------------------------------------------------------------------------------------------
def test_guidance_under_avg_pooling_and_layer_weights(eng, vgg_weights, jobs):
    job = jobs["64x96_L1"]
    cp, sp = level_planes(job, "soft", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    eng.set_pooling("avg")
    eng.set_style_weights(W_MIXED)
    set_guided(eng, job, cp, sp, (0.5, 1.5))
    tg = [guided_targets(cpu_ref.prepare_img(job.c[l]), cpu_ref.prepare_img(job.s[l]), sp[l], vgg_weights, feats=avg_features)
          for l in range(job.nlev)]
    held_to_restatement(eng, job, tg, cp, (0.5, 1.5), vgg_weights, "avg pooling + layer weights", W_MIXED, feats=avg_features,
                        weightings=WEIGHTINGS[1:])


def test_guidance_with_layer_weights(eng, vgg_weights, jobs):
    job = jobs["64x96_L1"]
    cp, sp = level_planes(job, "halves", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    eng.set_style_weights(W_MIXED)
    set_guided(eng, job, cp, sp)
    tg = cached_targets(job, "halves", sp, vgg_weights, DEFAULT)
    held_to_restatement(eng, job, tg, cp, (1.0, 1.0), vgg_weights, "layer weights", W_MIXED, weightings=WEIGHTINGS[1:])


def test_guidance_in_luminance_mode(eng, vgg_weights, jobs):
    """One plane u: the closure is the RGB restatement at E(u) = u - mean_c, the gradient summed over the channels."""
    from artstyletransfer_amd import host_image
    mean = torch.tensor(cpu_ref.IMAGENET_MEAN_255, dtype=torch.float32).view(1, 3, 1, 1)
    E = lambda u: u.reshape(1, 1, *u.shape[-2:]).float().cpu() - mean      # noqa: E731
    lum = lambda img: torch.from_numpy(host_image.luminance(img))           # noqa: E731
    job = jobs["64x96_L1"]
    cp, sp = level_planes(job, "soft", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    eng.set_color("luminance")
    for l in range(job.nlev):
        eng.set_guidance(l, dev(torch.from_numpy(cp[l])))
        eng.set_targets_guided(l, dev(lum(job.c[l])), dev(lum(job.s[l])), dev(torch.from_numpy(sp[l])))
    tg = [guided_targets(E(lum(job.c[l])), E(lum(job.s[l])), sp[l], vgg_weights) for l in range(job.nlev)]
    u = lum((0.6 * job.c[0] + 0.4 * cpu_ref.synthetic_image(64, 96, seed=9)).astype(np.float32)).reshape(1, 1, 64, 96)
    ud = dev(u)
    grad, losses = eng.closure(ud, CW, SW, TVW)
    assert tuple(grad.shape) == (1, 1, 64, 96)
    dec = device_decisions(eng, ud, vgg_weights, expand=E)
    loss, g_ref, rows = guided_closure(E(u), tg, cp, (1.0, 1.0), vgg_weights, CW, SW, TVW, decisions=dec)
    losses = losses.cpu().numpy()
    e_g = rel_l2(grad.cpu().numpy().reshape(64, 96), g_ref.sum(dim=1).numpy().reshape(64, 96))
    print(f"regions luminance: total rel {abs(float(losses[-1]) - float(loss)) / float(loss):.2e}, gradient rel-L2 {e_g:.2e}")
    assert float(losses[-1]) == pytest.approx(float(loss), rel=LOSS_TOL)
    check_rows(losses[:-1].reshape(2, 4), np.array(rows), LOSS_TOL)
    assert e_g < GRAD_TOL


# ---- 8. level sharding -------------------------------------------------------------------------------------------------------
def test_level_sharded_guided_closure_adds_up(eng, jobs):
    job = jobs["68x260_L2"]
    x = dev(job.x)
    cp, sp = level_planes(job, "bands3", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    set_guided(eng, job, cp, sp, (1.0, 0.5, 2.0))
    g, l = (t.clone() for t in eng.closure(x, CW, SW, TVW))
    parts = [tuple(t.clone() for t in eng.closure_levels(x, CW, SW, TVW, m)) for m in (0b001, 0b110)]
    assert rel_l2((parts[0][0] + parts[1][0]).cpu().numpy(), g.cpu().numpy()) < 1e-6
    rows = l.cpu().numpy()[:-1].reshape(3, 4)
    np.testing.assert_allclose(parts[0][1].cpu().numpy()[:4], rows[0], rtol=1e-6)
    np.testing.assert_allclose(parts[1][1].cpu().numpy()[4:12].reshape(2, 4), rows[1:], rtol=1e-6)
    assert not parts[0][1].cpu().numpy()[4:12].any() and not parts[1][1].cpu().numpy()[:4].any()


# ---- 9. staleness ----------------------------------------------------------------------------------------------------------
def test_backward_half_is_stale_after_set_guidance(eng, jobs):
    from artstyletransfer_amd import _lib
    job = jobs["64x96_L1"]
    x = dev(job.x)
    cp, sp = level_planes(job, "soft", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    set_guided(eng, job, cp, sp)
    g_ref, _ = eng.closure(x, CW, SW, TVW)
    g_ref = g_ref.clone()
    grad = torch.full_like(g_ref, -7.0)
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_guidance(1, dev(torch.from_numpy(cp[1])))              # even the same planes
    rc = eng.lib.nst_closure_backward(eng.ctx, C.c_void_p(x.data_ptr()), CW, SW, TVW, 0xFFFFFFFF, C.c_void_p(grad.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.NST_E_STATE and bool((grad == -7.0).all())
    # the guided targets survived planes of the same R, and the context goes on working
    g, _ = eng.closure(x, CW, SW, TVW)
    assert _same_bits(g, g_ref)


def test_guidance_change_between_lbfgs_steps_forces_an_evaluation(eng, vgg_weights, jobs):
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine
    job = jobs["64x96_L1"]
    cp, sp = level_planes(job, "soft", DEFAULT[1])
    cp2, _ = level_planes(job, "overlap", DEFAULT[1])
    eng.configure(job.nlev, *job.shapes[0])
    set_guided(eng, job, cp, sp)
    x = dev(job.x).clone()
    opt = PixelOptimizer(eng, "lbfgs", 10.0, 1)
    try:
        opt.step(x, CW, SW, TVW)
        before = opt.closure_stats()
        opt.step(x, CW, SW, TVW)
        ev, sv = opt.closure_stats()
        assert sv == before[1] + 1                         # nothing changed: the first closure of the step was served
        for l in range(job.nlev):
            eng.set_guidance(l, dev(torch.from_numpy(cp2[l])))
        x_at = x.clone()
        info, rows = opt.step(x, CW, SW, TVW)
        ev2, sv2 = opt.closure_stats()
        assert sv2 == sv and ev2 > ev                      # evaluated, not served
    finally:
        opt.close()
    fresh = StyleEngine(vgg_weights, 0)
    try:
        fresh.configure(job.nlev, *job.shapes[0])
        set_guided(fresh, job, cp2, sp)
        _, l = fresh.closure(x_at, CW, SW, TVW)
        assert np.array_equal(np.asarray(rows[0], np.float32).view(np.uint32), l.cpu().numpy().view(np.uint32))
        assert info.loss == float(l[-1])
    finally:
        fresh.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(engines, vgg_weights, jobs):
    from artstyletransfer_amd import _lib
    from artstyletransfer_amd._lib import NstError
    from artstyletransfer_amd.engine import PixelOptimizer, StyleEngine
    job = jobs["64x96_L1"]
    e = engines("f16x2")
    x = dev(job.x)
    cp, sp = level_planes(job, "soft", DEFAULT[1])
    e.configure(job.nlev, *job.shapes[0])
    set_guided(e, job, cp, sp)
    g_ref, l_ref = (t.clone() for t in e.closure(x, CW, SW, TVW))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def guidance(level, planes, lam=None):
        t = dev(torch.from_numpy(np.ascontiguousarray(planes, np.float32)))
        lam = (C.c_float * len(lam))(*lam) if lam is not None else None
        return e.lib.nst_level_set_guidance(e.ctx, level, planes.shape[0], C.c_void_p(t.data_ptr()), lam, stream)

    def unchanged():
        g, l = e.closure(x, CW, SW, TVW)
        return _same_bits(g, g_ref) and _same_bits(l, l_ref)

    h, w = job.shapes[0]
    bad = cp[0].copy(); bad[0, 3, 5] = 1.5
    assert guidance(0, bad) == _lib.NST_E_ARG and unchanged()
    bad[0, 3, 5] = -0.25
    assert guidance(0, bad) == _lib.NST_E_ARG and unchanged()
    bad[0, 3, 5] = np.nan
    assert guidance(0, bad) == _lib.NST_E_ARG and unchanged()
    assert guidance(0, np.ones((5, h, w), np.float32)) == _lib.NST_E_ARG and unchanged()
    thin = np.zeros((2, h, w), np.float32); thin[0] = 1.0; thin[1, :4, :4] = 1.0      # 16 pixels: 1/16 of a relu5_1 pixel
    assert guidance(0, thin) == _lib.NST_E_ARG and "mass" in e.lib.nst_last_error(e.ctx).decode() and unchanged()
    assert guidance(0, cp[0], (0.0, 0.0)) == _lib.NST_E_ARG and guidance(0, cp[0], (1.0, -1.0)) == _lib.NST_E_ARG and unchanged()
    # the style side: a region without mass
    hs, ws = job.style_shapes[0]
    sthin = np.zeros((2, hs, ws), np.float32); sthin[0] = 1.0; sthin[1, :4, :4] = 1.0
    with pytest.raises(NstError, match=r"\(-1\).*mass"):
        e.set_targets_guided(0, _prep(job.c[0]), _prep(job.s[0]), dev(torch.from_numpy(sthin)))
    assert unchanged()
    # a blend of several style images on a guided level
    with pytest.raises(NstError, match=r"\(-2\)"):
        e.set_targets_blend(0, _prep(job.c[0]), [_prep(job.s[0]), _prep(job.s[1])], [0.5, 0.5])
    assert unchanged()
    # guided and unguided levels in one closure
    e.set_guidance(1, None)
    e.set_targets(1, _prep(job.c[1]), _prep(job.s[1]))
    with pytest.raises(NstError, match=r"\(-2\).*all guided or all unguided"):
        e.closure(x, CW, SW, TVW)
    e.set_guidance(1, dev(torch.from_numpy(cp[1])))
    with pytest.raises(NstError, match=r"\(-2\).*guided targets of level 1"):
        e.closure(x, CW, SW, TVW)
    e.set_targets_guided(1, _prep(job.c[1]), _prep(job.s[1]), dev(torch.from_numpy(sp[1])))
    assert unchanged()
    # the other arithmetic modes
    for mode in ("bf16x3", "f32"):
        o = engines(mode)
        o.configure(job.nlev, *job.shapes[0])
        set_plain(o, job)
        g0, _ = o.closure(x, CW, SW, TVW)
        g0 = g0.clone()
        with pytest.raises(NstError, match=r"\(-2\).*f16x2"):
            o.set_guidance(0, dev(torch.from_numpy(cp[0])))
        g1, _ = o.closure(x, CW, SW, TVW)
        assert _same_bits(g0, g1)
    # the stripe closure
    s = StyleEngine(vgg_weights, 0)
    try:
        s.configure(1, 64, 96)
        s.set_guidance(0, dev(torch.from_numpy(cp[0])))
        s.set_targets_guided(0, _prep(job.c[0]), _prep(job.s[0]), dev(torch.from_numpy(sp[0])))
        s.set_targets(0, _prep(job.c[0]), _prep(job.s[0]))
        with pytest.raises(NstError, match=r"\(-2\).*spatial control"):
            s.window_begin(x, 0, 64, 64)
        opt = PixelOptimizer(s, "adam", 10.0)
        try:
            with pytest.raises(ValueError):
                opt.shard_stripes(0, 1, vgg_weights, _prep(job.c[0]), _prep(job.s[0]))
        finally:
            opt.close()
        s.set_guidance(0, None)
        sums = s.window_begin(x, 0, 64, 64)
        _, lw = s.window_end(x, 0, 64, 64, CW, SW, TVW, sums)
        assert np.isfinite(lw.cpu().numpy()).all()
    finally:
        s.close()


def test_pooled_engine_comes_back_without_guidance(vgg_weights, jobs):
    from artstyletransfer_amd import neural_nets
    job = jobs["50x76_L0"]
    neural_nets.set_weights(vgg_weights)
    e = neural_nets.lease_engine(torch.device("cuda", 0))
    e.configure(1, 50, 76)
    cp, _ = level_planes(job, "halves", DEFAULT[1])
    e.set_guidance(0, dev(torch.from_numpy(cp[0])))
    assert e.guidance(0)[0] == 2
    neural_nets.return_engine(e)
    again = neural_nets.lease_engine(torch.device("cuda", 0))
    try:
        assert again is e and again.guidance(0)[0] == 0
    finally:
        neural_nets.return_engine(again)


# ---- 11. the job driver ---------------------------------------------------------------------------------------------------------
def test_job_driver_with_label_maps(vgg_weights):
    """Three Adam steps from 64x96 images with two levels (512x768 + 256x384) and label maps: finite, the guided loss of the
    yielded images decreasing, the percent sequence of an unguided job."""
    from artstyletransfer_amd import config, device_image, neural_nets, regions
    from artstyletransfer_amd.engine import StyleEngine
    import neural_style_transfer as nst
    neural_nets.set_weights(vgg_weights)
    content = cpu_ref.synthetic_image(64, 96, seed=1)
    style = cpu_ref.synthetic_image(50, 76, seed=2)
    cfg = config.Config(levels_num=2, iters_num=3, optimizer="adam")
    c_labels = (np.arange(96)[None, :] >= 48).astype(np.int64) * np.ones((64, 1), np.int64)
    s_labels = (np.arange(50)[:, None] >= 25).astype(np.int64) * np.ones((1, 76), np.int64)

    def run(**kw):
        async def go():
            out = []
            async for percent, img in nst.neural_style_transfer(
                    nst.ContentStylePair(("c", content), ("s", style)), cfg.content_weight, cfg.style_weight, cfg.tv_weight,
                    cfg.optimizer, cfg.model, "content+noise", cfg.iters_num, cfg.levels_num, cfg.noise_factor,
                    cfg.noise_levels, cfg.noise_levels_central_amplitude, cfg.noise_levels_peripheral_amplitude,
                    cfg.noise_levels_dispersion, **kw):
                out.append((percent, img))
            return out
        return asyncio.run(go())

    guided = run(content_regions=c_labels, style_regions=s_labels, region_weights=(1.0, 0.5))
    plain = run()
    assert [p for p, _ in guided] == [p for p, _ in plain] and round(guided[-1][0]) == 100
    for _, img in guided:
        assert img.shape == (512, 768, 3) and np.isfinite(img).all()
    assert np.abs(guided[-1][1] - plain[-1][1]).max() > 1e-3
    # the guided loss of the yielded images, by an engine set up as the job's was
    e = StyleEngine(vgg_weights, 0)
    try:
        cl = device_image.pyramid(e, device_image.upload(e, content), 2)
        sl = device_image.pyramid(e, device_image.upload(e, style), 2)
        cs, ss, lam = regions.check_regions(c_labels, s_labels, (1.0, 0.5))
        e.configure(2, 512, 768)
        for l in range(2):
            e.set_guidance(l, dev(torch.from_numpy(regions.resize_nearest(cs, *cl[l].shape[:2]))), lam)
            e.set_targets_guided(l, e.prepare_img(cl[l]), e.prepare_img(sl[l]),
                                 dev(torch.from_numpy(regions.resize_nearest(ss, *sl[l].shape[:2]))))
        totals = []
        for _, img in guided:
            _, l = e.closure(e.prepare_img(dev(torch.from_numpy(img))), cfg.content_weight, cfg.style_weight, cfg.tv_weight)
            totals.append(float(l[-1]))
        print("regions driver totals", totals)
        assert np.isfinite(totals).all() and totals[-1] < totals[0]
    finally:
        e.close()
