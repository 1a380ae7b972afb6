"""GPU: the Gram pass against fp64 per 32 x 32 block, tile pair and row - on inputs that are zero outside a pixel window.

The pixel axis is the K axis of a Gram, so a defect in one chunk, one k-step, one split or one slab of the finish pass is
diluted by every other chunk of a whole map: the whole-matrix bounds the suite had (rel-L2 < 2e-6, rtol 1e-4) pass a launch
that drops the 2^-11-weighted cross products of a k-step in a block (tests/test_gram_local_host.py shows it on the CPU model).
A map that is zero outside [p0, p1) makes the window's chunks the whole sum.  tests/gram_local.py has the statistic, the split
rule restated and the window plan; tests/test_gram_local_host.py proves what the plan reaches on the shapes used here and that
the model's planted defects stand 35x and more above the bound.  Every comparison here: fp64 truth and torch-fp32 yardstick
on the CPU from the same fp32 input, the device within max(4 x torch-fp32's statistic, 5e-7) in every family; the plan is built
from the geometry the DEVICE reports (nst_gram_batch), which must be the restated rule's.

Engines: the default (packed), gram_pack = False, and conv_mode = "f32" (nst_gram's fp32 gram_partial_kernel there).
Consecutive calls use different windows: what a workgroup that never ran would leave in the workspace is another window's."""
import numpy as np
import pytest
import torch

import gram_local as gl
from hip_helpers import dev, report
from local_accuracy import FACTOR, FLOOR, MAX_FACTOR
from test_gram_local_host import FORM_SHAPES, SHAPES, SLAB_SHAPES

pytestmark = pytest.mark.gpu

E_ARG = -1
_ids = lambda v: "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


@pytest.fixture(scope="module")
def engines(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = {"packed": StyleEngine(vgg_weights, 0), "switch-off": StyleEngine(vgg_weights, 0, gram_pack=False),
         "f32": StyleEngine(vgg_weights, 0, conv_mode="f32")}
    assert e["packed"].lib.nst_ctx_gram_pack(e["packed"].ctx) == 1 and e["switch-off"].lib.nst_ctx_gram_pack(e["switch-off"].ctx) == 0
    assert e["f32"].conv_mode() == "f32" and e["packed"].conv_mode() == "f16x2"
    yield e
    for x in e.values():
        x.close()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _windowed(fd, p0, p1):
    """the device map with every pixel outside [p0, p1) zeroed"""
    c = fd.shape[1]
    out = torch.zeros_like(fd)
    out[0].view(c, -1)[:, p0:p1] = fd[0].view(c, -1)[:, p0:p1]
    return out


class Ledger:
    """Collects the failures of a test (one run names every window that is off) and, per (engine, form), every family's
    worst ratio to torch-fp32, worst multiple of the bound and largest statistic - reported at the end of the test."""

    def __init__(self, test):
        self.test, self.failures, self.worst = test, [], {}

    def hold(self, key, got, ref64, ref32, what, **kw):
        try:
            out = gl.assert_gram_locally_as_accurate(got, ref64, ref32, what, **kw)
        except AssertionError as err:
            self.failures.append(str(err))
            out = {fam: (gl.gram_stats(got, ref64, kw.get("scale"))[fam][0], gl.gram_stats(ref32, ref64, kw.get("scale"))[fam][0])
                   for fam in ("matrix",) + gl.FAMILIES}
        w = self.worst.setdefault(key, {})
        for fam, (d, t) in out.items():
            r, m, a = w.get(fam, (0.0, 0.0, 0.0))
            w[fam] = (max(r, d / t if t > 0 else 0.0), max(m, d / max(kw.get("factor", FACTOR) * t, kw.get("floor", FLOOR))), max(a, d))
        return out

    def note(self, cond, what):
        if not cond:
            self.failures.append(what)

    def close(self):
        for (engine, form), w in sorted(self.worst.items()):
            report(f"gram local summary [{self.test}] {engine} / {form}: " + ", ".join(
                f"{fam} worst {r:.2f}x torch-fp32, {m:.2f} of the bound, largest {a:.2e}" for fam, (r, m, a) in w.items()))
        assert not self.failures, "\n".join(self.failures)


def _device_geometry(eng, fd, C, N):
    """what the launcher used for a lone map - and it is the restated rule's"""
    out = eng.gram_batch([fd])[0]
    geo = (out["nsplit"], out["pix_per_split"])
    assert geo == gl.geometry(C, N), (C, N, geo, gl.geometry(C, N))
    return geo


# ---- 1. lone maps: every window of the plan --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lone_maps_on_every_window_of_the_plan(engines, shape):
    """eng.gram on the whole map and on every window of the plan: every family within the bound, G exactly symmetric, packed and
    switch-off bitwise equal.  Measured (profiles/gram_local.txt), worst family as a multiple of torch-fp32's / largest
    statistic: packed and switch-off (bitwise equal) 4.05x / 3.04e-07 in the rows family - one-pixel windows, where torch-fp32's
    own error is 1e-8 ... 7e-8 and the floor is the bound: 0.56 of the bound at most -, blocks 3.58x / 1.84e-07, tile pairs and
    the whole matrix 2.93x / 1.06e-07; f32 1.00x / 2.57e-07 (rows: the fp32 kernel adds in torch's order on these inputs)."""
    c, h, w = shape
    N, div = h * w, float(c * h * w)
    f = gl.feature_map(c, h, w)
    F, fd = gl.pixel_major(f), dev(f)
    ns, pps = _device_geometry(engines["packed"], fd, c, N)
    assert _device_geometry(engines["switch-off"], fd, c, N) == (ns, pps)
    led = Ledger(f"lone maps C={c} {h}x{w}")
    for name, p0, p1 in [("whole map", 0, N)] + gl.window_plan(c, N, ns, pps):
        ref64, ref32 = gl.window_truths(F, p0, p1, div)
        fw = fd if (p0, p1) == (0, N) else _windowed(fd, p0, p1)
        outs = {k: e.gram(fw) for k, e in engines.items()}
        for k, g in outs.items():
            led.hold((k, "plain"), g.cpu(), ref64, ref32, f"{k} C={c} {h}x{w} plain [{p0},{p1}) {name}")
            led.note(torch.equal(g[0], g[0].t()), f"{k} C={c} {h}x{w} [{p0},{p1}) {name}: G is not symmetric")
        led.note(np.array_equal(_bits(outs["packed"]), _bits(outs["switch-off"])), f"C={c} {h}x{w} [{p0},{p1}) {name}: packed != switch-off")
    led.close()


# ---- 2. slab positions of the finish pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SLAB_SHAPES, ids=_ids)
def test_a_window_in_each_slab_class_of_the_finish_pass(engines, shape):
    """One whole-split window in slab 0 ... 7 (the 8 lane groups), in the first slab of the 64-at-a-time loop past them, in the
    first of the 32-at-a-time tail and in the last slab: the result is the window's Gram whichever slab held it.  Measured:
    every engine at most 1.00x torch-fp32 in every family (f16x2 0.35x ... 0.93x), 0.25 of the bound, largest 2.92e-07."""
    c, h, w = shape
    N, div = h * w, float(c * h * w)
    f = gl.feature_map(c, h, w)
    F, fd = gl.pixel_major(f), dev(f)
    ns, pps = _device_geometry(engines["packed"], fd, c, N)
    led = Ledger(f"slab positions C={c} {h}x{w}, {ns} slabs")
    for name, p0, p1 in gl.slab_plan(c, N, ns, pps):
        ref64, ref32 = gl.window_truths(F, p0, p1, div)
        fw = _windowed(fd, p0, p1)
        outs = {k: e.gram(fw) for k, e in engines.items()}
        for k, g in outs.items():
            led.hold((k, "plain"), g.cpu(), ref64, ref32, f"{k} C={c} {h}x{w} ({ns} slabs) [{p0},{p1}) {name}")
            led.note(torch.equal(g[0], g[0].t()), f"{k} C={c} {h}x{w} {name}: G is not symmetric")
        led.note(np.array_equal(_bits(outs["packed"]), _bits(outs["switch-off"])), f"C={c} {h}x{w} {name}: packed != switch-off")
    led.close()


# ---- 3. the shifted form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FORM_SHAPES, ids=_ids)
def test_shifted_and_centred_forms_on_the_ragged_windows(engines, shape):
    """eng.gram_shifted with a constant shift and centred, whole map and the ragged windows.  Truth: (F + o)(F + o)^T in double
    with the device's own o for the centred case (held to the fp64 means to 1e-6, as test_hip_gram_shift.py does) - the
    window's zero pixels inside [0, N) contribute o o^T, the staged pixels behind N nothing.  Measured: shift -1 at most 1.10x
    torch-fp32 (largest 7.20e-08: o o^T over N pixels dominates), centred at most 2.68x / 3.58e-07 (rows, 0.67 of the bound)."""
    c, h, w = shape
    N, div = h * w, float(c * h * w)
    f = gl.feature_map(c, h, w)
    F, fd = gl.pixel_major(f), dev(f)
    ns, pps = _device_geometry(engines["packed"], fd, c, N)
    assert N % gl.gram_kp(c) and N % 8
    led = Ledger(f"shifted form C={c} {h}x{w}")
    wins = [("whole map", 0, N)] + [x for x in gl.window_plan(c, N, ns, pps) if x[0].startswith(("ragged", "last"))]
    for name, p0, p1 in wins:
        fw = fd if (p0, p1) == (0, N) else _windowed(fd, p0, p1)
        for form, kw in (("shift -1", dict(shift=-1.0)), ("centred", dict(center=True))):
            outs = {k: engines[k].gram_shifted(fw, **kw) for k in ("packed", "switch-off")}
            for k, (g, o) in outs.items():
                o = o.cpu()
                o_ref = -F[p0:p1].double().sum(dim=0) / N if "center" in kw else torch.full((c,), -1.0, dtype=torch.float64)
                led.note(float((o.double() - o_ref).abs().max()) <= 1e-6, f"{k} C={c} {h}x{w} {form} {name}: offsets off")
                ref64, ref32 = gl.window_truths(F, p0, p1, div, o=o)
                led.hold((k, form), g.cpu(), ref64, ref32, f"{k} C={c} {h}x{w} {form} [{p0},{p1}) {name}")
                led.note(torch.equal(g[0], g[0].t()), f"{k} C={c} {h}x{w} {form} {name}: G is not symmetric")
            led.note(np.array_equal(_bits(outs["packed"][0]), _bits(outs["switch-off"][0])), f"C={c} {h}x{w} {form} {name}: packed != switch-off")
    led.close()


# ---- 4. the guided form ---------------------------------------------------------------------------------------------------------
def _soft_plane(h, w):
    t = torch.full((h, w), 0.7)
    t[:, : w // 2] = 0.9
    return t


def _window_plane(h, w, p0, p1):
    t = torch.zeros(h * w)
    t[p0:p1] = 1.0
    return t.view(h, w)


@pytest.mark.parametrize("shape", FORM_SHAPES, ids=_ids)
def test_guided_form_batch_of_one(engines, shape):
    """nst_gram_batch, n = 1, guided: a soft 0.9 / 0.7 plane, and planes that are 1 on a window of the plan and 0 elsewhere over
    the FULL map - the window trick done by t, so the operand's absmax comes from outside the window.  Truth: sum_p t(p)^2 F F^T
    in double.  Measured: at most 3.59x torch-fp32 / 3.04e-07 (rows, 0.53 of the bound), blocks 2.34x, whole matrix 2.47x."""
    c, h, w = shape
    N, div = h * w, float(c * h * w)
    f = gl.feature_map(c, h, w)
    F, fd = gl.pixel_major(f), dev(f)
    ns, pps = _device_geometry(engines["packed"], fd, c, N)
    led = Ledger(f"guided form, n = 1, C={c} {h}x{w}")
    cases = [("0.9/0.7", _soft_plane(h, w), (0, N))] + [(f"window plane {name}", _window_plane(h, w, p0, p1), (p0, p1))
                                                        for name, p0, p1 in gl.window_plan(c, N, ns, pps)]
    for name, t, (p0, p1) in cases:
        ref64, ref32 = gl.window_truths(F, p0, p1, div, t=t.reshape(-1))
        outs = {k: engines[k].gram_batch([fd], guides=[dev(t)])[0] for k in ("packed", "switch-off")}
        for k, out in outs.items():
            led.note((out["nsplit"], out["pix_per_split"]) == (ns, pps), f"{k} C={c} {h}x{w} guided {name}: geometry {out['nsplit']}, {out['pix_per_split']}")
            led.hold((k, "guided"), out["G"].cpu(), ref64, ref32, f"{k} C={c} {h}x{w} guided [{p0},{p1}) {name}")
            led.note(torch.equal(out["G"][0], out["G"][0].t()), f"{k} C={c} {h}x{w} guided {name}: G is not symmetric")
        led.note(np.array_equal(_bits(outs["packed"]["G"]), _bits(outs["switch-off"]["G"])), f"C={c} {h}x{w} guided {name}: packed != switch-off")
    led.close()


def test_guided_form_batch_of_two(engines):
    """n = 2, guided: two sizes of one channel count (the smaller with fewer splits than alone) with soft planes, then a
    64-wide and a 128-wide item with window planes on their ragged ends."""
    led = Ledger("guided form, n = 2")
    for shapes, kind in (([(256, 50, 61), (256, 25, 30)], "soft"), ([(64, 23, 37), (128, 17, 9)], "tail")):
        maps = [gl.feature_map(*s) for s in shapes]
        items = [(s[0], s[1] * s[2]) for s in shapes]
        planes, wins = [], []
        for (c, h, w) in shapes:
            N = h * w
            if kind == "soft":
                planes.append(_soft_plane(h, w))
                wins.append((0, N))
            else:
                planes.append(_window_plane(h, w, N - N % 8 - 8, N))
                wins.append((N - N % 8 - 8, N))
        fds = [dev(m) for m in maps]
        outs = {k: engines[k].gram_batch(fds, guides=[dev(t) for t in planes]) for k in ("packed", "switch-off")}
        for i, (c, h, w) in enumerate(shapes):
            ref64, ref32 = gl.window_truths(gl.pixel_major(maps[i]), *wins[i], float(c * h * w), t=planes[i].reshape(-1))
            for k in outs:
                out = outs[k][i]
                led.note((out["nsplit"], out["pix_per_split"]) == gl.geometry(*items[i], items, i), f"{k} item {i} of {shapes}: geometry")
                led.hold((k, "guided"), out["G"].cpu(), ref64, ref32, f"{k} C={c} {h}x{w} guided {kind}, item {i} of 2")
            led.note(np.array_equal(_bits(outs["packed"][i]["G"]), _bits(outs["switch-off"][i]["G"])), f"item {i} of {shapes}: packed != switch-off")
    assert gl.geometry(256, 750, [(256, 3050), (256, 750)], 1)[0] < gl.gram_nsplit(256, 750)
    led.close()


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------
BATCHES = {
    # top, half and quarter size of one channel count: the smaller items get fewer splits than gram_nsplit gives them
    "pyramid-128": [(128, 96, 100), (128, 48, 50), (128, 24, 25)],
    "pyramid-64-512": [(64, 150, 230), (512, 30, 31), (64, 75, 115), (512, 15, 15), (64, 37, 57), (512, 7, 7)],
    # both tile shapes in one grid: one 64-wide workgroup among 150 128-wide ones, the reverse, and 16 of each
    "one-64-among-128": [(512, 30, 31), (64, 3, 5)],
    "one-128-among-64": [(128, 3, 5), (64, 150, 230)],
    "equal-counts": [(64, 32, 64), (128, 16, 32)],
    "sixteen": [(64, 23, 37), (128, 17, 9), (256, 5, 7), (64, 3, 5), (512, 3, 5), (128, 31, 33), (384, 9, 11), (64, 40, 41),
                (256, 12, 13), (128, 8, 8), (64, 16, 16), (512, 10, 11), (128, 17, 9), (256, 20, 21), (64, 9, 9), (128, 5, 5)],
}


def _first_middle_last(c, N, ns, pps):
    plan = gl.window_plan(c, N, ns, pps)
    return [("whole map", 0, N), plan[0], plan[len(plan) // 2], plan[-1]]


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batches_item_by_item(engines, name):
    """One launch_gram_batch for the whole list: every item's reported geometry is the restated rule's, every item is held to
    the statistic on its whole map and on the first, a middle and the last window of its own geometry, an item whose geometry is
    the lone launch's is bitwise eng.gram's, and packed and switch-off agree bitwise item by item.  Measured over the six lists:
    at most 4.65x torch-fp32 / 4.24e-07 in the rows family (a one-pixel window of the 16-item list, 0.62 of the bound; the
    floor is the bound there), blocks 3.85x / 1.84e-07, whole matrix 3.32x / 1.07e-07."""
    shapes = BATCHES[name]
    items = [(c, h * w) for c, h, w in shapes]
    geos = [gl.geometry(*it, items, i) for i, it in enumerate(items)]
    if name.startswith("pyramid"):
        assert sum(g[0] < gl.gram_nsplit(*it) for g, it in zip(geos, items)) >= 2, geos
    if name == "one-64-among-128":
        assert geos[0][0] * gl.gram_pairs(512) == 150 and geos[1][0] == 1
    if name == "one-128-among-64":
        assert geos[0][0] == 1 and geos[1][0] == 135
    if name == "equal-counts":
        assert geos[0][0] == geos[1][0] == 16
    maps = [gl.feature_map(*s) for s in shapes]
    Fs, fds = [gl.pixel_major(m) for m in maps], [dev(m) for m in maps]
    wins = [_first_middle_last(c, h * w, *geos[i]) for i, (c, h, w) in enumerate(shapes)]
    led = Ledger(f"batch {name}")
    for k in range(4):
        fws = [fds[i] if k == 0 else _windowed(fds[i], wins[i][k][1], wins[i][k][2]) for i in range(len(shapes))]
        outs = {e: engines[e].gram_batch(fws) for e in ("packed", "switch-off")}
        for i, (c, h, w) in enumerate(shapes):
            wname, p0, p1 = wins[i][k]
            ref64, ref32 = gl.window_truths(Fs[i], p0, p1, float(c * h * w))
            for e in outs:
                out = outs[e][i]
                led.note((out["nsplit"], out["pix_per_split"]) == geos[i], f"{e} {name} item {i}: geometry {out['nsplit']}, {out['pix_per_split']} != {geos[i]}")
                led.hold((e, "batch"), out["G"].cpu(), ref64, ref32, f"{e} {name} item {i} C={c} {h}x{w} [{p0},{p1}) {wname}")
                led.note(torch.equal(out["G"][0], out["G"][0].t()), f"{e} {name} item {i} {wname}: G is not symmetric")
            led.note(np.array_equal(_bits(outs["packed"][i]["G"]), _bits(outs["switch-off"][i]["G"])), f"{name} item {i} {wname}: packed != switch-off")
            if geos[i] == gl.geometry(c, h * w):
                led.note(np.array_equal(_bits(outs["packed"][i]["G"]), _bits(engines["packed"].gram(fws[i]))), f"{name} item {i} {wname}: not eng.gram's bits")
    led.close()


# ---- 6. the finish pass at a target ---------------------------------------------------------------------------------------------
FINISH_SHAPES = [(64, 23, 37), (128, 17, 9), (256, 50, 61), (384, 9, 11)]
COEF = 3.7e-3


def _cut3(s):
    """the three bf16 pieces of gram_finish_body, as 16-bit words: (C, C/32, 3, 32)"""
    s = np.ascontiguousarray(s, dtype=np.float32)
    c = s.shape[0]
    uh = s.view(np.uint32) & np.uint32(0xFFFF0000)
    r1 = (s - uh.view(np.float32)).astype(np.float32)
    um = r1.view(np.uint32) & np.uint32(0xFFFF0000)
    r2 = (r1 - um.view(np.float32)).astype(np.float32)
    words = np.stack([uh >> 16, um >> 16, r2.view(np.uint32) >> 16]).astype(np.uint16)          # (3, C, C)
    return words.reshape(3, c, c // 32, 32).transpose(1, 2, 0, 3)


def _finish_checks(led, what, out, G, Gt, coef):
    """S, S_bf, S_absmax and the squared sum against the device's own G (numpy fp32) and the target"""
    S = out["S"].cpu().numpy()
    want = np.float32(coef) * (G - Gt)                         # one subtraction, one multiplication, each rounded to fp32
    led.note(np.array_equal(S.view(np.uint32), want.view(np.uint32)), f"{what}: S is not coef (G - Gt) bitwise")
    led.note(np.array_equal(S, S.T), f"{what}: S is not symmetric")
    led.note(np.array_equal(out["S_bf"].cpu().numpy().view(np.uint16), _cut3(S)), f"{what}: S_bf is not the three-piece cut of S")
    led.note(np.float32(out["S_absmax"]).view(np.uint32) == np.abs(S).max().view(np.uint32), f"{what}: S_absmax {out['S_absmax']} != max|S| {np.abs(S).max()}")
    sq = float(((G - Gt).astype(np.float64) ** 2).sum())          # (the fp32 difference S is made of, squared and summed in double)
    report(f"gram finish {what}: sum (G - Gt)^2 device {out['mse']:.17e}, double {sq:.17e}")
    led.note(abs(out["mse"] - sq) <= 1e-12 * sq, f"{what}: squared sum {out['mse']} vs {sq}")


@pytest.mark.parametrize("shape", FINISH_SHAPES, ids=_ids)
def test_finish_pass_at_a_target(engines, shape):
    """nst_gram_batch with a target, given the device's own G: S bitwise coef (G - Gt) in fp32 and exactly symmetric, S_bf its
    three-piece cut, the S_amax record max|S| bitwise, the squared sum within 1e-12 of double arithmetic.  Targets: a random
    symmetric one; the device's G of the same map (everything exactly 0); the device's G of the map with one pixel moved by
    three ulps - G - Gt is cancellation there, and S is held against coef (G64 - Gt), normalised by the rms of the true
    difference G64 - Gt64, to the bound of every other comparison.  Measured there: S stands up to 159 TIMES the true
    difference away from coef (G64 - Gt) - the fp32 Gram's own error against a difference of a few ulps of one pixel (G and Gt
    differ in a handful of entries by one ulp) - and torch-fp32 stands further: the device is at 0.56x ... 0.79x torch-fp32 in
    every family, inside the factor 4."""
    c, h, w = shape
    N, div = h * w, float(c * h * w)
    f = gl.feature_map(c, h, w)
    F, fd = gl.pixel_major(f), dev(f)
    led = Ledger(f"finish pass C={c} {h}x{w}")
    for k in ("packed", "switch-off"):
        eng = engines[k]
        G_dev = eng.gram_batch([fd])[0]["G"]
        G = G_dev[0].cpu().numpy()
        gen = torch.Generator().manual_seed(c + 7)
        r = torch.randn(c, c, generator=gen) * 0.3
        Gt = (G_dev[0].cpu() * (1.0 + 0.5 * (r + r.t()))).contiguous()
        out = eng.gram_batch([fd], targets=[dev(Gt)], coefs=[COEF], want_S_bf=True)[0]
        led.note(np.array_equal(_bits(out["G"]), _bits(G_dev)), f"{k} C={c}: G moved with a target")
        _finish_checks(led, f"{k} C={c} {h}x{w} random target", out, G, Gt.numpy(), COEF)
        # the map's own Gram as the target: everything is exactly zero
        out = eng.gram_batch([fd], targets=[G_dev[0].contiguous()], coefs=[COEF], want_S_bf=True)[0]
        zero = (not out["S"].any().item()) and (not out["S_bf"].any().item()) and out["mse"] == 0.0 and np.float32(out["S_absmax"]).view(np.uint32) == 0
        led.note(zero, f"{k} C={c}: Gt = G does not give exact zeros ({out['mse']}, {out['S_absmax']})")
        # one pixel moved by three ulps: late-optimisation cancellation
        fp = f.clone()
        y, x = h // 2, w // 3
        fp[0, :, y, x] = (fp[0, :, y, x].view(torch.int32) + 3 * torch.sign(fp[0, :, y, x]).to(torch.int32)).view(torch.float32)
        Gt_dev = eng.gram_batch([dev(fp)])[0]["G"][0].contiguous()
        out = eng.gram_batch([fd], targets=[Gt_dev], coefs=[COEF], want_S_bf=True)[0]
        Gt = Gt_dev.cpu()
        _finish_checks(led, f"{k} C={c} {h}x{w} target three ulps away", out, G, Gt.numpy(), COEF)
        G64, G32 = gl.window_truths(F, 0, N, div)
        Gt64, _ = gl.window_truths(gl.pixel_major(fp), 0, N, div)
        scale = COEF * float(np.sqrt(np.mean((G64 - Gt64) ** 2)))
        s64 = COEF * (G64 - Gt.double().numpy())
        s32 = np.float32(COEF) * (G32 - Gt.numpy())
        led.hold((k, "S at cancellation"), out["S"].cpu(), s64, s32, f"{k} C={c} {h}x{w} S, target three ulps away", scale=scale)
    led.close()


# ---- refusals and bookkeeping ---------------------------------------------------------------------------------------------------
def test_refusals(engines):
    from artstyletransfer_amd import _lib
    from artstyletransfer_amd._lib import NstError
    eng = engines["packed"]
    fd = dev(gl.feature_map(64, 3, 5))
    with pytest.raises(NstError, match=r"\(-2\)"):
        engines["f32"].gram_batch([fd])                                       # the batch has no form outside f16x2
    g = torch.Generator().manual_seed(1)
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.gram_batch([dev(torch.rand((1, 96, 5, 7), generator=g))])         # C neither 64 nor a multiple of 128
    with pytest.raises(NstError, match=r"\(-1\)"):
        eng.gram_batch([fd, fd], guides=[dev(torch.ones(3, 5)), None])        # guided and unguided items mixed
    before = eng.bytes()
    items = (_lib.GramBatchItem * 17)()
    for n in (0, 17):
        assert eng.lib.nst_gram_batch(eng.ctx, items, n, 1, None) == E_ARG
    assert eng.lib.nst_gram_batch(eng.ctx, None, 1, 1, None) == E_ARG
    assert eng.lib.nst_gram_batch(eng.ctx, items, 1, 1, None) == E_ARG         # null map
    assert eng.lib.nst_gram_batch(None, items, 1, 1, None) == E_ARG
    assert eng.bytes() == before
    assert FACTOR <= MAX_FACTOR and _lib.NST_GRAM_BATCH_MAX == gl.BATCH_MAX == 16
