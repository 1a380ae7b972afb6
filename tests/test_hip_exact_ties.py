"""GPU: pooling ties and exact-zero ReLU units, held to an fp64 evaluation BITWISE on the integer-valued network of
exact_net.py (ternary weights, integer biases, an integer block image).

Every other comparison of the suite runs on seeded Gaussian images and weights, where two positive units of a pooling window
are never bitwise equal and no pre-activation is exactly 0 - and reads the device's pooling choice off its activations with
torch's own first-maximum rule (cpu_ref.Decisions).  The arg-max code the forward epilogues write and the un-pooling loaders
read is observable only through the GRADIENT of a window that ties.  Here 9-29 % of the windows tie positively, 6-16 % of the
pre-activations are exactly 0, and - every value and every partial sum being an integer (a multiple of 2^-8 under average
pooling) far below 2^22, see test_exact_net_host.py - the right answer is one fp32 bit pattern per entry: a gradient handed to
the last maximum, a window numbered column-major in one register layout or a unit kept on at pre == 0 changes an integer entry
of the image gradient (11-89 % of them: the host module's sensitivity test).  No tolerance, no near-tie allowance."""
import numpy as np
import pytest
import torch

import exact_net as E
from hip_helpers import (BULK_RTOL, TERMS, check_rows, closure_vs_oracle_under_equal_decisions, dev, device_decisions,
                         levels as _levels, oracle_targets, rel_l2, report, setup as _setup)
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SIZES = ((37, 50), (64, 96), (67, 33))          # the third: bitwise checks only (odd rows at the first two pools, an odd width at the first)
CLOSURE_SIZES = ((37, 50), (64, 96))
ENGINES = {
    "default": {},
    "bf16x3": dict(conv_mode="bf16x3"),
    "f32": dict(conv_mode="f32"),
    "per-level": dict(batched=False),
    "winograd": dict(h2_winograd=True),
    "direct": dict(h2_winograd=False),
    "mfma-0": dict(h2_mfma16=0),
    "mfma-2": dict(h2_mfma16=2),
    "mfma-3": dict(h2_mfma16=3),
    "wg256": dict(h2_wg256=True),
    "rows4": dict(h2_tile_rows=4),
    "rows8": dict(h2_tile_rows=8),
    "rows16": dict(h2_tile_rows=16),
}
CLOSURE_ENGINES = ("default", "bf16x3", "f32", "per-level")
KEEPS = ((0, 1, 2, 3, 4, 5), (0,), (4,), (5,))


def _engine(setting, mode):
    from artstyletransfer_amd.engine import StyleEngine
    return StyleEngine(E.weights_of(setting), 0, **ENGINES[mode])


def _same(got, ref, what):
    """torch.equal, with the first differing entry in the message: the integer mismatch pinpoints layer, channel and position."""
    got = got.detach().cpu().reshape(ref.shape)
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    i = tuple(int(v) for v in bad[0])
    pytest.fail(f"{what}: {bad.shape[0]} of {ref.numel()} entries differ; first at {i}: device {float(got[i])!r}, fp64 {float(ref[i])!r}; "
                f"largest |difference| {float((got.double() - ref.double()).abs().max())!r}")


def _exercised(p):
    return sum(q["tied"] for q in p["pools"]), sum(l["zeros"] for l in p["layers"])


# ---- forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(ENGINES))
def test_forward_is_bitwise_the_fp64_network(mode):
    """nst_vgg_activations (all 13 post-ReLU maps) and nst_vgg_features (the six taps) equal relu(pre64) cast to fp32, on NARROW
    and WIDE under max pooling and on NARROW under average pooling.  The pooled values show in the next layer's map."""
    tied = zeros = maps = 0
    for setting, poolings in (("narrow", ("max", "avg")), ("wide", ("max",))):
        eng = _engine(setting, mode)
        try:
            for pooling in poolings:
                eng.set_pooling(pooling)
                for h, w in SIZES:
                    p = E.case(setting, pooling, h, w)
                    x = dev(E.image_of(h, w))
                    ref = [torch.relu(pre).float() for pre in p["pre"]]
                    acts = eng.vgg_activations(x)
                    for (name, _, _), a, r in zip(cpu_ref.VGG19_CONVS, acts, ref):
                        _same(a, r, f"{mode} {setting}/{pooling} {h}x{w} ReLU({name})")
                    feats = eng.vgg_features(x)
                    for name, f in zip(cpu_ref.TAPS, feats):
                        _same(f, ref[[n for n, _, _ in cpu_ref.VGG19_CONVS].index(name)], f"{mode} {setting}/{pooling} {h}x{w} map {name}")
                    t, z = _exercised(p)
                    tied, zeros, maps = tied + (t if pooling == "max" else 0), zeros + z, maps + 19
        finally:
            eng.close()
    report(f"exact ties [{mode}]: forward bitwise on {maps} maps; {tied} positively tied max-pooling windows and {zeros} units with "
           f"pre == 0 exercised")


# ---- backward --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(ENGINES))
def test_backward_is_bitwise_fp64_autograd(mode):
    """nst_vgg_features_backward with ternary output gradients (5 % dense) on all six maps, and on relu1_1, conv4_2 and relu5_1
    alone, equals torch's fp64 autograd cast to fp32, under max and under average pooling.  Under max pooling every positively
    tied window routes its gradient through the arg-max code; every pre == 0 unit must be off."""
    tied = zeros = grads = 0
    eng = _engine("narrow", mode)
    try:
        for pooling in ("max", "avg"):
            eng.set_pooling(pooling)
            for h, w in SIZES:
                x = dev(E.image_of(h, w))
                for keep in KEEPS:
                    gouts = E.ternary_gouts(E.tap_shapes(h, w), keep)
                    ref = E.autograd_of("narrow", pooling, h, w, keep).float()
                    assert bool(ref.any())
                    got = eng.vgg_features_backward(x, [dev(g) if g is not None else None for g in gouts])
                    _same(got, ref, f"{mode} narrow/{pooling} {h}x{w} image gradient of the maps {keep}")
                    grads += 1
                t, z = _exercised(E.case("narrow", pooling, h, w))
                tied, zeros = tied + (t if pooling == "max" else 0), zeros + z
    finally:
        eng.close()
    report(f"exact ties [{mode}]: backward bitwise on {grads} image gradients; {tied} positively tied max-pooling windows and {zeros} "
           f"units with pre == 0 exercised")


# ---- the closure of one level, by both walkers -----------------------------------------------------------------------------------
# A one-level job below 256 x 256 pixels is evaluated by the per-level walker, and so are nst_vgg_activations / nst_vgg_features /
# nst_vgg_features_backward above: they reach the first-maximum chains of the per-level conv_h2 kernel and of
# launch_maxpool_bwd_relu.  The chains of the BATCHED conv_h2 kernel (its 16x16-MFMA and general epilogues) and of conv_wino.hip
# run only under the batched walker, which a job of two levels takes at any size: the same level-0 closure is therefore also
# evaluated as nst_closure_levels(mask = 1) of a two-level job, with every convolution direct (the conv_h2 epilogues at all four
# pools) and with the Winograd default (conv_wino.hip's at conv3_4 and conv4_4).
BATCHED_ENGINES = {
    "default": {},
    "bf16x3": dict(conv_mode="bf16x3"),
    "direct": dict(h2_winograd=False),
    "mfma-0-direct": dict(h2_mfma16=0, h2_winograd=False),
    "mfma-2-direct": dict(h2_mfma16=2, h2_winograd=False),
    "mfma-3": dict(h2_mfma16=3),
    "mfma-3-direct": dict(h2_mfma16=3, h2_winograd=False),
    "rows8-direct": dict(h2_tile_rows=8, h2_winograd=False),
    "rows8-mfma-3-direct": dict(h2_tile_rows=8, h2_mfma16=3, h2_winograd=False),
    "rows16-direct": dict(h2_tile_rows=16, h2_winograd=False),
    "rows16-wg256-direct": dict(h2_tile_rows=16, h2_wg256=True, h2_winograd=False),
}
_OWN = {}          # (h, w) -> (contents, styles, oracle targets of level 0, {term: the oracle's own evaluation of level 0})


def _job(h, w):
    if (h, w) not in _OWN:
        c, s = _levels(h, w, 2, 1), _levels(45, 61, 2, 2)            # (level 0 of a pyramid does not depend on its depth)
        _OWN[(h, w)] = (c, s, oracle_targets(c[:1], s[:1], E.weights_of("narrow")), {})
    return _OWN[(h, w)]


def _closure_is_the_oracles_own(opts, mode, h, w, nlev):
    from artstyletransfer_amd.engine import StyleEngine
    weights = E.weights_of("narrow")
    c, s, tg, own = _job(h, w)
    xt = E.image_of(h, w)
    what = f"[{mode}, {'batched' if nlev > 1 else 'per-level'} walker] {h}x{w}"
    eng = StyleEngine(weights, 0, **opts)
    parts = {}
    try:
        _setup(eng, c[:nlev], s[:nlev])
        xd = dev(xt)
        for name, (cw, sw, tvw) in TERMS:
            grad, losses = eng.closure(xd, cw, sw, tvw) if nlev == 1 else eng.closure_levels(xd, cw, sw, tvw, 1)
            dec = device_decisions(eng, xd, only_levels=[0])[0]
            losses, g = losses.cpu().numpy(), grad.cpu().numpy()
            parts[name] = g.astype(np.float64)
            if name not in own:
                rec = []
                loss, grad_own, rows = cpu_ref.closure_eval(xt, tg, weights, cw, sw, tvw, record=rec)
                own[name] = (loss, grad_own, rows, cpu_ref.Decisions([torch.relu(p) for p in rec[0]], xt), rec[0])
            loss, grad_own, rows, dec_own, pre = own[name]
            for (lname, _, _), m, mo, p32, p64 in zip(cpu_ref.VGG19_CONVS, dec.relu, dec_own.relu, pre, E.case("narrow", "max", h, w)["pre"]):
                assert torch.equal(p32.double(), p64), lname                    # the oracle's own forward is the exact one
                assert torch.equal(m, mo), (what, name, lname, int((m != mo).sum()))
            for lname in cpu_ref.POOL_AFTER:
                assert torch.equal(dec.pool[lname], dec_own.pool[lname]), (what, name, lname)
            assert torch.equal(dec.tv[0], dec_own.tv[0]) and torch.equal(dec.tv[1], dec_own.tv[1])
            e_l = abs(float(losses[-1]) - float(loss)) / abs(float(loss))
            e_g = rel_l2(g, grad_own.numpy())
            report(f"exact ties closure {what} [{name}]: identical decisions; loss rel {e_l:.1e}, whole gradient rel-L2 under the "
                   f"oracle's own decisions {e_g:.1e}")
            assert e_l <= 1e-5, (what, name, float(losses[-1]), float(loss))
            level_rows = losses[:-1].reshape(nlev, 4)
            check_rows(level_rows[:1], np.array(rows), 2e-5, cw, sw, tvw)
            assert not level_rows[1:].any()                                     # the level outside the mask adds nothing
            assert e_g < BULK_RTOL, (what, name, e_g)
        total = parts["content"] + parts["style"] + parts["tv"]
        add = float(np.linalg.norm(parts["all"] - total) / np.linalg.norm(total))
        report(f"exact ties closure {what}: |g(all) - sum of the terms| / |.| = {add:.1e}")
        assert add < 2e-6, (what, add)
    finally:
        eng.close()


@pytest.mark.parametrize("h,w", CLOSURE_SIZES)
@pytest.mark.parametrize("mode", CLOSURE_ENGINES)
def test_closure_decisions_are_the_oracles_own(mode, h, w):
    """The closure of the block image on the NARROW network against ordinary synthetic content and style targets: the decisions
    read off the device are IDENTICAL to the oracle's own (ReLU masks, pooling indices, TV signs - the oracle's fp32 forward of
    an integer image is exact), losses agree to 1e-5 (rows 2e-5) and, for every term, the WHOLE gradient is within BULK_RTOL of
    the oracle under its own decisions: no flipped-field allowance.  The terms add up."""
    _closure_is_the_oracles_own(ENGINES[mode], mode, h, w, 1)


@pytest.mark.parametrize("h,w", CLOSURE_SIZES)
@pytest.mark.parametrize("mode", list(BATCHED_ENGINES))
def test_closure_by_the_batched_walker_is_the_oracles_own(mode, h, w):
    """The same level-0 closure as the masked closure of a two-level job (the batched walker: its conv_h2 kernel and the Winograd
    kernel write the arg-max code there), to the same conditions: identical decisions, losses 1e-5, the whole gradient of every
    term within BULK_RTOL of the oracle under its own decisions.  A window routed to the wrong one of two tied positions moves
    the gradient by orders of magnitude more (measured with the Winograd chain scanning column-major: 1e-1)."""
    _closure_is_the_oracles_own(BATCHED_ENGINES[mode], mode, h, w, 2)


def test_two_level_job_on_the_block_image():
    """One two-level job on the 64x96 block image through the standing strict comparison, unchanged: level 1 (the bicubic half of
    the block image) is not integral, so the standing tolerances and near-tie rules apply."""
    weights = E.weights_of("narrow")
    h, w = 64, 96
    c, s = _levels(h, w, 2, 1), _levels(50, 76, 2, 2)
    eng = _engine("narrow", "default")
    try:
        _setup(eng, c, s)
        closure_vs_oracle_under_equal_decisions(eng, E.image_of(h, w), oracle_targets(c, s, weights), weights, "exact ties 64x96 L1")
    finally:
        eng.close()
