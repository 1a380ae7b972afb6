"""CPU: the premises of the exact-tie GPU tests (test_hip_exact_ties.py) on the integer-valued network of exact_net.py.

The GPU tests demand bitwise agreement with an fp64 evaluation.  That is a fair demand only while (a) every value of the
network is a multiple of 2^-f with every partial sum, in any order, below 2^22 of those units - then fp32 accumulation never
rounds - and (b) the operand splittings of the f16x2 and bf16x3 kernels reconstruct such operands exactly; and the tests see
pooling ties and exact-zero units only while the construction is alive and rich in them.  The floors below are conditions on
the construction (with another generator: keep the floors, change the seeds in exact_net.py), not measurements.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_net as E
from hip_helpers import report
from oracle import cpu_ref

ALL = (0, 1, 2, 3, 4, 5)
FLOOR_SIZES = [(37, 50), (64, 96)]


# ---- the generators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [E.NARROW, E.WIDE])
def test_ternary_weights_are_what_they_say(setting):
    ws = E.ternary_vgg19_weights(**setting)
    ref = cpu_ref.synthetic_vgg19_weights()
    assert len(ws) == len(ref)
    for (w, b), (wr, br) in zip(ws, ref):
        assert w.shape == wr.shape and b.shape == br.shape and w.dtype == b.dtype == torch.float32
        assert bool(((w == 0) | (w.abs() == 1)).all())
        assert bool(((w != 0).flatten(1).sum(1) == setting["nnz"]).all())          # nnz taps per output channel
        assert bool((b == b.round()).all()) and setting["bias_lo"] <= float(b.min()) and float(b.max()) <= setting["bias_hi"]
    again = E.ternary_vgg19_weights(**setting)
    assert all(torch.equal(w, w2) and torch.equal(b, b2) for (w, b), (w2, b2) in zip(ws, again))
    assert 0.3 < float((ws[9][0][ws[9][0] != 0] > 0).float().mean()) < 0.7       # both signs


@pytest.mark.parametrize("h,w", [(37, 50), (64, 96), (67, 33)])
def test_block_image_is_integral_and_constant_on_blocks(h, w):
    x = E.block_image(h, w, **E.IMAGE)
    blk, amp = E.IMAGE["blk"], E.IMAGE["amp"]
    assert x.shape == (1, 3, h, w) and x.dtype == torch.float32
    assert bool((x == x.round()).all()) and float(x.abs().max()) <= amp and x.unique().numel() > amp
    corner = x[:, :, ::blk, ::blk].repeat_interleave(blk, 2).repeat_interleave(blk, 3)[:, :, :h, :w]
    assert torch.equal(x, corner)
    assert torch.equal(x, E.block_image(h, w, **E.IMAGE))


# ---- NARROW: integral, bounded, alive, rich in ties and zeros -----------------------------------------------------------------
@pytest.mark.parametrize("h,w", FLOOR_SIZES)
def test_narrow_is_integral_bounded_alive_and_rich_in_ties(h, w):
    p = E.case("narrow", "max", h, w)
    worst = max(l["bound"] for l in p["layers"])
    report(f"exact net NARROW {h}x{w}: largest partial-sum bound {worst:.0f}; alive per layer "
           f"{min(l['alive'] for l in p['layers']):.1%}..{max(l['alive'] for l in p['layers']):.1%}; pre == 0 per layer "
           f"{min(l['zero'] for l in p['layers']):.1%}..{max(l['zero'] for l in p['layers']):.1%}")
    for l in p["layers"]:
        assert l["frac_bits"] == 0, l                      # every pre-activation an integer
        assert l["bound"] < 2 ** 11, l
        assert l["alive"] >= 0.30 and l["zero"] >= 0.03, l
    assert len(p["pools"]) == 4
    for q in p["pools"]:
        report(f"exact net NARROW {h}x{w} pool after {q['name']}: {q['tied']} of {q['windows']} windows positively tied "
               f"({q['tied'] / q['windows']:.1%}), first maximum at 0 / 1 / 2: {q['first']}, positions 1 == 2 above 0: {q['one_two']}")
        assert q["tied"] >= 0.03 * q["windows"], q
        assert q["first"][1] >= 10 and q["first"][2] >= 10 and q["one_two"] >= 10, q


@pytest.mark.parametrize("h,w", FLOOR_SIZES)
def test_narrow_under_average_pooling_has_eight_fractional_bits(h, w):
    p = E.case("narrow", "avg", h, w)
    f = max(l["frac_bits"] for l in p["layers"])
    worst = max(l["bound"] for l in p["layers"])
    report(f"exact net NARROW/avg {h}x{w}: fractional bits per layer {[l['frac_bits'] for l in p['layers']]}, largest bound {worst}")
    assert p["layers"][-1]["frac_bits"] is not None and f <= 8       # multiples of 2^-8 at conv5_1: two bits per pool
    assert all(l["bound"] * 2.0 ** 8 < 2 ** 22 for l in p["layers"])
    assert all(l["alive"] >= 0.30 and l["zero"] >= 0.03 for l in p["layers"])


@pytest.mark.parametrize("h,w", FLOOR_SIZES + [(67, 33)])
def test_wide_is_integral_and_below_two_to_the_22(h, w):
    p = E.case("wide", "max", h, w)
    worst = max(l["bound"] for l in p["layers"])
    report(f"exact net WIDE {h}x{w}: largest partial-sum bound {worst:.0f}, largest |pre| {max(l['max_abs'] for l in p['layers']):.0f}")
    assert all(l["frac_bits"] == 0 for l in p["layers"])
    assert worst < 2 ** 22
    assert max(l["max_abs"] for l in p["layers"]) >= 2 ** 12          # wide enough for the f16x2 low piece to carry bits


# ---- backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,pooling", [("narrow", "max"), ("narrow", "avg"), ("wide", "max")])
@pytest.mark.parametrize("h,w", FLOOR_SIZES)
def test_backward_is_exact_too(setting, pooling, h, w):
    """Ternary output gradients, 5 % dense, on all six maps: every layer's gradient a multiple of 2^-f (f = 0 under max pooling,
    <= 8 under average pooling) with conv_transpose2d(|g|, |w|) 2^f below 2^22; the hand-written fp64 backward that yields
    the bounds is torch's own autograd."""
    gouts = E.ternary_gouts(E.tap_shapes(h, w))
    for g in gouts:
        assert bool(((g == 0) | (g.abs() == 1)).all()) and 0.03 < float((g != 0).float().mean()) < 0.07
    p = E.case(setting, pooling, h, w, ALL)
    fmax = 0 if pooling == "max" else 8
    assert len(p["backward"]) == 13
    for l in p["backward"]:
        assert l["frac_bits"] is not None and l["frac_bits"] <= fmax, l
        assert l["bound"] * 2.0 ** fmax < 2 ** 22, l
    g = p["grad"]
    report(f"exact net {setting}/{pooling} {h}x{w} backward: largest image-gradient entry {float(g.abs().max())}, "
           f"{float((g != 0).double().mean()):.1%} of the entries non-zero, largest bound {max(l['bound'] for l in p['backward'])}")
    assert float((g != 0).double().mean()) > 0.5
    assert torch.equal(g, E.autograd64(E.image_of(h, w), E.weights_of(setting), gouts, pooling))
    for keep in ((0,), (4,), (5,)):
        one = E.case(setting, pooling, h, w, keep)
        assert bool(one["grad"].any())
        assert torch.equal(one["grad"], E.autograd64(E.image_of(h, w), E.weights_of(setting),
                                                     E.ternary_gouts(E.tap_shapes(h, w), keep), pooling))


def test_first_rule_and_position_numbering_are_torchs():
    """The `first` rule of exact_net (position q = 2 dy + dx, first maximum in that order) gives the indices of
    F.max_pool2d(return_indices=True) on the tie-rich maps themselves."""
    h, w = 37, 50
    p = E.case("narrow", "max", h, w)
    for (name, _, _), pre in zip(cpu_ref.VGG19_CONVS, p["pre"]):
        if name in cpu_ref.POOL_AFTER:
            a = torch.relu(pre)
            pos = p["picks"][name]
            wa = a.shape[-1]
            oy = torch.arange(pos.shape[-2]).view(-1, 1) * 2
            ox = torch.arange(pos.shape[-1]).view(1, -1) * 2
            idx = (oy + pos // 2) * wa + ox + pos % 2
            assert torch.equal(idx, F.max_pool2d(a, 2, 2, return_indices=True)[1])


# ---- the arithmetic of the three conv modes on the real operands ----------------------------------------------------------------
def _acc_f32(chains):
    """test_f16x2_model._acc_f32 for operands of any shape: per 16-wide K block every chain adds its exact block sum (the
    products of A (M,K) and W (N,K) summed in fp64: integers far below 2^53) into the fp32 accumulator, chain after chain."""
    (a0, w0) = chains[0]
    acc = np.zeros((a0.shape[0], w0.shape[0]), np.float32)
    for k0 in range(0, a0.shape[1], 16):
        for a, w in chains:
            acc = (acc.astype(np.float64) + a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T).astype(np.float32)
    return acc


@pytest.mark.parametrize("setting,pooling", [("narrow", "max"), ("narrow", "avg"), ("wide", "max")])
def test_three_conv_arithmetics_reproduce_fp64_on_the_widest_layer(setting, pooling):
    """The operand splittings of the kernels (test_f16x2_model._cut2 of conv_h2.hip, _cut3_bf16 of conv_bf3.hip) and an fp32
    accumulator fed 16-wide K blocks, on the layer with the largest partial-sum bound: each gives the fp64 pre-activation
    exactly.  This is why the device must be bitwise."""
    from test_f16x2_model import _cut2, _cut3_bf16, _scale
    h, w = 64, 96
    p = E.case(setting, pooling, h, w)
    f = max(l["frac_bits"] for l in p["layers"])
    li = max(range(13), key=lambda i: p["layers"][i]["bound"] * 2.0 ** p["layers"][i]["frac_bits"])
    wt, b = E.weights_of(setting)[li]
    a_in = E.layer_input(p, li, E.image_of(h, w), pooling)
    A = F.unfold(a_in, 3, padding=1)[0].T.contiguous().numpy().astype(np.float32)          # (pixels, Cin*9)
    W = wt.flatten(1).numpy()
    assert np.array_equal(A.astype(np.float64), F.unfold(a_in, 3, padding=1)[0].T.numpy())      # the operands are fp32 numbers
    ref = p["pre"][li][0].flatten(1).T.numpy()                                                # (pixels, Cout), fp64
    bias = b.numpy().astype(np.float64)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    assert np.array_equal(A64 @ W64.T + bias, ref)
    report(f"exact net {setting}/{pooling} arithmetic on {cpu_ref.VGG19_CONVS[li][0]} (K = {A.shape[1]}, {A.shape[0]} pixels, "
           f"bound {p['layers'][li]['bound']}, {f} fractional bits)")
    # fp32 MFMA
    assert np.array_equal(_acc_f32([(A64, W64)]).astype(np.float64) + bias, ref)
    # bf16x3: six chains into one accumulator
    ah, am, al = _cut3_bf16(A)
    wh, wm, wl = _cut3_bf16(W)
    assert np.array_equal(ah + am + al, A64) and np.array_equal(wh + wm + wl, W64)
    got = _acc_f32([(al, wh), (ah, wl), (am, wm), (am, wh), (ah, wm), (ah, wh)])
    assert np.array_equal(got.astype(np.float64) + bias, ref)
    # f16x2: main and 2^-11-weighted cross products in accumulators of their own, combined in fp32
    sa, sw = _scale(A), _scale(W)
    ah, al = _cut2(A, sa)
    wh, wl = _cut2(W, sw)
    assert np.array_equal((ah + al / 2048.0) / sa, A64) and np.array_equal((wh + wl / 2048.0) / sw, W64)
    main, cross = _acc_f32([(ah, wh)]), _acc_f32([(al, wh), (ah, wl)])
    got = ((main + cross * np.float32(2.0 ** -11)).astype(np.float32) * np.float32(1.0 / (sa * sw))).astype(np.float32)
    assert np.array_equal(got.astype(np.float64) + bias, ref)
    if setting == "wide":
        assert np.abs(al).max() > 0                        # the low piece carries real bits


# ---- what a wrong rule would change -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", FLOOR_SIZES)
def test_a_wrong_tie_rule_or_position_code_changes_the_image_gradient(h, w):
    x, ws = E.image_of(h, w), E.weights_of("narrow")
    gouts = E.ternary_gouts(E.tap_shapes(h, w))
    right = E.case("narrow", "max", h, w, ALL)["grad"]
    assert torch.equal(right, E.autograd64(x, ws, gouts))                   # torch's own rule
    shares = {}
    for rule in ("last", "swap12"):
        pres, masks, picks = E.forward64(x, ws, rule=rule)
        assert all(torch.equal(a, b) for a, b in zip(pres, E.case("narrow", "max", h, w)["pre"]))   # a tie: the forward is the same
        shares[rule] = float((E.backward64(ws, pres, masks, picks, gouts) != right).double().mean())
    pres, masks, picks = E.forward64(x, ws, alive=lambda pre: pre >= 0)
    shares["zero_on"] = float((E.backward64(ws, pres, masks, picks, gouts) != right).double().mean())
    report(f"exact net NARROW {h}x{w} sensitivity: image-gradient entries that change with the last maximum {shares['last']:.1%}, "
           f"with positions 1 and 2 exchanged {shares['swap12']:.1%}, with units kept on at pre == 0 {shares['zero_on']:.1%}")
    assert shares["last"] > 0 and shares["swap12"] > 0 and shares["zero_on"] > 0
