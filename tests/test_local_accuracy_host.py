"""CPU: the local accuracy statistic (tests/local_accuracy.py) sees what the whole-map norms miss.

A model of the f16x2 arithmetic of conv_h2.hip / conv_wino.hip on one small 3x3 layer (Cin 256, Cout 128, a 17 x 65 map,
post-ReLU-like input): every operand cut into two scaled fp16 pieces (cut2 and the scale as in tests/test_f16x2_model.py), the
hi x hi chain and the two 2^-11-weighted cross chains (lo x hi, hi x lo) as separate convolutions.  The chains accumulate in
double here, so the numbers are indicative: what the model shows is what the PIECES leave, not the fp32 accumulators.  Four
defects of the kind a launch can have are then planted, each a loss of low-order products somewhere:

                                                                    whole map   worst class / torch-fp32's     (measured)
    torch fp32                                                       1.7e-7     1 (rows, columns, channel groups, blocks 1.7 - 1.8e-7)
    healthy f16x2                                                    0.75e-7    0.44x in every family
    (a) both cross chains lost on the last column, one tap           1.2e-5     columns   555x
    (b) lo x hi lost in one 4 x 16 tile, one tap, one 32-ch. chunk   5.6e-6     blocks    129x
    (c) 32 output channels lose hi x w_lo                            9.7e-5     channels  1140x
    (d) a one-row partial last tile loses both cross chains          6.0e-5     rows      1390x

(a) and (b) sit under the 2e-5 that every whole-gradient comparison of the suite allows: the documented gap.  Every defect
stands above 16x torch-fp32 in the family that owns it - the most a family's factor may ever be set to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import local_accuracy as la
from test_f16x2_model import _cut2, _scale

CIN, COUT, H, W = 256, 128, 17, 65
TILE = (slice(4, 8), slice(32, 48))          # one 4 x 16 block, aligned at the origin
TAP = (1, 0)                                 # (a tap that reads inside the map from the last column)
CHUNK = slice(64, 96)                        # one 32-channel chunk of K
GROUP = slice(32, 64)                        # one wave's 32 output channels


def _conv(a, w):
    return F.conv2d(torch.from_numpy(a)[None], torch.from_numpy(w), padding=1)[0].numpy()


def _one_tap(w, tap, cin=slice(None)):
    out = np.zeros_like(w)
    out[:, cin, tap[0], tap[1]] = w[:, cin, tap[0], tap[1]]
    return out


@pytest.fixture(scope="module")
def model():
    rng = np.random.default_rng(5)
    a = np.maximum(rng.normal(0, 100, (CIN, H, W)), 0).astype(np.float32)          # post-ReLU-like: half of the units are 0
    w = rng.normal(0, 0.02, (COUT, CIN, 3, 3)).astype(np.float32)
    ref64 = _conv(a.astype(np.float64), w.astype(np.float64))
    ref32 = _conv(a, w)
    sa, sw = _scale(a), _scale(w)
    ah, al = _cut2(a, sa)
    wh, wl = _cut2(w, sw)
    un = lambda main, cross: (main + cross / 2048.0) / (sa * sw)
    main, lo_hi, hi_lo = _conv(ah, wh), _conv(al, wh), _conv(ah, wl)
    cases = {"healthy": un(main, lo_hi + hi_lo)}
    # (a) the last column of the output loses one tap's contribution to both cross chains
    tap_cross = _conv(al, _one_tap(wh, TAP)) + _conv(ah, _one_tap(wl, TAP))
    cross = lo_hi + hi_lo
    cross[:, :, W - 1] -= tap_cross[:, :, W - 1]
    cases["a"] = un(main, cross)
    # (b) one tile loses lo x hi of one tap over one 32-channel chunk
    cross = lo_hi + hi_lo
    cross[(slice(None),) + TILE] -= _conv(al, _one_tap(wh, TAP, CHUNK))[(slice(None),) + TILE]
    cases["b"] = un(main, cross)
    # (c) 32 output channels lose hi x w_lo
    cross = lo_hi + hi_lo
    cross[GROUP] -= hi_lo[GROUP]
    cases["c"] = un(main, cross)
    # (d) 17 = 4 x 4 + 1 rows: the one-row last tile loses both cross chains
    cross = lo_hi + hi_lo
    cross[:, H - 1, :] = 0
    cases["d"] = un(main, cross)
    return ref64, ref32, cases


def _ratios(got, ref64, ref32):
    d, t = la.local_stats(got, ref64), la.local_stats(ref32, ref64)
    return {fam: d[fam][0] / t[fam][0] for fam in d}, d, t


def test_healthy_model_passes_at_factor_4_in_every_family(model):
    ref64, ref32, cases = model
    out = la.assert_locally_as_accurate(cases["healthy"], ref64, ref32, "f16x2 model, healthy", floor=0.0)
    t32 = la.local_stats(ref32, ref64)
    assert 0.5e-7 < t32["map"][0] < 3e-7                                           # torch fp32 itself: ~1.3e-7
    for fam in la.FAMILIES:                                                        # ... alike in every class
        assert t32[fam][0] < 1.5 * t32["map"][0], (fam, t32[fam])
    assert all(d <= 1.5 * t for d, t in out.values()), out                         # measured 0.6x everywhere


@pytest.mark.parametrize("case,family,where", [("a", "columns", W - 1), ("b", "blocks", (1, 2)), ("c", "channels", 1),
                                                 ("d", "rows", H - 1)])
def test_planted_defect_stands_above_16x_in_its_family(model, case, family, where):
    ref64, ref32, cases = model
    ratios, d, t = _ratios(cases[case], ref64, ref32)
    la.report(f"f16x2 model, defect ({case}): whole map {d['map'][0]:.2e}; worst class / torch-fp32's: "
              + ", ".join(f"{fam} {ratios[fam]:.0f}x" for fam in la.FAMILIES))
    assert ratios[family] > 16.0, (case, ratios)
    assert d[family][1] == where, (case, d[family])                                # ... and the statistic names the place
    with pytest.raises(AssertionError):
        la.assert_locally_as_accurate(cases[case], ref64, ref32, f"f16x2 model, defect ({case})", factor=16.0)
    if case in ("a", "b"):                                                         # the documented gap
        assert d["map"][0] < 2e-5, d["map"]
    else:
        assert d["map"][0] > 2e-5, d["map"]


# ---- the fp32 accumulators: where a healthy launch may stand above 4x -------------------------------------------------------
# The model above accumulates in double.  The one below keeps the fp32 accumulators, in the kernels' K order (32-channel chunk,
# tap, K block), on a layer of conv4_2's K = 4608 (Cin 512; Cout 64 on an 8 x 16 map is all the statistic needs):
#   bf16x3 (conv_bf3.hip): three exact bf16 pieces per operand (cut3 truncates), six product chains per K block - smallest first,
#     l x h, h x l, m x m, m x h, h x m, h x h - into ONE accumulator: six roundings at the accumulator's magnitude per block;
#   f16x2 (conv_h2.hip): the hi x hi chain in one accumulator, the two cross chains in a second one weighted 2^-11.
# A K block is what one rounding covers.  With the K = 16 of a matrix instruction the model sits a uniform sqrt(2) under BOTH
# arithmetics' device measurements at every K; with each instruction rounding after each K = 8 half it reproduces them:
#                      K = 576   1152     2304     4608    (map error vs fp64)
#   bf16x3 model K 16  2.6e-7   3.6e-7   4.9e-7   7.0e-7
#   bf16x3 model K 8   3.4e-7   4.9e-7   6.7e-7   9.9e-7   = 5.3x torch-fp32 (worst family 5.5x)
#   bf16x3 device      3.5e-7   5.3e-7   7.3e-7   1.0e-6   = 5.3 - 5.5x, worst family 6.3x   (profiles/local_accuracy.txt)
#   f16x2 model K 8    1.7e-7   2.3e-7   3.0e-7   4.2e-7   = 2.2x
#   f16x2 direct, dev.           2.3e-7   3.2e-7   4.3e-7   = 2.2x
# So bf16x3's excess over 4x is its single accumulator, everywhere alike, not a local loss.
def _k_blocks(cin, kb):
    return [[(c * 32 + ks * kb + j) * 9 + t for j in range(kb)] for c in range(cin // 32) for t in range(9) for ks in range(32 // kb)]


def _f32(x):
    return x.astype(np.float32).astype(np.float64)


def _accumulator_models(cin, cout, h, w, kb, seed=7):
    from test_f16x2_model import _cut3_bf16
    rng = np.random.default_rng(seed)
    a = np.maximum(rng.normal(0, 100, (cin, h, w)), 0).astype(np.float32)
    wt = (rng.normal(0, 1, (cout, cin, 3, 3)) * np.sqrt(2.0 / (cout * 9))).astype(np.float32)
    b = rng.normal(0, 2, cout).astype(np.float32)
    ta, tw, tb = torch.from_numpy(a)[None], torch.from_numpy(wt), torch.from_numpy(b)
    ref64 = F.conv2d(ta.double(), tw.double(), tb.double(), padding=1)[0].numpy()
    ref32 = F.conv2d(ta, tw, tb, padding=1)[0].numpy()
    A = F.unfold(ta, 3, padding=1)[0].numpy().T.copy()                  # (pixels, Cin * 9), k = channel * 9 + tap
    Wm = wt.reshape(cout, cin * 9).T.copy()
    back = lambda acc: _f32(acc + b[None, :]).T.reshape(cout, h, w)
    blocks = _k_blocks(cin, kb)
    ap, wp = _cut3_bf16(A), _cut3_bf16(Wm)
    acc = np.zeros((h * w, cout))
    for blk in blocks:
        for i, j in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
            acc = _f32(acc + ap[i][:, blk] @ wp[j][blk, :])
    bf3 = back(acc)
    sa, sw = _scale(A), _scale(Wm)
    (ah, al), (wh, wl) = _cut2(A, sa), _cut2(Wm, sw)
    main, cross = np.zeros((h * w, cout)), np.zeros((h * w, cout))
    for blk in blocks:
        main = _f32(main + ah[:, blk] @ wh[blk, :])
        cross = _f32(_f32(cross + al[:, blk] @ wh[blk, :]) + ah[:, blk] @ wl[blk, :])
    h2 = back(_f32(_f32(main + cross / 2048.0) / (sa * sw)))
    return ref64, ref32, bf3, h2


def test_bf16x3_factor_is_twice_what_the_model_predicts():
    ref64, ref32, bf3, h2 = _accumulator_models(512, 64, 8, 16, kb=8)
    r_bf3, d_bf3, t = _ratios(bf3, ref64, ref32)
    r_h2, d_h2, _ = _ratios(h2, ref64, ref32)
    la.report(f"accumulator model, K = 4608, one rounding per K = 8: torch-fp32 {t['map'][0]:.2e}; bf16x3 {d_bf3['map'][0]:.2e} = "
              + ", ".join(f"{fam} {r_bf3[fam]:.2f}x" for fam in r_bf3) + f"; f16x2 {d_h2['map'][0]:.2e} = "
              + ", ".join(f"{fam} {r_h2[fam]:.2f}x" for fam in r_h2))
    assert 8.5e-7 < d_bf3["map"][0] < 1.15e-6                    # what the device measures at conv4_2 ... conv4_4: 1.0e-6
    assert 3.6e-7 < d_h2["map"][0] < 4.9e-7                      # ... and the direct f16x2 launches there: 4.3e-7
    worst = max(r_bf3.values())
    assert worst > la.FACTOR                                      # the standing factor cannot hold for this arithmetic
    assert la.BF16X3_FORWARD_FACTOR <= la.MAX_FACTOR
    assert abs(la.BF16X3_FORWARD_FACTOR - 2.0 * worst) <= 0.25 * la.BF16X3_FORWARD_FACTOR, worst      # measured 5.5x
    assert max(r_h2.values()) < la.FACTOR                         # f16x2 stays inside the standing factor: 2.3x
    # the spread between the families is small: the excess is everywhere alike, which is what tells it from a local loss
    assert max(r_bf3.values()) < 1.15 * min(r_bf3.values()), r_bf3
    # with one rounding per K = 16 instruction the model is a uniform sqrt(2) lower
    _, _, bf3_16, h2_16 = _accumulator_models(512, 64, 8, 16, kb=16)
    for lo, hi_ in ((bf3_16, bf3), (h2_16, h2)):
        q = la.local_stats(hi_, ref64)["map"][0] / la.local_stats(lo, ref64)["map"][0]
        assert 1.25 < q < 1.6, q


# ---- the helper itself ---------------------------------------------------------------------------------------------------------
def test_class_sizes_and_merging_on_odd_maps():
    # 1 x 4, 64 channels: a column is 64 entries - exactly the minimum -, one row, one (partial) block
    g = la.class_grid((64, 1, 4))
    s = la.class_sizes((64, 1, 4))
    assert g["rows"] == [0, 1] and g["columns"] == [0, 1, 2, 3, 4] and g["channels"] == [0, 32, 64] and g["blocks"] == ([0, 1], [0, 4])
    assert s["columns"].tolist() == [64] * 4 and s["channels"].tolist() == [128, 128] and s["blocks"].tolist() == [[256]]
    # 17 x 65, 256 channels: the one-row last tile and the one-column last tile are classes of their own, corner included
    g, s = la.class_grid((256, 17, 65)), la.class_sizes((256, 17, 65))
    assert g["blocks"] == ([0, 4, 8, 12, 16, 17], [0, 16, 32, 48, 64, 65])
    assert s["blocks"][0, 0] == 256 * 64 and s["blocks"][4, 0] == 256 * 16 and s["blocks"][0, 4] == 256 * 4 and s["blocks"][4, 4] == 256
    assert len(s["rows"]) == 17 and len(s["columns"]) == 65 and len(s["channels"]) == 8
    # 31 x 63, 128 channels: 3-row and 15-column edge blocks
    g, s = la.class_grid((128, 31, 63)), la.class_sizes((128, 31, 63))
    assert g["blocks"] == ([0, 4, 8, 12, 16, 20, 24, 28, 31], [0, 16, 32, 48, 63]) and s["blocks"][7, 3] == 128 * 3 * 15
    # an image gradient: each channel, 16 x 16 pixel blocks; 33 x 17 leaves a 1 x 16 (48 entries), a 16 x 1 and a 1 x 1 block
    # behind: the short row segment joins the block row above it, then the short column segment the block column before it
    g, s = la.class_grid((3, 33, 17), image=True), la.class_sizes((3, 33, 17), image=True)
    assert g["channels"] == [0, 1, 2, 3] and g["blocks"] == ([0, 16, 33], [0, 17])
    assert s["blocks"].tolist() == [[3 * 16 * 17], [3 * 17 * 17]]
    # rows of fewer than 64 entries are merged in runs, a short last run into the one before it: 3 x 7 x 10 -> rows of 30
    g = la.class_grid((3, 7, 10), image=True)
    assert g["rows"] == [0, 3, 7] and g["columns"] == [0, 4, 10]
    for shape in ((64, 1, 4), (256, 17, 65), (128, 31, 63), (512, 2, 8), (64, 68, 260)):
        s = la.class_sizes(shape)
        assert all(s[f].min() >= la.MIN_CLASS and s[f].sum() == np.prod(shape) for f in la.FAMILIES), shape
    with pytest.raises(AssertionError):
        la.class_grid((3, 1, 4), image=True)                                        # 12 entries: no class can hold 64


def test_a_zero_channel_does_not_divide_by_zero():
    rng = np.random.default_rng(1)
    ref = rng.normal(0, 1, (64, 8, 16))
    ref[:32] = 0.0                                                                  # a dead channel group
    got = ref.copy()
    got[:32] += 1e-3                                                                # ... that the device does not leave at zero
    e = la.local_errors(got, ref)
    scale = np.sqrt(np.mean(ref ** 2))
    assert np.isfinite(e["channels"]).all()
    np.testing.assert_allclose(e["channels"], [1e-3 / scale, 0.0], rtol=1e-12)
    np.testing.assert_allclose(e["map"], 1e-3 * np.sqrt(0.5) / scale, rtol=1e-12)
    with pytest.raises(AssertionError):
        la.local_errors(got * 0, ref * 0)                                           # a truth that is all zero normalises nothing


def test_exact_values_on_a_hand_made_error_pattern():
    C, Hh, Ww = 64, 9, 33                                                           # blocks: rows 4 + 4 + 1, columns 16 + 16 + 1
    ref = np.full((C, Hh, Ww), 2.0)                                                 # whole-map rms 2
    got = ref.copy()
    got[:, 8, :] += 0.5                                                             # the last row, every channel
    got[40, 2, 20] += 8.0                                                           # one entry: channel group 1, block (0, 1)
    s = la.local_stats(got, ref)
    n = C * Hh * Ww
    sq_row, sq_one = 0.25 * C * Ww, 64.0
    assert s["map"][0] == pytest.approx(np.sqrt((sq_row + sq_one) / n) / 2.0, rel=1e-12)
    assert s["rows"] == (pytest.approx(0.25), 8)                                    # rms 0.5 over the row / 2
    assert s["columns"] == (pytest.approx(np.sqrt((0.25 * C + sq_one) / (C * Hh)) / 2.0), 20)
    assert s["channels"] == (pytest.approx(np.sqrt((0.25 * 32 * Ww + sq_one) / (32 * Hh * Ww)) / 2.0), 1)
    assert s["blocks"][1] == (2, 0) and s["blocks"][0] == pytest.approx(0.25)       # a last-row block: every entry off by 0.5
    e = la.local_errors(got, ref)
    assert e["blocks"].shape == (3, 3)
    assert e["blocks"][0, 1] == pytest.approx(np.sqrt(sq_one / (C * 4 * 16)) / 2.0)
    assert e["blocks"][0, 0] == 0.0 and e["blocks"][1, 2] == 0.0 and e["blocks"][2, 2] == pytest.approx(0.25)
    # torch tensors with a leading batch axis are taken as they come off the device
    s2 = la.local_stats(torch.from_numpy(got)[None].float(), torch.from_numpy(ref)[None])
    assert s2["rows"][1] == 8 and s2["rows"][0] == pytest.approx(0.25)
    # the assertion: fails in the family that owns the excess, passes under a per-family factor, holds the floor
    ref32 = ref + 1e-7
    with pytest.raises(AssertionError) as exc:
        la.assert_locally_as_accurate(got, ref, ref32, "hand-made")
    assert "rows" in str(exc.value)
    la.assert_locally_as_accurate(ref + 3e-7, ref, ref32, "hand-made, 3x", floor=0.0)           # 3x "torch-fp32": under 4x
    with pytest.raises(AssertionError):
        la.assert_locally_as_accurate(ref + 5e-7, ref, ref32, "hand-made, 5x", floor=0.0)
    la.assert_locally_as_accurate(ref + 5e-7, ref, ref32, "hand-made, 5x, 6 allowed on rows ... blocks",
                                  factor=dict.fromkeys(("map",) + la.FAMILIES, 6.0), floor=0.0)
    la.assert_locally_as_accurate(ref + 9e-7, ref, ref, "hand-made, under the floor")           # 4.5e-7 < 5e-7
    with pytest.raises(AssertionError):
        la.assert_locally_as_accurate(ref + 1.1e-6, ref, ref, "hand-made, over the floor")
