"""GPU: the long-term anchor (nst_anchor_fold, StyleEngine.anchor_fold, video.long_term_anchor and
video.neural_style_transfer_video_long_term; Ruder, Dosovitskiy & Brox 2016, section 4.3) against the fp64 restatement of the
definitions in include/nst_hip.h (tests/long_term_ref.py).

Bounds.  The anchor: rel-L2 to fp64 at most 3 x the distance of the same formula in torch fp32 from fp64 (the project's rule
for a streaming kernel; with one live source per pixel both are 0 and the anchor has the source's bits).  `weight` and `parts`:
bit for bit the numpy fp32 evaluation - subtraction, addition, min and max are single roundings.

The kernel's geometry (temporal.hip): a lane owns four consecutive pixels, a block 256 lanes - 1024 pixels a pass; a plane
takes 16-byte accesses where it starts on a 16-byte boundary (long_term_ref.vec_paths restates the rule), the last h w % 4
pixels and every other plane go pixel by pixel."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch

import long_term_ref as ref
import temporal_ref
from oracle import cpu_ref
from hip_helpers import dev, rel_l2, report

pytestmark = pytest.mark.gpu

E_ARG = -1
POISON = -777.0


def _bits(t):
    if isinstance(t, np.ndarray):
        return np.ascontiguousarray(t, np.float32).view(np.int32)
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


def _place(arr, off):
    """A device copy of `arr` that starts `off` floats past a 16-byte boundary (torch's allocations start on one)."""
    flat = torch.empty(arr.size + 4, dtype=torch.float32, device="cuda:0")
    assert flat.data_ptr() % 16 == 0
    view = flat[off:off + arr.size].view(*arr.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr, np.float32)))
    return view


def _raw(eng, sources, weights, anchor, weight, parts, J=None, C_=None):
    """nst_anchor_fold itself on the caller's buffers; returns its code."""
    J = len(sources) if J is None else J
    c, h, w = sources[0].shape
    src = (C.c_void_p * max(len(sources), 1))(*[s.data_ptr() for s in sources])
    wts = (C.c_void_p * max(len(weights), 1))(*[p.data_ptr() for p in weights])
    code = eng.lib.nst_anchor_fold(eng.ctx, J, src, wts, c if C_ is None else C_, h, w, C.c_void_p(anchor.data_ptr()),
                                   C.c_void_p(weight.data_ptr()), C.c_void_p(parts.data_ptr() if parts is not None else 0),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code


def _fold_at(eng, sources, weights, off=0):
    """The fold of host arrays with every plane `off` floats past a 16-byte boundary; (anchor, weight, parts, paths)."""
    J, (c, h, w) = len(sources), sources[0].shape
    ds, dw = [_place(s, off) for s in sources], [_place(p, off) for p in weights]
    anchor, weight, parts = (_place(np.full(shape, POISON, np.float32), off) for shape in ((c, h, w), (h, w), (J, h, w)))
    assert _raw(eng, ds, dw, anchor, weight, parts) == 0
    paths = ref.vec_paths([s.data_ptr() for s in ds], [p.data_ptr() for p in dw], anchor.data_ptr(), weight.data_ptr(), parts.data_ptr(),
                          c, h * w)
    return anchor.cpu().numpy(), weight.cpu().numpy(), parts.cpu().numpy(), paths


# (h, w, floats past a boundary); what _expected_paths says of each is asserted in the test
SHAPES = [(1, 1, 0), (3, 5, 0), (25, 41, 0), (33, 128, 0), (8, 12, 1)]


def _expected_paths(h, w, off, J, C_):
    """Which path a shape takes: 1x1 - one pixel, no group of four; 3x5 - three groups and a tail of three, and since 15 is
    no multiple of four only plane 0 (and planes 4 and 8 ...) of a stack is aligned; 25x41 = 1025 pixels - 256 groups, one
    more pixel than a block's pass, so a second block runs and takes the tail; 33x128 - every plane aligned, five blocks, no
    tail; 8x12 one float past a boundary - every plane misaligned: pixel by pixel throughout."""
    hw = h * w
    al = lambda k: off == 0 and (k * hw) % 4 == 0
    return {"weights": off == 0, "channels": [al(ch) for ch in range(C_)], "parts": [al(j) for j in range(J)], "quads": hw // 4,
            "tail": hw % 4}


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("J", [1, 2, 3, 8])
def test_fold_against_fp64(eng, J, C_):
    for k, (h, w, off) in enumerate(SHAPES):
        weights = ref.random_weights(J, h, w, seed=100 * J + 10 * C_ + k)
        sources = ref.random_sources(J, C_, h, w, seed=1000 + 100 * J + 10 * C_ + k)
        anchor, weight, parts, paths = _fold_at(eng, sources, weights, off)
        assert paths == _expected_paths(h, w, off, J, C_), (h, w, paths)
        if (h, w) == (25, 41):
            assert paths["quads"] == 256 and paths["tail"] == 1 and h * w == 256 * 4 + 1          # one past a block's pass
        if (h, w) == (33, 128):
            assert all(paths["channels"]) and all(paths["parts"]) and paths["quads"] > 4 * 256      # several blocks, all 16-byte
        if off:
            assert not (paths["weights"] or any(paths["channels"]) or any(paths["parts"]))
        a64, w64, p64, _ = ref.fold(sources, weights)
        _, w32, p32, _ = ref.fold(sources, weights, np.float32)
        a32 = ref.fold_torch(sources, weights)
        assert np.array_equal(_bits(weight), _bits(w32)) and np.array_equal(_bits(parts), _bits(p32)), (h, w)
        assert weight.max() <= 1.0
        e_dev, e_32 = rel_l2(anchor, a64), rel_l2(a32, a64)
        report(f"anchor fold J={J} C={C_} {h}x{w}{' (+1 float)' if off else ''}: rel-L2 to fp64 {e_dev:.2e}, torch fp32 {e_32:.2e} "
               f"(bound {3 * e_32:.2e}); bitwise the torch fp32 anchor: {np.array_equal(_bits(anchor), _bits(a32))}")
        assert e_dev <= 3 * e_32, (h, w, e_dev, e_32)
        if J == 1:
            assert e_32 == 0.0


def test_binary_disjoint_weights_select_and_dead_sources_do_not_leak(eng):
    """Weights of 0 and 1: the anchor has the bits of the nearest source whose weight is 1 and of source 0 where none is;
    NaNs planted in every source wherever its l_j = 0 (but in source 0 where nothing is chosen) never appear."""
    for J, C_, (h, w) in ((3, 3, (25, 41)), (8, 1, (33, 128)), (2, 3, (3, 5))):
        rng = np.random.RandomState(J)
        weights = [(rng.uniform(size=(h, w)) < 0.35).astype(np.float32) for _ in range(J)]
        sources = ref.random_sources(J, C_, h, w, seed=50 + J)
        stack = np.stack(weights)
        chosen = np.where(stack.max(0) > 0, np.argmax(stack, axis=0), 0)
        for j in range(J):
            sources[j][:, chosen != j] = np.nan
        anchor, weight, parts, _ = _fold_at(eng, sources, weights)
        want = np.choose(chosen[None], sources)
        assert np.isfinite(want).all() and np.array_equal(_bits(anchor), _bits(want))
        assert np.array_equal(weight, stack.max(0)) and set(np.unique(weight)) <= {0.0, 1.0}
        assert np.array_equal(parts.sum(0), weight) and set(np.unique(parts)) <= {0.0, 1.0}
        assert np.array_equal(np.argmax(parts, axis=0)[weight > 0], chosen[weight > 0])


def test_one_source_keeps_its_bits_and_its_weights(eng):
    for C_, (h, w, off) in ((3, (25, 41, 0)), (1, (8, 12, 1)), (3, (33, 128, 0))):
        weights = ref.random_weights(1, h, w, seed=5)
        assert ((weights[0] > 0) & (weights[0] < 1)).mean() > 0.4
        sources = ref.random_sources(1, C_, h, w, seed=6)
        anchor, weight, parts, _ = _fold_at(eng, sources, weights, off)
        assert np.array_equal(_bits(anchor), _bits(sources[0]))
        assert np.array_equal(_bits(weight), _bits(weights[0])) and np.array_equal(_bits(parts[0]), _bits(weights[0]))
    # through the engine call, which allocates the outputs
    a, c = eng.anchor_fold([dev(torch.from_numpy(sources[0]))], [dev(torch.from_numpy(weights[0]))])
    assert np.array_equal(_bits(a), _bits(sources[0])) and np.array_equal(_bits(c), _bits(weights[0]))
    a, c, p = eng.anchor_fold([dev(torch.from_numpy(sources[0]))], [dev(torch.from_numpy(weights[0]))], want_parts=True)
    assert tuple(p.shape) == (1, h, w) and np.array_equal(_bits(p[0]), _bits(weights[0]))


def test_weights_are_sanitised(eng):
    """NaN, -0.5 and 1.5 in a weight plane act as 0, 0 and 1."""
    h, w = 5, 8
    w0 = np.full((h, w), 0.5, np.float32)
    w0[0, :], w0[1, :], w0[2, :] = np.nan, -0.5, 1.5
    clean = w0.copy()
    clean[0, :], clean[1, :], clean[2, :] = 0.0, 0.0, 1.0
    w1 = np.full((h, w), 0.75, np.float32)
    sources = ref.random_sources(2, 3, h, w, seed=9)
    got = _fold_at(eng, sources, [w0, w1])
    want = _fold_at(eng, sources, [clean, w1])
    for g, x in zip(got[:3], want[:3]):
        assert np.array_equal(_bits(g), _bits(x))
    assert np.array_equal(got[2][0], clean) and np.array_equal(got[2][1][:3], [[0.75] * w, [0.75] * w, [0.0] * w])
    assert np.isfinite(got[0]).all() and np.array_equal(got[1][:4], [[0.75] * w, [0.75] * w, [1.0] * w, [0.75] * w])


def test_refusals_leave_the_outputs_untouched(eng):
    h, w = 6, 8
    ds = [dev(torch.from_numpy(s)) for s in ref.random_sources(9, 3, h, w, seed=1)]
    dw = [dev(torch.from_numpy(c)) for c in ref.random_weights(9, h, w, seed=2)]
    anchor = torch.full((3, h, w), POISON, device="cuda:0")
    weight = torch.full((h, w), POISON, device="cuda:0")
    parts = torch.full((9, h, w), POISON, device="cuda:0")

    def untouched():
        return bool((anchor == POISON).all() and (weight == POISON).all() and (parts == POISON).all())

    assert _raw(eng, ds[:2], dw[:2], anchor, weight, parts, J=0) == E_ARG and untouched()
    assert _raw(eng, ds, dw, anchor, weight, parts, J=9) == E_ARG and untouched()
    assert _raw(eng, ds[:2], dw[:2], anchor, weight, parts, C_=2) == E_ARG and untouched()
    before = ds[1].clone()
    assert _raw(eng, ds[:3], dw[:3], ds[1], weight, parts) == E_ARG and untouched() and torch.equal(ds[1], before)
    assert _raw(eng, ds[:3], dw[:3], anchor, dw[2], parts) == E_ARG and untouched()
    assert _raw(eng, ds[:3], dw[:3], anchor, weight, anchor.view(-1)[h * w:].view(2, h, w)) == E_ARG and untouched()
    assert _raw(eng, ds[:3], dw[:3], anchor, weight, None) == 0 and not (anchor == POISON).any() and bool((parts == POISON).all())


@pytest.mark.parametrize("h,w", [(25, 41), (33, 128)])
def test_the_identity_on_the_device(eng, h, w):
    """J = 3, C = 3, through nst_anchor_loss.  With G the fp64 gradient of the three-term loss sum_j l_j (y - a_j)^2 / n:
    (a) the device's gradient under the folded (a~, W) is within 3 x the torch-fp32 distance of that evaluation from G;
    (b) it is within 3 x (that distance + the torch-fp32 distance of the three-term evaluation from G) of the sum of the
        device's three gradients under (a_j, l_j) - both sides are fp32 evaluations of G, each held to its own bound;
    (c) (sum_j tmp_j) - tmp_fold is the restatement's constant to 1e-6 of (sum_j tmp_j + tmp_fold) (a value of the term is
        held to 1e-6 relative, tests/test_hip_temporal.py) plus what the rounding of a~ moves tmp_fold by, at most
        2 mean(W |y - a~|) times six roundings of values below 256 (the difference, the ratio, the product and two sums):
        6 x 2^-24 x 256;
    (d) with weights of 0 and 1 the restatement's constant is exactly 0, the two gradients are equal entry by entry - every
        sum has one term that is not zero - and the values agree to the first part of (c)'s tolerance alone."""
    J, C_ = 3, 3
    n = C_ * h * w
    y = np.random.RandomState(3).uniform(-120.0, 135.0, (C_, h, w)).astype(np.float32)
    sources = ref.random_sources(J, C_, h, w, seed=4)
    yd = dev(torch.from_numpy(y))[None]
    for binary in (False, True):
        weights = ref.random_weights(J, h, w, seed=5)
        if binary:
            weights = [(c > 0.6).astype(np.float32) for c in weights]
        ds, dw = [dev(torch.from_numpy(s)) for s in sources], [dev(torch.from_numpy(c)) for c in weights]
        anchor, weight, parts = eng.anchor_fold(ds, dw, want_parts=True)
        tmp_fold, g_fold = eng.anchor_loss(yd, anchor[None], weight, want_grad=True)
        tmp_j, g_j = zip(*[eng.anchor_loss(yd, ds[j][None], parts[j].contiguous(), want_grad=True) for j in range(J)])
        g_sum = (g_j[0] + g_j[1]) + g_j[2]
        a64, w64, p64, _ = ref.fold(sources, weights)
        p64m = [np.where(p64[j] > 0, 1.0, 0.0) for j in range(J)]
        yt = torch.from_numpy(y)[None]
        G = sum(temporal_ref.anchor_piece(yt, torch.from_numpy(sources[j])[None], torch.from_numpy(p64[j]), torch.float64)[1]
                for j in range(J)).numpy()
        _, w32, p32, _ = ref.fold(sources, weights, np.float32)
        a32 = ref.fold_torch(sources, weights)
        g32_fold = temporal_ref.anchor_piece(yt, torch.from_numpy(a32)[None], torch.from_numpy(w32), torch.float32)[1].numpy()
        g32_sum = sum(temporal_ref.anchor_piece(yt, torch.from_numpy(sources[j])[None], torch.from_numpy(p32[j]), torch.float32)[1]
                      for j in range(J)).numpy()
        e_fold, e_pair = rel_l2(g_fold.cpu().numpy(), G), rel_l2(g_fold.cpu().numpy(), g_sum.cpu().numpy())
        b_fold, b_sum = rel_l2(g32_fold, G), rel_l2(g32_sum, G)
        vals = [float(t.cpu()) for t in tmp_j]
        diff = sum(vals) - float(tmp_fold.cpu())
        const = ref.constant(sources, p64)
        fold64 = float((w64[None] * (y.astype(np.float64) - a64) ** 2).sum()) / n
        sens = 2.0 * float((w64[None] * np.abs(y - a64)).mean()) * 6 * 2.0 ** -24 * 256
        tol = 1e-6 * (const + 2 * fold64) + (0.0 if binary else sens)
        report(f"long-term identity {h}x{w} {'binary' if binary else 'fractional'} weights: gradient under (a~, W) to the fp64 three-term "
               f"gradient rel-L2 {e_fold:.2e} (torch fp32 {b_fold:.2e}), to the device's three-term sum {e_pair:.2e} (torch fp32 three-term "
               f"{b_sum:.2e}); sum tmp_j - tmp_fold = {diff:.6e}, constant {const:.6e} (tolerance {tol:.1e})")
        assert e_fold <= 3 * b_fold and e_pair <= 3 * (b_fold + b_sum), (e_fold, b_fold, e_pair, b_sum)
        assert abs(diff - const) <= tol, (diff, const, tol)
        if binary:
            assert const == 0.0 and sum(p64m).max() <= 1
            assert torch.equal(g_fold, g_sum)


# ================================================================================================ the driver
def _run(fn, frames, style, *flows, cfg, **kw):
    async def go():
        return [(i, p, img) async for i, p, img in fn(frames, style, *flows, temporal_weight=1e9, cfg=cfg, **kw)]
    return asyncio.run(go())


def test_video_driver_takes_an_uncovered_region_from_two_frames_back(vgg_weights):
    """Three 64x96 frames yielding 512x768: f0; f1 = f0 with an occluder on rows 16..31, columns 24..47; f2 = f0.  Zero
    flows; the offset-1 weights of frame 2 are 0 on the occluder's rectangle at the yielded size (rows 128..255, columns
    192..383) - what it covered has no anchor in frame 1 - and 1 elsewhere; long_term=(2,) with zero flows and weights of
    ones.  Frames 0 and 1 are bitwise those of the run without long_term; the fold of the recorded results takes the
    rectangle from frame 0 and everything else from frame 1; over the rectangle frame 2 ends nearer frame 0's result with
    long_term than without; outside it both runs are held to frame 1 alike."""
    from artstyletransfer_amd import config, neural_nets, video
    from artstyletransfer_amd.neural_nets import shared_engine
    neural_nets.set_weights(vgg_weights)
    f0 = cpu_ref.synthetic_image(64, 96, seed=1)
    f1 = f0.copy()
    f1[16:32, 24:48] = cpu_ref.synthetic_image(64, 96, seed=3)[16:32, 24:48]
    frames = [f0, f1, f0.copy()]
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=2, iters_num=4, optimizer="adam", init_method="content")
    hh, ww = video.result_size(f0.shape, 2)
    assert (hh, ww) == (512, 768)
    zero = np.zeros((hh, ww, 2), np.float32)
    ones = np.ones((hh, ww), np.float32)
    holed = ones.copy()
    holed[128:256, 192:384] = 0.0
    rect = holed == 0
    short = _run(video.neural_style_transfer_video, frames, style, [zero, zero], None, [ones, holed], cfg=cfg)
    long_ = _run(video.neural_style_transfer_video_long_term, frames, style, [zero, zero], None, [ones, holed], cfg=cfg,
                 long_term=(2,), long_term_flows={2: ([zero], None, [ones])})
    assert [(i, p) for i, p, _ in long_] == [(i, p) for i in range(3) for p in (25.0, 50.0, 75.0, 100.0)] == [(i, p) for i, p, _ in short]
    for a, b in zip(short[:8], long_[:8]):
        assert np.array_equal(_bits(a[2]), _bits(b[2]))
    r0, r1 = long_[3][2], long_[7][2]
    e = shared_engine(torch.device("cuda", torch.cuda.current_device()))
    chw = lambda img: dev(torch.from_numpy(img).permute(2, 0, 1))
    z = dev(torch.zeros((2, hh, ww)))
    omega, c, parts = video.long_term_anchor(e, [chw(r1), chw(r0)], [z, z], None, [dev(torch.from_numpy(holed)), dev(torch.from_numpy(ones))])
    parts = parts.cpu().numpy()
    assert np.array_equal(parts[1], rect.astype(np.float32)) and np.array_equal(parts[0], holed) and bool((c == 1).all())
    want = np.where(rect[..., None], r0, r1)
    assert np.array_equal(_bits(omega.permute(1, 2, 0)), _bits(want))
    msd = lambda a, b, m: float(((a.astype(np.float64) - b.astype(np.float64)) ** 2)[m].mean())
    d_long, d_short = msd(long_[-1][2], r0, rect), msd(short[-1][2], r0, rect)
    o_long, o_short = msd(long_[-1][2], r1, ~rect), msd(short[-1][2], r1, ~rect)
    report(f"long-term driver 512x768, 4 Adam steps, occluder rectangle 128x192: msd(frame 2, frame 0's result) over the rectangle "
           f"{d_long:.4e} with long_term=(2,), {d_short:.4e} without; msd(frame 2, frame 1's result) outside it {o_long:.4e} / {o_short:.4e}")
    assert np.isfinite(long_[-1][2]).all() and d_long < d_short
    assert 0.5 * o_short <= o_long <= 2.0 * o_short


def test_video_driver_with_estimated_flows_covers_what_a_moving_object_uncovers(vgg_weights, monkeypatch):
    """Three 64x96 frames: a static textured background and a differently textured 16x20 rectangle that moves 2 px per frame
    (16 px at the 512x768 yielded) - to the right, then back, so that the band frame 2 uncovers was visible in frame 0.
    TVL1Params(), long_term=(2,), one iteration.  From the planes the driver formed for frame 2: W >= c_1 at every pixel
    (the definition); the uncovered band, known in closed form, has at least 1000 pixels; the share of its pixels with W = 1
    is strictly larger than the share with c_1 = 1."""
    from artstyletransfer_amd import config, neural_nets, video
    from artstyletransfer_amd.flow_modes import TVL1Params
    neural_nets.set_weights(vgg_weights)
    back = cpu_ref.synthetic_image(64, 96, seed=1)
    obj = cpu_ref.synthetic_image(64, 96, seed=4)
    y0, x0, rh, rw = 24, 30, 16, 20
    frames = []
    for x in (x0, x0 + 2, x0):
        f = back.copy()
        f[y0:y0 + rh, x:x + rw] = obj[:rh, :rw]
        frames.append(f)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=2, iters_num=1, optimizer="adam", init_method="content")
    hh, ww = video.result_size(back.shape, 2)
    assert (hh, ww) == (512, 768)
    seen = []
    inner = video.long_term_anchor

    def recording(engine, results_chw, backward, forward=None, weights=None):
        out = inner(engine, results_chw, backward, forward, weights)
        seen.append((len(results_chw), out[1].cpu().numpy(), out[2].cpu().numpy()))
        return out

    monkeypatch.setattr(video, "long_term_anchor", recording)
    out = _run(video.neural_style_transfer_video_long_term, frames, style, TVL1Params(), cfg=cfg, long_term=(2,))
    assert [(i, p) for i, p, _ in out] == [(0, 100.0), (1, 100.0), (2, 100.0)] and np.isfinite(out[-1][2]).all()
    assert [s[0] for s in seen] == [1, 2]
    _, W, parts = seen[1]
    c1 = parts[0]
    assert set(np.unique(c1)) <= {0.0, 1.0} and (W >= c1).all()
    band = np.zeros((hh, ww), bool)
    band[8 * y0:8 * (y0 + rh), 8 * (x0 + rw):8 * (x0 + rw + 2)] = True      # covered in frame 1, free in frames 0 and 2
    assert band.sum() == 8 * rh * 16 >= 1000
    share_w, share_c1 = float((W[band] == 1).mean()), float((c1[band] == 1).mean())
    report(f"long-term driver, estimated TV-L1 flows 512x768: uncovered band of {int(band.sum())} pixels, share with W = 1 {share_w:.4f}, "
           f"with c_1 = 1 {share_c1:.4f}; whole image W = 1 {float((W == 1).mean()):.4f}, c_1 = 1 {float((c1 == 1).mean()):.4f}")
    assert share_w > share_c1
