"""GPU: the flow estimator (nst_flow_estimate, nst_flow_reduce, nst_flow_prolong, nst_flow_linearize, nst_flow_sweeps; multi-scale
Horn-Schunck with warping) against the restatement of the definitions in include/nst_hip.h (tests/flow_ref.py), and the video
driver that estimates its own flows.

Bounds.  Every stage, and the whole estimate: at most 3 x the distance of the fp32 restatement of the same formula from the fp64
one, in max-abs and in relative L2 (the margin tests/test_hip_temporal.py gives fp32 arithmetic in another order; the kernels
keep the header's order, so in practice they give the restatement's bits).  The device's mean endpoint error may exceed the
fp64 restatement's by no more than the estimate's bound.  Identical frames, repeated runs, a refused call and nst_ctx_bytes:
exact.  The measured figures are in profiles/r17_flow.txt.

Shapes: the smallest that reach every branch - 1x1 and one-row / one-column planes (replicated borders on both sides at once),
sizes below one group of four, 33x130 (rows that start on and off a 16-byte boundary, more than 32 groups of four and a tail
of two pixels)."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch

import flow_ref as ref
from oracle import cpu_ref
from hip_helpers import dev, rel_l2, report

pytestmark = pytest.mark.gpu

E_ARG = -1
PARAM_SETS = ({}, {"scales": 1})


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


def _hold(what, got, f64, f32):
    """got (device result, numpy) against fp64 under 3 x the fp32 restatement's own distance, max-abs and rel-L2."""
    got, f64, f32 = (np.asarray(a, np.float64) for a in (got, f64, f32))
    assert got.shape == f64.shape, (what, got.shape, f64.shape)
    a_dev, a_32 = float(np.abs(got - f64).max()), float(np.abs(f32 - f64).max())
    r_dev, r_32 = rel_l2(got, f64), rel_l2(f32, f64)
    report(f"flow {what}: max-abs {a_dev:.3e} (fp32 restatement {a_32:.3e}), rel-L2 {r_dev:.3e} (fp32 restatement {r_32:.3e})")
    assert a_dev <= 3 * a_32 and r_dev <= 3 * r_32, (what, a_dev, a_32, r_dev, r_32)


def _image(h, w, seed):
    return np.random.RandomState(seed).uniform(0.0, 255.0, (h, w)).astype(np.float32)


# ================================================================================================ the stages against fp64
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (5, 7), (16, 24), (33, 130)])
def test_reduce_against_fp64(eng, shape):
    a = _image(*shape, seed=11)
    got = eng.flow_reduce(dev(torch.from_numpy(a))).cpu().numpy()
    _hold(f"reduce {shape}", got, ref.reduce(a, np.float64), ref.reduce(a, np.float32))


@pytest.mark.parametrize("fine", [(5, 7), (6, 8), (1, 1), (2, 2)])
def test_prolong_against_fp64(eng, fine):
    h, w = fine
    c = np.random.RandomState(12).uniform(-4.0, 4.0, (2, (h + 1) // 2, (w + 1) // 2)).astype(np.float32)
    got = eng.flow_prolong(dev(torch.from_numpy(c)), h, w).cpu().numpy()
    _hold(f"prolong {c.shape[1:]} -> {fine}", got, ref.prolong(c, h, w, np.float64), ref.prolong(c, h, w, np.float32))


def _linearise_flow(h, w, seed):
    """Fractional flows of up to 3 pixels; a block of zero flow, a block of integer flows; borders whose samples leave the
    image on each of the four sides (the corners on two at once)."""
    rng = np.random.RandomState(seed)
    f = rng.uniform(-3.0, 3.0, (2, h, w)).astype(np.float32)
    f[:, h // 3: h // 3 + 2, w // 3: w // 3 + 3] = 0.0
    f[0, h // 2: h // 2 + 2, 2: w // 2] = 2.0
    f[1, h // 2: h // 2 + 2, 2: w // 2] = -1.0
    f[0, :, 0] = -5.5
    f[0, :, -1] = 5.25
    f[1, 0, :] = -4.5
    f[1, -1, :] = 4.75
    return f


@pytest.mark.parametrize("shape", [(9, 13), (33, 130)])
def test_linearise_against_fp64(eng, shape):
    h, w = shape
    A, B, f = _image(h, w, 21), _image(h, w, 22), _linearise_flow(h, w, 23)
    got = [t.cpu().numpy() for t in eng.flow_linearize(dev(torch.from_numpy(A)), dev(torch.from_numpy(B)), dev(torch.from_numpy(f)))]
    w64, w32 = ref.linearize(A, B, f, np.float64), ref.linearize(A, B, f, np.float32)
    zero = w64[0] == 0
    assert 0.05 < zero.mean() < 0.7 and zero[:, 0].all() and zero[:, -1].all() and zero[0].all() and zero[-1].all()
    for name, g, a, b in zip(("Ix", "Iy", "rho"), got, w64, w32):
        assert not g[(w64[0] == 0) & (w64[1] == 0) & (w64[2] == 0)].any(), name        # no data term: exact zeros
        _hold(f"linearise {shape} {name}", g, a, b)
    # a non-finite flow: no data term either
    f[0, 4, 5] = np.nan
    f[1, 5, 6] = np.inf
    got = [t.cpu().numpy() for t in eng.flow_linearize(dev(torch.from_numpy(A)), dev(torch.from_numpy(B)), dev(torch.from_numpy(f)))]
    assert all(g[4, 5] == 0 and g[5, 6] == 0 and np.isfinite(g).all() for g in got)


def _placed(a, offset):
    """The array on the device, `offset` floats past a 16-byte boundary."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device="cuda:0")
    lead = (-(buf.data_ptr() // 4)) % 4 + offset
    t = buf[lead: lead + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and (t.data_ptr() // 4) % 4 == offset % 4
    return t


def _sweep_groups(h, w, un, vn, u, v, ix, iy, rho):
    """flow.hip's rule for the groups of a sweep, restated on the addresses (in bytes) of the seven planes: how many groups
    of four take 16 bytes per lane on every plane with the rows above and below wide too ("full"), how many with a row above
    or below off a boundary ("mixed"), how many groups take single floats ("narrow"); the longest run of pixels before a
    row's first boundary and the longest tail."""
    full = mixed = narrow = head_max = tail_max = 0
    for y in range(h):
        off, up, dn = y * w, max(y - 1, 0) * w, min(y + 1, h - 1) * w
        head = min(((16 - (un + 4 * off) % 16) % 16) // 4, w)
        head_max = max(head_max, head)
        narrow += head > 0
        for x0 in range(head, w, 4):
            n = min(x0 + 4, w) - x0
            if n == 4 and all((p + 4 * (off + x0)) % 16 == 0 for p in (un, vn, u, v, ix, iy, rho)):
                rows = all((p + 4 * (r + x0)) % 16 == 0 for p in (u, v) for r in (up, dn))
                full, mixed = full + rows, mixed + (not rows)
            else:
                narrow += 1
                if n < 4:
                    tail_max = max(tail_max, n)
    return dict(full=full, mixed=mixed, narrow=narrow, head=head_max, tail=tail_max)


# shape, floats past a boundary at which every plane starts, and the groups the kernel must form there (_sweep_groups).  The
# planes of a (2,h,w) flow are h w floats apart: with h w % 4 != 0 (the first five) no group is wide.
SWEEP_CASES = [
    ((1, 1), 0, dict(full=0, mixed=0, narrow=1, head=0, tail=1)),
    ((1, 9), 0, dict(full=0, mixed=0, narrow=3, head=0, tail=1)),
    ((9, 1), 0, dict(full=0, mixed=0)),
    ((3, 5), 0, dict(full=0, mixed=0)),
    ((33, 130), 0, dict(full=0, mixed=0, tail=2)),                            # rows on and off a boundary, single floats throughout
    ((8, 12), 0, dict(full=24, mixed=0, narrow=0, head=0, tail=0)),           # every row on a boundary: wide everywhere
    ((4, 136), 0, dict(full=136, mixed=0, narrow=0)),                         # rows of 34 wide groups
    ((34, 130), 0, dict(full=0, mixed=34 * 32, head=2, tail=2)),              # wide centre rows, rows above and below off a boundary
    ((8, 12), 1, dict(full=16, mixed=0, narrow=16, head=3, tail=1)),          # three pixels before each row's first boundary, a tail of one
]


@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("shape,offset,groups", SWEEP_CASES)
def test_sweeps_against_fp64(eng, shape, offset, groups, n):
    from artstyletransfer_amd import engine as E
    h, w = shape
    rng = np.random.RandomState(31 + n)
    ix, iy = (rng.uniform(-30.0, 30.0, (h, w)).astype(np.float32) for _ in range(2))
    rho = rng.uniform(-20.0, 20.0, (h, w)).astype(np.float32)
    flow = rng.uniform(-3.0, 3.0, (2, h, w)).astype(np.float32)
    none = rng.uniform(0.0, 1.0, (h, w)) < 0.2            # pixels without a data term
    ix[none] = iy[none] = rho[none] = 0.0
    dix, diy, drho, dflow = (_placed(a, offset) for a in (ix, iy, rho, flow))
    poison = np.full((2, h, w), -777.0, np.float32)
    out, scratch = _placed(poison, offset), _placed(poison, offset)
    # the kernel forms the groups this case is here for - in every launch, whichever of out and scratch it writes
    for dst, src in ((out, dflow), (scratch, out), (out, scratch)):
        got = _sweep_groups(h, w, dst.data_ptr(), dst.data_ptr() + 4 * h * w, src.data_ptr(), src.data_ptr() + 4 * h * w,
                            dix.data_ptr(), diy.data_ptr(), drho.data_ptr())
        assert {k: got[k] for k in groups} == groups, (shape, offset, got)
    E._lib.check(eng.ctx, eng.lib.nst_flow_sweeps(eng.ctx, E._ptr(dix), E._ptr(diy), E._ptr(drho), E._ptr(dflow), h, w, 15.0, n, E._ptr(out),
                                                 E._ptr(scratch if n > 1 else None), E._stream(eng.device)), "nst_flow_sweeps")
    assert np.array_equal(_bits(dflow), torch.from_numpy(flow).view(torch.int32).numpy())          # flow_in is left as it is
    if offset == 0:      # the engine's own call gives the same bits
        assert np.array_equal(_bits(eng.flow_sweeps(dix, diy, drho, dflow, 15.0, n)), _bits(out))
    _hold(f"sweeps {shape} n={n} planes {offset} floats past a boundary", out.cpu().numpy(), ref.sweeps(ix, iy, rho, flow, 15.0, n, np.float64),
          ref.sweeps(ix, iy, rho, flow, 15.0, n, np.float32))


def test_stages_refuse_overlapping_buffers_and_an_alpha_whose_square_is_not_positive(eng):
    from artstyletransfer_amd import engine as E
    h, w = 8, 12
    buf = torch.zeros(16 * h * w, dtype=torch.float32, device="cuda:0")
    P = lambda k: C.c_void_p(buf.data_ptr() + 4 * k * h * w)           # plane k of the buffer
    st = E._stream(eng.device)
    assert eng.lib.nst_flow_reduce(eng.ctx, P(0), h, w, P(0), st) == E_ARG
    assert eng.lib.nst_flow_reduce(eng.ctx, P(0), h, w, C.c_void_p(buf.data_ptr() + 4 * (h * w - 1)), st) == E_ARG      # the last float
    assert eng.lib.nst_flow_reduce(eng.ctx, P(0), h, w, P(1), st) == 0
    assert eng.lib.nst_flow_prolong(eng.ctx, P(0), h, w, P(0), st) == E_ARG
    assert eng.lib.nst_flow_prolong(eng.ctx, P(0), h, w, P(1), st) == 0           # (coarse: half a plane)
    for ix, iy, rho in ((0, 5, 6), (4, 1, 6), (4, 5, 3), (4, 4, 6), (4, 5, 5), (6, 5, 6)):
        assert eng.lib.nst_flow_linearize(eng.ctx, P(0), P(1), P(2), h, w, P(ix), P(iy), P(rho), st) == E_ARG, (ix, iy, rho)
    assert eng.lib.nst_flow_linearize(eng.ctx, P(0), P(1), P(2), h, w, P(4), P(5), P(6), st) == 0
    for fin, out, scr, n in ((3, 3, 7, 2), (3, 4, 7, 2), (3, 5, 3, 2), (3, 5, 6, 2), (3, 0, 7, 2), (3, 5, 2, 2), (3, 2, 7, 1)):
        assert eng.lib.nst_flow_sweeps(eng.ctx, P(0), P(1), P(2), P(fin), h, w, 15.0, n, P(out), P(scr), st) == E_ARG, (fin, out, scr, n)
    assert eng.lib.nst_flow_sweeps(eng.ctx, P(0), P(1), P(2), P(3), h, w, 15.0, 2, P(5), P(7), st) == 0
    assert eng.lib.nst_flow_sweeps(eng.ctx, P(0), P(1), P(2), P(3), h, w, 15.0, 1, P(5), P(3), st) == 0          # n = 1: scratch is not read
    for alpha in (1e-30, 1e-22, 1e20, 0.0, float("nan")):
        assert eng.lib.nst_flow_sweeps(eng.ctx, P(0), P(1), P(2), P(3), h, w, alpha, 2, P(5), P(7), st) == E_ARG, alpha
    # all zeros in, so all zeros out - and no NaN where a pixel has no data term, at the smallest alpha accepted
    assert eng.lib.nst_flow_sweeps(eng.ctx, P(0), P(1), P(2), P(3), h, w, 1e-18, 2, P(5), P(7), st) == 0
    assert not _bits(buf).any()


# ================================================================================================ the estimate
@pytest.fixture(scope="module")
def pipeline():
    """(pair, parameter set) -> (from, to, fp64 flow, fp32 flow) of the restatement; computed once."""
    out = {}
    for k, (shape, t, seed) in enumerate(ref.PAIRS):
        A, B = ref.synthetic_pair(shape, t, seed)
        for j, kw in enumerate(PARAM_SETS):
            out[k, j] = (A, B, ref.estimate(A, B, np.float64, **kw)[0], ref.estimate(A, B, np.float32, **kw)[0])
    return out


@pytest.mark.parametrize("j", range(len(PARAM_SETS)))
@pytest.mark.parametrize("k", range(len(ref.PAIRS)))
def test_estimate_against_the_fp64_restatement(eng, pipeline, k, j):
    from artstyletransfer_amd.flow_modes import FlowParams
    shape, t, _ = ref.PAIRS[k]
    A, B, f64, f32 = pipeline[k, j]
    got = eng.flow_estimate(dev(torch.from_numpy(A)), dev(torch.from_numpy(B)), FlowParams(**PARAM_SETS[j])).cpu().numpy()
    r_dev, r_32 = rel_l2(got, f64), rel_l2(f32, f64)
    e_dev, e_64 = ref.endpoint_error(got, t), ref.endpoint_error(f64, t)
    report(f"flow estimate {shape} t={t} {PARAM_SETS[j] or 'defaults'}: rel-L2 {r_dev:.3e} (fp32 restatement {r_32:.3e}, bound "
           f"{3 * r_32:.3e}); mean endpoint error {e_dev:.6f} px (fp64 restatement {e_64:.6f} px)")
    assert got.shape == (2,) + shape and r_dev <= 3 * r_32
    assert e_dev <= e_64 + 3 * r_32 and e_dev < 0.5


def test_identical_frames_give_exactly_zero_flow(eng):
    for shape, _, seed in ref.PAIRS:
        A = dev(torch.from_numpy(ref.synthetic_pair(shape, (0.0, 0.0), seed)[0]))
        assert not _bits(eng.flow_estimate(A, A.clone())).any()


def test_two_runs_give_the_same_bits_and_the_context_allocates_nothing(eng):
    A, B = (dev(torch.from_numpy(a)) for a in ref.synthetic_pair((33, 130), (1.25, -0.75), 7))
    before = eng.bytes()
    one = eng.flow_estimate(A, B)
    two = eng.flow_estimate(A, B)
    assert eng.bytes() == before
    assert np.array_equal(_bits(one), _bits(two)) and np.isfinite(one.cpu().numpy()).all() and one.abs().max() > 0.1


def test_refusals_launch_nothing_and_leave_the_output_untouched(eng):
    from artstyletransfer_amd import engine as E
    h, w = 33, 47
    A, B = (dev(torch.from_numpy(a)) for a in ref.synthetic_pair((h, w), (1.5, 0.5), 3))
    floats, used = E.flow_workspace(h, w, 0)
    assert used == 3
    work = torch.empty(floats, dtype=torch.float32, device=A.device)
    poison = float(np.float32(-1234.5))
    out = torch.full((2, h, w), poison, dtype=torch.float32, device=A.device)
    stream = E._stream(eng.device)

    def call(a=A, b=B, hh=h, ww=w, alpha=15.0, scales=0, warps=5, iterations=50, o=out, wk=work, n=floats):
        return eng.lib.nst_flow_estimate(eng.ctx, E._ptr(a), E._ptr(b), hh, ww, alpha, scales, warps, iterations, E._ptr(o), E._ptr(wk), n, stream)

    refused = [dict(n=floats - 1), dict(a=None), dict(b=None), dict(o=None), dict(wk=None), dict(hh=0), dict(ww=0), dict(alpha=0.0),
               dict(alpha=-15.0), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=1e-30), dict(alpha=1e20), dict(o=A), dict(wk=out), dict(warps=0), dict(iterations=0), dict(scales=-1),
               dict(scales=13)]
    for kw in refused:
        assert call(**kw) == E_ARG, kw
        assert (out == poison).all(), kw
    with pytest.raises(E.NstError, match="workspace"):
        E._lib.check(eng.ctx, call(n=floats - 1), "nst_flow_estimate")
    assert call() == 0 and not (out == poison).any()
    assert np.array_equal(_bits(out), _bits(eng.flow_estimate(A, B)))


# ================================================================================================ the driver
def test_video_driver_estimates_the_flows_it_is_not_given(vgg_weights):
    """Two 64x96 frames, the second the first moved one pixel to the right (8 pixels at the 512x768 a two-level job yields),
    Adam, two iterations, temporal weight 1e9.  backward_flows=None yields the bits of a run that is handed the flows
    StyleEngine.flow_estimate gives for the same luminance planes, forward flows included; and frame 1's first yielded image
    is closer to the warped frame-0 result than the first image of the same frame run without an anchor."""
    from artstyletransfer_amd import config, neural_nets, video
    from artstyletransfer_amd.neural_nets import shared_engine
    neural_nets.set_weights(vgg_weights)
    f0 = cpu_ref.synthetic_image(64, 96, seed=1)
    f1 = np.roll(f0, 1, axis=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=2, iters_num=2, optimizer="adam", init_method="content")
    hh, ww = video.result_size(f0.shape, 2)
    assert (hh, ww) == (512, 768)

    def run(frames, *flows):
        async def go():
            return [(i, p, img) async for i, p, img in video.neural_style_transfer_video(frames, style, *flows, temporal_weight=1e9, cfg=cfg)]
        return asyncio.run(go())

    own = run([f0, f1])
    assert [(i, p) for i, p, _ in own] == [(0, 50.0), (0, 100.0), (1, 50.0), (1, 100.0)]
    e = shared_engine(torch.device("cuda", torch.cuda.current_device()))
    p0, p1 = (e.luminance(e.resize(dev(torch.from_numpy(f)), hh, ww)).reshape(hh, ww) for f in (f0, f1))
    bwd, fwd = e.flow_estimate(p1, p0), e.flow_estimate(p0, p1)
    handed = run([f0, f1], [bwd.permute(1, 2, 0).cpu().numpy()], [fwd.permute(1, 2, 0).cpu().numpy()])
    for a, b in zip(own, handed):
        assert a[:2] == b[:2] and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    # the estimate itself: the frames differ by 8 pixels along x (the backward flow points left), away from the wrapped border
    inner = bwd[:, 64:-64, 64:-64].cpu().numpy()
    report(f"video driver 512x768: estimated backward flow, inner mean ({inner[0].mean():.3f}, {inner[1].mean():.3f}) px for a true (-8, 0)")
    assert abs(inner[0].mean() + 8.0) < 1.0 and abs(inner[1].mean()) < 1.0
    omega, valid = e.warp_bilinear(dev(torch.from_numpy(own[1][2]).permute(2, 0, 1)), bwd)
    omega = omega.permute(1, 2, 0).cpu().numpy().astype(np.float64)
    c = valid.cpu().numpy() == 1
    alone = run([f1])
    d_own = float(((own[2][2].astype(np.float64) - omega) ** 2)[c].mean())
    d_alone = float(((alone[0][2].astype(np.float64) - omega) ** 2)[c].mean())
    report(f"video driver 512x768: msd(frame 1's first image, warped frame 0) {d_own:.4e} from the warped start, {d_alone:.4e} without an anchor")
    assert c.mean() > 0.9 and np.isfinite(own[-1][2]).all() and d_own < d_alone
