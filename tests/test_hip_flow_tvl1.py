"""GPU: the TV-L1 flow estimator (nst_flow_tvl1_estimate, nst_flow_tvl1_iterations, nst_flow_tvl1_workspace) against the
restatement of the definitions in include/nst_hip.h (tests/flow_tvl1_ref.py), beside Horn-Schunck on the device, and the video
driver handed a TVL1Params.

Bounds.  The stage and the whole estimate: test_hip_flow's _hold - at most 3 x the distance of the fp32 restatement of the same
formula from the fp64 one, in max-abs and in relative L2 (the kernel keeps the header's order of operations, so in practice it
gives the restatement's bits; the test reports whether it does).  The device's mean endpoint error may exceed the fp64
restatement's by no more than the estimate's bound, and is at most half of the device's Horn-Schunck error on every scene and
pair.  Identical frames, repeated runs, the duals' last column / row, untouched inputs, refused calls and nst_ctx_bytes: exact.
The measured figures are in profiles/r18_flow_tvl1.txt.

Shapes of the stage: 1x1, one row, one column (every difference degenerate on one axis), 5x7 (below two groups, h w odd),
8x12 (every group takes 16 bytes on all fifteen planes), 34x130 (h w a multiple of 4 but not w: the rows above and below a
wide group lie off a boundary; a head and a tail of two), 8x12 with every buffer one float past a boundary (three pixels
before each row's first boundary, a tail of one)."""
import asyncio
import ctypes as C

import numpy as np
import pytest
import torch

import flow_ref as hs
import flow_tvl1_ref as ref
from oracle import cpu_ref
from hip_helpers import dev, rel_l2, report
from test_hip_flow import _bits, _hold, _placed

pytestmark = pytest.mark.gpu

E_ARG = -1
L, TH, TAU = 0.15, 0.3, 0.25
PARAM_SETS = ({}, {"scales": 1})


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


# ================================================================================================ the stage against fp64
def _groups(h, w, fo, po, f, p, ix, iy, rho):
    """flow_tvl1.hip's rule for the groups of an iteration, restated on the addresses (in bytes) of the buffers (the planes of a
    flow and of the duals are h w floats apart): how many groups of four take 16 bytes per lane on all fifteen planes with the
    rows above and below wide too ("full": w a multiple of 4), how many with those rows off a boundary ("mixed"), how many
    groups take single floats ("narrow"); the longest run of pixels before a row's first boundary and the longest tail."""
    full = mixed = narrow = head_max = tail_max = 0
    for y in range(h):
        off = y * w
        head = min(((16 - (fo + 4 * off) % 16) % 16) // 4, w)
        head_max = max(head_max, head)
        narrow += head > 0
        for x0 in range(head, w, 4):
            n = min(x0 + 4, w) - x0
            if n == 4 and (h * w) % 4 == 0 and all((q + 4 * (off + x0)) % 16 == 0 for q in (fo, po, f, p, ix, iy, rho)):
                full, mixed = full + (w % 4 == 0), mixed + (w % 4 != 0)
            else:
                narrow += 1
                if n < 4:
                    tail_max = max(tail_max, n)
    return dict(full=full, mixed=mixed, narrow=narrow, head=head_max, tail=tail_max)


# shape, floats past a boundary at which every buffer starts, and the groups the kernel must form there (_groups)
STAGE_CASES = [
    ((1, 1), 0, dict(full=0, mixed=0, narrow=1, head=0, tail=1)),
    ((1, 9), 0, dict(full=0, mixed=0, narrow=3, head=0, tail=1)),
    ((9, 1), 0, dict(full=0, mixed=0)),
    ((5, 7), 0, dict(full=0, mixed=0)),
    ((8, 12), 0, dict(full=24, mixed=0, narrow=0, head=0, tail=0)),
    ((34, 130), 0, dict(full=0, mixed=34 * 32, head=2, tail=2)),
    ((8, 12), 1, dict(full=16, mixed=0, narrow=16, head=3, tail=1)),
]


@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("shape,offset,groups", STAGE_CASES)
def test_iterations_against_fp64(eng, shape, offset, groups, n):
    from artstyletransfer_amd import engine as E
    h, w = shape
    rng = np.random.RandomState(41 + n)
    ix, iy = (rng.uniform(-30.0, 30.0, (h, w)).astype(np.float32) for _ in range(2))
    rho = rng.uniform(-20.0, 20.0, (h, w)).astype(np.float32)
    flow = rng.uniform(-3.0, 3.0, (2, h, w)).astype(np.float32)
    sign = np.where(rng.uniform(size=(4, h, w)) < 0.5, -1.0, 1.0)
    dual = (sign * rng.uniform(0.05, 0.95, (4, h, w))).astype(np.float32)          # non-zero everywhere, the last column / row too
    none = rng.uniform(0.0, 1.0, (h, w)) < 0.2                                     # pixels without a data term
    ix[none] = iy[none] = rho[none] = 0.0
    dix, diy, drho, dflow, ddual = (_placed(a, offset) for a in (ix, iy, rho, flow, dual))
    out, pout = _placed(np.full((2, h, w), -777.0, np.float32), offset), _placed(np.full((4, h, w), -777.0, np.float32), offset)
    scratch = _placed(np.full((6, h, w), -777.0, np.float32), offset)
    hw4 = 4 * h * w
    where = lambda fl, du: (fl.data_ptr(), du.data_ptr())
    tmp = (scratch.data_ptr(), scratch.data_ptr() + 2 * hw4)
    # the kernel forms the groups this case is here for - in every launch, whichever copy it writes
    for dst, src in ((where(out, pout), where(dflow, ddual)), (tmp, where(out, pout)), (where(out, pout), tmp)):
        got = _groups(h, w, dst[0], dst[1], src[0], src[1], dix.data_ptr(), diy.data_ptr(), drho.data_ptr())
        assert {k: got[k] for k in groups} == groups, (shape, offset, got)

    def run(du, o, po):
        E._lib.check(eng.ctx, eng.lib.nst_flow_tvl1_iterations(eng.ctx, E._ptr(dix), E._ptr(diy), E._ptr(drho), E._ptr(dflow), E._ptr(du), h, w,
                                                              L, TH, TAU, n, E._ptr(o), E._ptr(po), E._ptr(scratch if n > 1 else None),
                                                              E._stream(eng.device)), "nst_flow_tvl1_iterations")

    run(ddual, out, pout)
    # the inputs are left as they are
    assert np.array_equal(_bits(dflow), flow.view(np.int32)) and np.array_equal(_bits(ddual), dual.view(np.int32))
    assert np.array_equal(_bits(dix), ix.view(np.int32)) and np.array_equal(_bits(drho), rho.view(np.int32))
    if n == 1:
        assert (scratch == -777.0).all()
    got_f, got_p = out.cpu().numpy(), pout.cpu().numpy()
    # the last column of p11, p21 and the last row of p12, p22 were read as 0 whatever was passed: they come out 0, and a
    # call handed zeros there gives the same bits
    assert not got_p[0][:, -1].any() and not got_p[2][:, -1].any() and not got_p[1][-1].any() and not got_p[3][-1].any()
    out2, pout2 = torch.full_like(out, -1.0), torch.full_like(pout, -1.0)
    if offset == 0:
        run(dev(torch.from_numpy(ref.read_duals(dual, np.float32))), out2, pout2)
        assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(_bits(pout2), _bits(pout))
        # the engine's own call, and so a second run, gives the same bits
        ef, ep = eng.flow_tvl1_iterations(dix, diy, drho, dflow, ddual, L, TH, TAU, n)
        assert np.array_equal(_bits(ef), _bits(out)) and np.array_equal(_bits(ep), _bits(pout))
    else:
        run(ddual, out, pout)
        assert np.array_equal(out.cpu().numpy().view(np.int32), got_f.view(np.int32))
        assert np.array_equal(pout.cpu().numpy().view(np.int32), got_p.view(np.int32))
    f64, p64 = ref.iterate(ix, iy, rho, flow, dual, L, TH, TAU, n, np.float64)
    f32, p32 = ref.iterate(ix, iy, rho, flow, dual, L, TH, TAU, n, np.float32)
    same = np.array_equal(got_f.view(np.int32), f32.view(np.int32)) and np.array_equal(got_p.view(np.int32), p32.view(np.int32))
    what = f"tvl1 iterations {shape} n={n} buffers {offset} floats past a boundary"
    report(f"flow {what}: the bits of the fp32 restatement: {'yes' if same else 'NO'}")
    _hold(what + " flow", got_f, f64, f32)
    _hold(what + " duals", got_p, p64, p32)


def test_the_stage_refuses_and_leaves_poisoned_outputs_untouched(eng):
    from artstyletransfer_amd import engine as E
    h, w = 8, 12
    hw = h * w
    buf = torch.zeros(40 * hw, dtype=torch.float32, device="cuda:0")
    P = lambda k: C.c_void_p(buf.data_ptr() + 4 * k * hw) if k is not None else C.c_void_p(0)      # plane k of the buffer
    poison = float(np.float32(-1234.5))
    buf[9 * hw:] = poison                                  # outputs: flow 9-10, duals 11-14, scratch 15-20; 21.. spare
    st = E._stream(eng.device)

    def call(ix=0, iy=1, rho=2, fin=3, din=5, hh=h, ww=w, lam=L, th=TH, tau=TAU, n=2, fo=9, do=11, sc=15):
        return eng.lib.nst_flow_tvl1_iterations(eng.ctx, P(ix), P(iy), P(rho), P(fin), P(din), hh, ww, lam, th, tau, n, P(fo), P(do), P(sc), st)

    refused = [dict(ix=None), dict(iy=None), dict(rho=None), dict(fin=None), dict(din=None), dict(fo=None), dict(do=None), dict(sc=None),
               dict(hh=0), dict(ww=0), dict(hh=-1), dict(n=0), dict(n=-2),
               dict(lam=0.0), dict(lam=-0.15), dict(lam=float("nan")), dict(lam=float("inf")), dict(th=0.0), dict(th=-0.3),
               dict(th=float("nan")), dict(th=float("inf")), dict(tau=0.0), dict(tau=-0.25), dict(tau=float("nan")), dict(tau=float("inf")),
               dict(lam=1e-20, th=1e-20), dict(lam=1e20, th=1e20), dict(tau=1e-20, th=1e20), dict(tau=1e20, th=1e-20),
               # an output that overlaps another argument: inputs, and one another
               dict(fo=0), dict(fo=2), dict(fo=3), dict(fo=4), dict(fo=6), dict(do=0), dict(do=4), dict(do=8), dict(do=10), dict(do=9),
               dict(sc=0), dict(sc=8), dict(sc=10), dict(sc=14), dict(sc=4), dict(fo=13), dict(fo=20), dict(do=18)]
    for kw in refused:
        assert call(**kw) == E_ARG, kw
        assert (buf[9 * hw:] == poison).all() and not buf[:9 * hw].any(), kw
    assert call(n=1, sc=None) == 0 and call(n=1, sc=3) == 0          # n = 1: scratch is neither needed nor read
    assert (buf[15 * hw:] == poison).all()
    assert call() == 0
    # all zeros in: all zeros out, and no NaN where no pixel has a data term
    assert not buf[:15 * hw].any() and torch.isfinite(buf[15 * hw: 21 * hw]).all() and (buf[21 * hw:] == poison).all()


# ================================================================================================ the estimate
@pytest.fixture(scope="module")
def cases():
    """name -> (from, to, endpoint error function of a flow -> {region: px}); the pairs of flow_ref and the three scenes."""
    out = {}
    for k, (shape, t, seed) in enumerate(hs.PAIRS):
        A, B = hs.synthetic_pair(shape, t, seed)
        out[f"pair{k}"] = (A, B, lambda f, t=t: {"all": hs.endpoint_error(f, t)})
    for k, sc in enumerate(ref.SCENES):
        A, B, truth, visible, band = ref.scene(*sc)
        out[f"scene{k}"] = (A, B, lambda f, tr=truth, v=visible, b=band: {"visible": ref.endpoint_error(f, tr, v),
                                                                          "band": ref.endpoint_error(f, tr, b)})
    return out


CASES = ["pair0", "pair1", "scene0", "scene1", "scene2"]


@pytest.mark.parametrize("j", range(len(PARAM_SETS)))
@pytest.mark.parametrize("name", CASES)
def test_estimate_against_the_fp64_restatement_and_beside_horn_schunck(eng, cases, name, j):
    from artstyletransfer_amd.flow_modes import FlowParams, TVL1Params
    A, B, epe = cases[name]
    kw = PARAM_SETS[j]
    f64, f32 = ref.estimate(A, B, np.float64, **kw)[0], ref.estimate(A, B, np.float32, **kw)[0]
    dA, dB = dev(torch.from_numpy(A)), dev(torch.from_numpy(B))
    before = eng.bytes()
    got_t = eng.flow_estimate(dA, dB, TVL1Params(**kw))
    again = eng.flow_estimate(dA, dB, TVL1Params(**kw))
    got_hs = eng.flow_estimate(dA, dB, FlowParams(**kw) if kw else None).cpu().numpy()
    assert eng.bytes() == before                                          # the context allocates nothing
    assert np.array_equal(_bits(got_t), _bits(again))                     # two runs: the same bits
    got = got_t.cpu().numpy()
    r_dev, r_32 = rel_l2(got, f64), rel_l2(f32, f64)
    same = np.array_equal(got.view(np.int32), f32.view(np.int32))
    report(f"flow tvl1 estimate {name} {A.shape} {kw or 'defaults'}: rel-L2 {r_dev:.3e} (fp32 restatement {r_32:.3e}, bound {3 * r_32:.3e}); "
           f"the bits of the fp32 restatement: {'yes' if same else 'NO'}")
    assert got.shape == (2,) + A.shape and r_dev <= 3 * r_32
    e_dev, e_64, e_hs, e_hs64 = epe(got), epe(f64), epe(got_hs), epe(hs.estimate(A, B, np.float64, **kw)[0])
    for region in e_dev:
        report(f"flow tvl1 estimate {name} {kw or 'defaults'}: {region} EPE {e_dev[region]:.4f} px (fp64 restatement {e_64[region]:.4f} px; "
               f"Horn-Schunck on the device {e_hs[region]:.4f} px, ratio {e_dev[region] / e_hs[region]:.2f}; ratio of the fp64 "
               f"restatements {e_64[region] / e_hs64[region]:.2f})")
        assert e_dev[region] <= e_64[region] + 3 * r_32, (name, region)
        # Half of Horn-Schunck's error: at the defaults everywhere.  With scales=1 a motion of 4 px is beyond what one scale
        # follows, and on scene1 the fp64 restatements themselves stand at 0.53 (visible) and 0.63 (band) - there the device is
        # held to the restatement by the two assertions above; everywhere else (fp64 ratios 0.18 ... 0.39) to the half as well.
        if not kw or e_64[region] <= 0.5 * e_hs64[region]:
            assert e_dev[region] <= 0.5 * e_hs[region], (name, region, e_dev[region], e_hs[region])
        else:
            assert (name, region) in (("scene1", "visible"), ("scene1", "band")), (name, region)


def test_identical_frames_give_exactly_zero_flow(eng):
    from artstyletransfer_amd.flow_modes import TVL1Params
    for shape, _, seed in hs.PAIRS:
        A = dev(torch.from_numpy(hs.synthetic_pair(shape, (0.0, 0.0), seed)[0]))
        assert not _bits(eng.flow_estimate(A, A.clone(), TVL1Params())).any()


def test_refusals_launch_nothing_and_leave_the_output_untouched(eng):
    from artstyletransfer_amd import engine as E
    from artstyletransfer_amd.flow_modes import TVL1Params
    h, w = 33, 47
    A, B = (dev(torch.from_numpy(a)) for a in hs.synthetic_pair((h, w), (1.5, 0.5), 3))
    floats, used = E.flow_tvl1_workspace(h, w, 0)
    assert used == 3 and floats > E.flow_workspace(h, w, 0)[0]
    work = torch.empty(floats, dtype=torch.float32, device=A.device)
    poison = float(np.float32(-1234.5))
    out = torch.full((2, h, w), poison, dtype=torch.float32, device=A.device)
    stream = E._stream(eng.device)

    def call(a=A, b=B, hh=h, ww=w, lam=L, th=TH, tau=TAU, scales=0, warps=5, iterations=50, o=out, wk=work, n=floats):
        return eng.lib.nst_flow_tvl1_estimate(eng.ctx, E._ptr(a), E._ptr(b), hh, ww, lam, th, tau, scales, warps, iterations, E._ptr(o),
                                              E._ptr(wk), n, stream)

    refused = [dict(n=floats - 1), dict(n=E.flow_workspace(h, w, 0)[0]), dict(a=None), dict(b=None), dict(o=None), dict(wk=None), dict(hh=0),
               dict(ww=0), dict(lam=0.0), dict(lam=-0.15), dict(lam=float("nan")), dict(lam=float("inf")), dict(th=0.0), dict(th=-0.3),
               dict(th=float("nan")), dict(th=float("inf")), dict(tau=0.0), dict(tau=-0.25), dict(tau=float("nan")), dict(tau=float("inf")),
               dict(lam=1e-20, th=1e-20), dict(lam=1e20, th=1e20), dict(tau=1e-20, th=1e20), dict(tau=1e20, th=1e-20),
               dict(o=A), dict(o=B), dict(wk=out), dict(wk=A), dict(warps=0), dict(iterations=0), dict(scales=-1), dict(scales=13)]
    for kw in refused:
        assert call(**kw) == E_ARG, kw
        assert (out == poison).all(), kw
    with pytest.raises(E.NstError, match="workspace"):
        E._lib.check(eng.ctx, call(n=floats - 1), "nst_flow_tvl1_estimate")
    assert call() == 0 and not (out == poison).any()
    assert np.array_equal(_bits(out), _bits(eng.flow_estimate(A, B, TVL1Params())))
    # odd counts of warps and iterations, one and two scales: the result still ends in the caller's buffer
    for kw in (dict(warps=1, iterations=1, scales=1), dict(warps=3, iterations=5, scales=2), dict(warps=2, iterations=3, scales=0)):
        out.fill_(poison)
        assert call(**kw) == 0 and not (out == poison).any(), kw
        w64, w32 = (ref.estimate(A.cpu().numpy(), B.cpu().numpy(), dt, **kw)[0] for dt in (np.float64, np.float32))
        _hold(f"tvl1 estimate {(h, w)} {kw}", out.cpu().numpy(), w64, w32)


# ================================================================================================ the driver
def test_video_driver_estimates_tvl1_flows_when_handed_a_tvl1params(vgg_weights):
    """Two 64x96 frames, the second the first moved two pixels to the right (8 pixels at the 256x384 a one-level job yields:
    the smallest size the driver's job accepts), Adam, two iterations, temporal weight 1e9.  backward_flows=TVL1Params()
    yields the bits of a run that is handed the flows StyleEngine.flow_estimate(..., TVL1Params()) gives for the same luminance
    planes and the weights flow_weights gives for the pair; backward_flows=None still yields the bits of the run handed the
    Horn-Schunck flows - and not those of the TV-L1 run."""
    from artstyletransfer_amd import config, neural_nets, video
    from artstyletransfer_amd.flow_modes import TVL1Params
    from artstyletransfer_amd.neural_nets import shared_engine
    neural_nets.set_weights(vgg_weights)
    f0 = cpu_ref.synthetic_image(64, 96, seed=1)
    f1 = np.roll(f0, 2, axis=1)
    style = cpu_ref.synthetic_image(64, 96, seed=2)
    cfg = config.Config(levels_num=1, iters_num=2, optimizer="adam", init_method="content")
    hh, ww = video.result_size(f0.shape, 1)
    assert (hh, ww) == (256, 384)

    def run(frames, *flows, **kw):
        async def go():
            return [(i, p, img) async for i, p, img in video.neural_style_transfer_video(frames, style, *flows, temporal_weight=1e9, cfg=cfg, **kw)]
        return asyncio.run(go())

    def same(a, b):
        return all(x[:2] == y[:2] and np.array_equal(x[2].view(np.int32), y[2].view(np.int32)) for x, y in zip(a, b))

    e = shared_engine(torch.device("cuda", torch.cuda.current_device()))
    p0, p1 = (e.luminance(e.resize(dev(torch.from_numpy(f)), hh, ww)).reshape(hh, ww) for f in (f0, f1))
    hwc = lambda flow: flow.permute(1, 2, 0).cpu().numpy()
    own = run([f0, f1], TVL1Params())
    assert [(i, p) for i, p, _ in own] == [(0, 50.0), (0, 100.0), (1, 50.0), (1, 100.0)]
    bwd, fwd = e.flow_estimate(p1, p0, TVL1Params()), e.flow_estimate(p0, p1, TVL1Params())
    handed = run([f0, f1], [hwc(bwd)], weights=[e.flow_weights(fwd, bwd).cpu().numpy()])
    assert same(own, handed)
    inner = bwd[:, 32:-32, 32:-32].cpu().numpy()
    report(f"video driver 256x384: TV-L1 backward flow, inner mean ({inner[0].mean():.3f}, {inner[1].mean():.3f}) px for a true (-8, 0)")
    assert abs(inner[0].mean() + 8.0) < 1.0 and abs(inner[1].mean()) < 1.0
    plain = run([f0, f1])
    b_hs, f_hs = e.flow_estimate(p1, p0), e.flow_estimate(p0, p1)
    assert same(plain, run([f0, f1], [hwc(b_hs)], [hwc(f_hs)]))
    assert not np.array_equal(_bits(b_hs), _bits(bwd)) and np.isfinite(own[-1][2]).all()
