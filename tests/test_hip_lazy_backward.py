"""GPU: the closure in two halves (nst_closure_forward / nst_closure_backward) and the L-BFGS driver that uses them
(nst_opt_set_lazy_backward): a trial point whose gradient can only be read if the point is taken is evaluated by its forward
half, and the backward half runs only when it is taken.  Everything the halves and the lazy driver return must be bitwise
what the whole closure and the eager driver return."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels, setup

pytestmark = pytest.mark.gpu

FIELDS = ("closures", "total_closures", "accepted", "loss", "lr", "t", "history")
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _start(c0, seed=9):
    """A start image away from the content image: every loss term and its gradient is non-zero."""
    h, w = c0.shape[:2]
    return (0.6 * c0 + 0.4 * cpu_ref.synthetic_image(h, w, seed=seed)).astype(np.float32)


def _rgb_job(e, h, w, seed=0):
    c, s = levels(h, w, 2, 1 + 2 * seed), levels(h, w, 2, 2 + 2 * seed)
    setup(e, c, s)
    return dev(cpu_ref.prepare_img(_start(c[0])))


def _luminance_job(e, h, w):
    from artstyletransfer_amd import host_image
    c, s = levels(h, w, 2, 5), levels(h, w, 2, 6)
    e.configure(2, h, w)
    e.set_color("luminance")
    alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
    for i in range(2):
        e.set_targets(i, dev(torch.from_numpy(host_image.luminance(c[i]))),
                      dev(torch.from_numpy(host_image.luminance(s[i], alpha, beta))))
    return dev(torch.from_numpy(host_image.luminance(_start(c[0]))).reshape(1, 1, h, w))


def _halves_equal_the_whole(e, x):
    """nst_closure, then the halves into fresh buffers, then nst_closure again: three times the same bits."""
    g0, l0 = e.closure(x, CW, SW, TVW)
    l1 = e.closure_forward(x, CW, SW, TVW)
    g1 = torch.full_like(g0, SENTINEL)
    e.closure_backward(x, CW, SW, TVW, grad=g1)
    g2, l2 = e.closure(x, CW, SW, TVW)
    torch.cuda.synchronize()
    assert np.isfinite(l0.cpu().numpy()).all() and float(g0.abs().max()) > 0
    assert np.array_equal(_bits(l0), _bits(l1)), "loss row of the forward half"
    assert np.array_equal(_bits(g0), _bits(g1)), "gradient of the backward half"
    assert np.array_equal(_bits(l0), _bits(l2)) and np.array_equal(_bits(g0), _bits(g2)), "the halves left state behind"


# name -> (h, w, pooling, colour, taps (content, style, use_relu) or None); all with levels_num = 2: the batched schedule
JOBS = {
    "64x96": (64, 96, "max", "rgb", None),
    "100x152_ragged": (100, 152, "max", "rgb", None),          # odd coarse sizes (50x76 -> 25x38 ...), ragged pool edges
    "avg_pool": (64, 96, "avg", "rgb", None),
    "luminance": (64, 96, "max", "luminance", None),
    "prerelu_top": (64, 96, "max", "rgb", (4, [0, 1, 2, 3, 5], False)),
    "content_is_a_style_map": (64, 96, "max", "rgb", (2, [2, 3], True)),
}


@pytest.mark.parametrize("job", sorted(JOBS))
def test_halves_equal_the_whole_bitwise(eng, job):
    h, w, pooling, colour, taps = JOBS[job]
    try:
        eng.configure(2, h, w)
        if taps:
            eng.set_taps(*taps)
        eng.set_pooling(pooling)
        x = _luminance_job(eng, h, w) if colour == "luminance" else _rgb_job(eng, h, w)
        _halves_equal_the_whole(eng, x)
    finally:
        eng.reset_taps()
        eng.reset_color()
        eng.reset_pooling()


def test_halves_equal_the_whole_under_level_split(vgg_weights):
    """nst_options.level_split: the two chains of the closure on two streams, in both halves."""
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, level_split=True)
    try:
        _halves_equal_the_whole(e, _rgb_job(e, 64, 96))
    finally:
        e.close()


def test_forward_half_is_unavailable_off_the_batched_schedule(vgg_weights):
    """The per-level walker has no halves: a distinct status before anything is launched, and the whole closure works."""
    from artstyletransfer_amd import _lib
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0, batched=False)
    try:
        x = _rgb_job(e, 64, 96)
        losses = torch.full((9,), SENTINEL, device=x.device)
        rc = e.lib.nst_closure_forward(e.ctx, C.c_void_p(x.data_ptr()), CW, SW, TVW, 0xFFFFFFFF, C.c_void_p(losses.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.NST_E_UNAVAILABLE
        torch.cuda.synchronize()
        assert bool((losses == SENTINEL).all())
        e.closure(x, CW, SW, TVW)
    finally:
        e.close()


def test_stale_backward_is_refused(eng):
    """No forward, nst_level_set_targets in between, nst_closure in between, another x pointer, other weights: NST_E_STATE
    each time, the gradient buffer untouched, and the context goes on working."""
    from artstyletransfer_amd import _lib
    c, s = levels(64, 96, 2, 1), levels(64, 96, 2, 2)
    setup(eng, c, s)
    x = dev(cpu_ref.prepare_img(_start(c[0])))
    x2 = x.clone()
    g_ref, l_ref = eng.closure(x, CW, SW, TVW)
    grad = torch.full_like(g_ref, SENTINEL)

    def backward(xx=x, cw=CW):
        return eng.lib.nst_closure_backward(eng.ctx, C.c_void_p(xx.data_ptr()), cw, SW, TVW, 0xFFFFFFFF, C.c_void_p(grad.data_ptr()),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def refused(rc):
        torch.cuda.synchronize()
        assert rc == _lib.NST_E_STATE, rc
        assert b"nst_closure_backward" in eng.lib.nst_last_error(eng.ctx)
        assert bool((grad == SENTINEL).all())

    refused(backward())                                                      # the last use was a whole closure: no forward
    eng.closure_forward(x, CW, SW, TVW)
    eng.set_targets(1, dev(cpu_ref.prepare_img(c[1])), dev(cpu_ref.prepare_img(s[1])))
    refused(backward())
    eng.closure_forward(x, CW, SW, TVW)
    eng.closure(x, CW, SW, TVW)
    refused(backward())
    eng.closure_forward(x, CW, SW, TVW)
    refused(backward(xx=x2))
    refused(backward(cw=2.0 * CW))
    # ... and the forward made before the two refusals is still good, once
    assert backward() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(grad), _bits(g_ref))
    grad.fill_(SENTINEL)
    refused(backward())
    g, l = eng.closure(x, CW, SW, TVW)
    assert np.array_equal(_bits(g), _bits(g_ref)) and np.array_equal(_bits(l), _bits(l_ref))


# ---- the driver ---------------------------------------------------------------------------------------------------------
def _info_tuple(info):
    f32 = lambda v: int(np.asarray(v, dtype=np.float32).view(np.uint32))      # noqa: E731  (NaN and -0 compare exactly)
    return tuple(f32(getattr(info, f)) if f in ("loss", "lr", "t") else int(getattr(info, f)) for f in FIELDS)


def _run(eng, x0, name, max_eval, steps, lazy, reuse, lr=10.0):
    from artstyletransfer_amd.engine import PixelOptimizer
    opt = PixelOptimizer(eng, name, lr, max_eval)
    try:
        opt.set_lazy_backward(lazy)
        opt.set_closure_reuse(reuse)
        x = x0.clone()
        out = []
        for _ in range(steps):
            info, rows = opt.step(x, CW, SW, TVW)
            out.append((_info_tuple(info), rows.view(np.uint32).copy(), _bits(x)))
        return out, opt.closure_stats(), opt.backward_stats()
    finally:
        opt.close()


def _driver_job(eng):
    """64x96, levels_num = 2, seed 0 of test_hip_closure_reuse's job (content images levels(64, 96, 2, 1), style images
    levels(64, 96, 2, 2)), started at the content image, weights (CW, SW, TVW) = (1e3, 4e5, 1e2)."""
    c, s = levels(64, 96, 2, 1), levels(64, 96, 2, 2)
    setup(eng, c, s)
    return dev(cpu_ref.prepare_img(c[0]))


STEPS = 8


@pytest.mark.parametrize("reuse", (True, False), ids=("reuse_on", "reuse_off"))
@pytest.mark.parametrize("name,max_eval,lr", (("lbfgs", 1, 10.0), ("lbfgs", 2, 10.0), ("lbfgs", 2, 100.0), ("lbfgs", 3, 100.0),
                                              ("lbfgs", 26, 10.0), ("adam", 1, 10.0)),
                         ids=("lbfgs_1", "lbfgs_2", "lbfgs_2_lr100", "lbfgs_3_lr100", "lbfgs_26", "adam"))
def test_driver_returns_the_same_with_lazy_backward(eng, name, max_eval, lr, reuse):
    """Lazy on against lazy off over STEPS = 8 optimiser steps: x after every step, all loss rows, every nst_step_info field
    and the closure counts, bitwise.

    The job, seed and STEPS were chosen on the CPU with oracle/cpu_ref.py (LbfgsState(max_eval=1) on closure_eval of this
    job): its steps 1 and 2 are accepted and steps 3 .. 12 rejected, so 8 steps of the max_eval 1 run hold accepted and
    rejected trials both - asserted below on the lazy-off run.  What is skipped is counted:
    skipped backward passes == evaluated trial closures - accepted steps at max_eval 1, 0 with the switch off, 0 under Adam.

    max_eval 2 and 3 (max_ls 1 and 2) put the lazy evaluation INSIDE strong_wolfe's loops: a step whose line search uses
    all of max_ls + 1 evaluations (max_eval + 1 closures) ends on a forward half made in the bracket or the zoom loop.  The
    max_eval 26 run of this job never gets there.  Chosen with the same CPU run: at lr 10 and max_eval 2, 11 of 12 steps
    use up the line search and every one of them takes its last point; at lr 100 (max_eval 2 and 3) every step uses it up,
    the first takes its last point and all later ones drop it.  So the lr 10 case must show taken lazy points and the
    lr 100 cases taken and dropped ones."""
    x0 = _driver_job(eng)
    steps = STEPS
    off, stats_off, bw_off = _run(eng, x0, name, max_eval, steps, False, reuse, lr)
    on, stats_on, bw_on = _run(eng, x0, name, max_eval, steps, True, reuse, lr)
    for k, (a, b) in enumerate(zip(on, off)):
        assert a[0] == b[0], (k, a[0], b[0])
        assert a[1].shape == b[1].shape and np.array_equal(a[1], b[1]), k
        assert np.array_equal(a[2], b[2]), k
    assert stats_on == stats_off
    assert bw_off == (0, 0)
    accepted = sum(i[0][2] for i in off)
    trials = sum(i[0][0] - 1 for i in off)             # every closure of a step after its first
    print(f"{name} max_eval {max_eval} lr {lr} reuse {reuse}: {steps} steps, {accepted} accepted, {trials} trial closures, "
          f"closures (evaluated, served) {stats_on}, (forward-only, skipped) {bw_on}")
    if name == "adam":
        assert bw_on == (0, 0)
    elif max_eval == 1:
        assert 1 <= accepted < STEPS and trials == STEPS, (accepted, trials)
        assert bw_on == (trials, trials - accepted)
    else:
        # only the evaluation that exhausts the line search (max_ls = max_eval - 1 iterations after its first point) is lazy
        assert bw_on[0] == sum(1 for i in off if i[0][0] == max_eval + 1) and bw_on[1] <= bw_on[0]
        if max_eval in (2, 3):
            assert bw_on[0] - bw_on[1] > 0, bw_on                 # lazy points taken: their backward half ran
            if lr == 100.0:
                assert bw_on[1] > 0, bw_on                        # ... and lazy points dropped


def test_env_switch_turns_lazy_backward_off(eng, monkeypatch):
    from artstyletransfer_amd.engine import PixelOptimizer
    x = _driver_job(eng)
    monkeypatch.setenv("NST_LAZY_BACKWARD", "0")
    opt = PixelOptimizer(eng, "lbfgs", 10.0, 1)
    try:
        for _ in range(3):
            opt.step(x, CW, SW, TVW)
        assert opt.backward_stats() == (0, 0)
    finally:
        opt.close()


def test_timing_totals_of_the_halves_are_those_of_the_whole(eng):
    """Timing mode 2: a forward half and its backward half are ONE closure with the 24 conv launches, the conv1_1 and Gram
    launches and the matrix-pipe FLOPs of one nst_closure."""
    c, s = levels(64, 96, 2, 1), levels(64, 96, 2, 2)
    setup(eng, c, s)
    x = dev(cpu_ref.prepare_img(_start(c[0])))
    eng.set_timing(2)
    try:
        def totals(run):
            eng.timing_totals(-1, reset=True)
            run()
            torch.cuda.synchronize()
            mf = [eng.timing_mfma_flops(k) for k in range(3)]
            per = [eng.timing_totals(k)[1:] for k in range(3)]           # (launches, flops) of conv3x3, Gram, conv1_1
            return eng.timing_totals(-1)[1], per, mf

        def halves():
            eng.closure_forward(x, CW, SW, TVW)
            eng.closure_backward(x, CW, SW, TVW)

        def forward_only():
            eng.closure_forward(x, CW, SW, TVW)

        whole = totals(lambda: eng.closure(x, CW, SW, TVW))
        assert whole[0] == 1 and whole[1][0][0] == 24
        assert totals(halves) == whole
        n, per, mf = totals(forward_only)
        assert n == 1 and per[0][0] == 12
        # ... whose FLOPs are those of what it launched: the forward share, and with a LATER backward half the whole closure's
        assert all(0 < f < w for f, w in zip(mf, whole[2])), (mf, whole[2])
        eng.closure_backward(x, CW, SW, TVW)
        torch.cuda.synchronize()
        assert [eng.timing_mfma_flops(k) for k in range(3)] == whole[2]
        assert [eng.timing_totals(k)[1:] for k in range(3)] == whole[1] and eng.timing_totals(-1)[1] == 1
    finally:
        eng.timing_totals(-1, reset=True)
        eng.set_timing(0)
