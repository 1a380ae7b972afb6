"""GPU: L-BFGS closure reuse (nst_opt_set_closure_reuse).  When a step starts at bitwise the image the previous step left,
its first closure is served from what the optimiser remembers instead of evaluated.  Every test drives the same job with
two optimisers, reuse on and reuse off, and requires every StepInfo field, every loss row and x after every step to be
bitwise equal; the served / evaluated counts say how often the reuse applied."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from hip_helpers import CW, SW, TVW, dev, levels, setup

pytestmark = pytest.mark.gpu

FIELDS = ("closures", "total_closures", "accepted", "loss", "lr", "t", "history")


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def _info_tuple(info):
    # floats as their bit patterns: NaN and -0 compare exactly
    return tuple(int(_bits(getattr(info, f))) if f in ("loss", "lr", "t") else int(getattr(info, f)) for f in FIELDS)


class Pair:
    """The same job under two optimisers on one engine: reuse on and reuse off, each with its own image."""

    def __init__(self, eng, x0, name="lbfgs", max_eval=1):
        from artstyletransfer_amd.engine import PixelOptimizer
        self.eng = eng
        self.opts = [PixelOptimizer(eng, name, 10.0, max_eval), PixelOptimizer(eng, name, 10.0, max_eval)]
        self.opts[0].set_closure_reuse(True)
        self.opts[1].set_closure_reuse(False)
        self.xs = [x0.clone(), x0.clone()]
        self.steps = 0
        self.closures = 0
        self.moved = []

    def step(self, cw=CW, sw=SW, tvw=TVW):
        got = []
        for opt, x in zip(self.opts, self.xs):
            info, rows = opt.step(x, cw, sw, tvw)
            got.append((_info_tuple(info), rows))
        (i_on, r_on), (i_off, r_off) = got
        assert i_on == i_off, (self.steps, i_on, i_off)
        assert r_on.shape == r_off.shape and np.array_equal(_bits(r_on), _bits(r_off)), self.steps
        assert torch.equal(self.xs[0].view(torch.int32), self.xs[1].view(torch.int32)), self.steps
        self.steps += 1
        self.closures = i_on[1]
        self.moved.append(bool(i_on[2]))
        return i_on, r_on

    def run(self, closures, **w):
        while self.closures < closures:
            self.step(**w)

    def stats(self):
        (ev_on, sv_on), (ev_off, sv_off) = (o.closure_stats() for o in self.opts)
        assert ev_on + sv_on == ev_off + sv_off == self.closures
        assert sv_off == 0
        return ev_on, sv_on

    def close(self):
        for o in self.opts:
            o.close()


def _job(eng, seed=0, nlev=2, h=128, w=192):
    c, s = levels(h, w, nlev, 1 + 2 * seed), levels(h, w, nlev, 2 + 2 * seed)
    setup(eng, c, s)
    return c, s, dev(cpu_ref.prepare_img(c[0]))


def test_lbfgs_max_eval_1_every_later_step_is_served(eng):
    """max_eval 1 (the reference's constructor arguments): a step either rejects its one trial (x stays: memo A) or accepts
    it, and then the trial's closure is the last one made (memo B).  So every step after the first is served."""
    _, _, x0 = _job(eng)
    p = Pair(eng, x0)
    try:
        p.run(60)
        ev, sv = p.stats()
        print(f"max_eval 1: {p.steps} steps, {sum(p.moved)} accepted, evaluated {ev}, served {sv}")
        assert sv == p.steps - 1
    finally:
        p.close()


def test_lbfgs_line_search_is_served(eng):
    """max_eval 26: the accepted point is usually the last point the line search evaluated."""
    _, _, x0 = _job(eng)
    p = Pair(eng, x0, max_eval=26)
    try:
        p.run(40)
        ev, sv = p.stats()
        print(f"max_eval 26: {p.steps} steps, {sum(p.moved)} accepted, evaluated {ev}, served {sv}")
        assert sv > 0
    finally:
        p.close()


def test_adam_is_never_served(eng):
    _, _, x0 = _job(eng)
    p = Pair(eng, x0, name="adam")
    try:
        p.run(12)
        assert p.stats()[1] == 0
    finally:
        p.close()


def test_luminance_and_other_taps(eng):
    """Luminance mode (one plane) with non-default taps: the same equality, and served closures."""
    from artstyletransfer_amd import host_image
    c, s = levels(128, 192, 2, 5), levels(128, 192, 2, 6)
    eng.configure(2, 128, 192)
    try:
        eng.set_color("luminance")
        eng.set_taps(2, [0, 2, 3])
        alpha, beta = host_image.luminance_params(host_image.color_stats(c[0]), host_image.color_stats(s[0]))
        for i in range(2):
            eng.set_targets(i, dev(torch.from_numpy(host_image.luminance(c[i]))),
                            dev(torch.from_numpy(host_image.luminance(s[i], alpha, beta))))
        x0 = dev(torch.from_numpy(host_image.luminance(c[0])).reshape(1, 1, 128, 192))
        p = Pair(eng, x0)
        try:
            p.run(30)
            ev, sv = p.stats()
            print(f"luminance, taps (2, [0, 2, 3]): {p.steps} steps, evaluated {ev}, served {sv}")
            assert sv > 0
        finally:
            p.close()
    finally:
        eng.reset_taps()
        eng.reset_color()


def test_changes_between_steps_force_an_evaluation(eng):
    """Between two steps, on both runs: x moved by one ulp, other targets, another content weight, other taps (which need
    targets again), and a set_taps call that fails (the context stays as it was, but the call still counts as a change).
    Each time the next step evaluates its first closure, and the runs still match."""
    c, s, x0 = _job(eng)
    p = Pair(eng, x0)
    cw = CW

    def served():
        return p.opts[0].closure_stats()[1]

    def settle():
        # two steps with nothing changed: the second one is served again
        p.step(cw=cw)
        before = served()
        p.step(cw=cw)
        assert served() == before + 1

    def bump_one_ulp():
        for x in p.xs:
            flat = x.view(-1).view(torch.int32)
            flat[1234] += 1

    def other_targets():
        c2, s2 = levels(128, 192, 2, 11), levels(128, 192, 2, 12)
        for i in range(2):
            eng.set_targets(i, dev(cpu_ref.prepare_img(c2[i])), dev(cpu_ref.prepare_img(s2[i])))

    def other_cw():
        nonlocal cw
        cw = 2.0 * CW

    def other_taps():
        eng.set_taps(3, [0, 1, 2])
        for i in range(2):
            eng.set_targets(i, dev(cpu_ref.prepare_img(c[i])), dev(cpu_ref.prepare_img(s[i])))

    def failed_set_taps():
        assert eng.lib.nst_job_set_taps(eng.ctx, 3, 0, 1) != 0          # an empty style set: refused, nothing changed

    try:
        settle()
        for change in (bump_one_ulp, other_targets, other_cw, other_taps, failed_set_taps):
            change()
            before = served()
            p.step(cw=cw)
            assert served() == before, change.__name__
            settle()
        p.stats()
    finally:
        p.close()
        eng.reset_taps()


def test_rejected_step_reevaluates_bitwise_without_reuse(eng):
    """The premise of the reuse, with reuse off: the first closure after a rejected step gives bitwise its predecessor's
    row (the first row of the rejected step)."""
    from artstyletransfer_amd.engine import PixelOptimizer
    _, _, x = _job(eng)
    opt = PixelOptimizer(eng, "lbfgs", 10.0, 1)
    try:
        opt.set_closure_reuse(False)
        prev = None
        checked = 0
        for _ in range(30):
            info, rows = opt.step(x, CW, SW, TVW)
            if prev is not None and not prev[0].accepted:
                assert np.array_equal(_bits(rows[0]), _bits(prev[1][0]))
                checked += 1
            prev = (info, rows)
        assert checked > 0
        assert opt.closure_stats()[1] == 0
    finally:
        opt.close()


def test_bench_job_20_steps(vgg_weights):
    """The job bench.py measures (L = 2, built as bench.build_job builds it), 20 steps."""
    import bench
    e, x, cfg, _ = bench.build_job(3, 0, 0)
    try:
        p = Pair(e, x)
        try:
            for _ in range(20):
                p.step(cw=cfg.content_weight, sw=cfg.style_weight, tvw=cfg.tv_weight)
            ev, sv = p.stats()
            print(f"bench job: 20 steps, {sum(p.moved)} accepted, evaluated {ev}, served {sv}")
            assert sv == 19
        finally:
            p.close()
    finally:
        e.close()
