"""GPU: closure rate of the L=2 benchmark job (bench.build_job) in the three colour modes of neural_style_transfer's
preserve_color - RGB (None), luminance (nst_job_set_color: one plane u = 255 Y through the pyramid, conv1_1, TV and the
optimiser) and histogram (the RGB closure on recoloured style targets) - and the cost of an L-BFGS step with a full
100-pair history in RGB and in luminance (the line search of older torch builds, max_eval = 26, so that steps are
accepted and the history fills, as tools/time_lbfgs_history.py does).
    python tools/time_color.py [reps=200] [closures]     ("closures": the closure rates only, e.g. under rocprofv3)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from artstyletransfer_amd import device_image
from artstyletransfer_amd.engine import PixelOptimizer

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
init = torch.from_numpy(host[2]).cuda()
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight


def setup(mode):
    eng.set_color("luminance" if mode == "luminance" else "rgb")
    if mode == "luminance":
        alpha, beta = device_image.luminance_params(eng, cl[0], sl[0])
        for l in range(levels):
            eng.set_targets(l, eng.luminance(cl[l]), eng.luminance(sl[l], alpha, beta))
        return eng.luminance(init)
    styles = device_image.recolor_histogram(eng, cl[0], sl) if mode == "histogram" else sl
    for l in range(levels):
        eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(styles[l]))
    return eng.prepare_img(init)


def rate(x):
    for _ in range(10):
        eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        eng.closure(x, cw, sw, tvw)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


# the modes alternated, ROUNDS times over: a box drifts by ~1 % over a minute, so one sequential run per mode cannot tell a
# 0.5 % difference from the drift
ROUNDS = 3
runs = {m: [] for m in ("rgb", "luminance", "histogram")}
for r in range(ROUNDS):
    for mode in runs:
        ms = rate(setup(mode))
        runs[mode].append(ms)
        print(f"round {r} closure {mode:10s} {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s", flush=True)
closure_ms = {m: sum(v) / len(v) for m, v in runs.items()}
for mode, v in runs.items():
    ratios = [a / b for a, b in zip(runs["rgb"], v)]        # rate vs RGB of the same round
    print(f"closure {mode:10s} mean {closure_ms[mode]:7.3f} ms/closure  {1e3 / closure_ms[mode]:6.1f} it/s  rate vs RGB per round "
          + " ".join(f"{q:6.4f}x" for q in ratios) + f"  (mean {sum(ratios) / len(ratios):6.4f}x)", flush=True)

for mode in (("rgb", "luminance") if "closures" not in sys.argv[2:] else ()):
    x = setup(mode).clone()
    opt = PixelOptimizer(eng, "lbfgs", 1.0, 26)
    for _ in range(300):
        opt.step(x, cw, sw, tvw, want_losses=False)
        if opt.history()[0] >= 100:
            break
    pairs = opt.history()[0]
    torch.cuda.synchronize(); t0 = time.perf_counter(); ncl = 0
    for _ in range(10):
        info, _ = opt.step(x, cw, sw, tvw, want_losses=False)
        ncl += info.closures
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) * 1e3 / 10
    # non-closure: the step time less its closures at the mean closure time measured above (not in this loop)
    print(f"lbfgs step {mode:10s} history {pairs:3d} pairs: {dt:7.2f} ms/step, {ncl / 10:4.1f} closures/step, "
          f"non-closure {dt - ncl / 10 * closure_ms[mode]:6.2f} ms/step", flush=True)
    opt.close()
eng.close()
