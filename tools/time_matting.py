"""GPU: closure rate of the L=3 benchmark job (bench.build_job) with the matting term (nst_job_set_matting) off and on,
alternated three times in one process; the streaming-class kernel time of one timed closure of each (nst_last_closure_class 3:
the term's two kernels per level are the difference to the term-off closure) and the term's magnitude beside the level totals
(mat and the loss row at the benchmark's start image), so that a weight can be picked: gamma = share * total / mat gives the term
that share of a level total.
    python tools/time_matting.py [reps=200]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
CLASSES = ("conv3x3", "gram", "conv1_1", "other")
SETTINGS = {"off": None, "on": (1.0, 1e-7)}


def setup(setting):
    if setting:
        eng.set_matting(*setting)
    else:
        eng.reset_matting()
    for l in range(levels):
        eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))


def rate():
    for _ in range(10):
        eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        eng.closure(x, cw, sw, tvw)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def split():
    """Per-class milliseconds and launch counts of one closure with an event pair around every launch (timing mode 2)."""
    eng.set_timing(2)
    try:
        eng.closure(x, cw, sw, tvw)
        eng.closure(x, cw, sw, tvw)
        torch.cuda.synchronize()
        return [eng.last_closure_class(k)[:2] for k in range(4)]
    finally:
        eng.set_timing(0)


# the settings alternated, ROUNDS times over: a box drifts by ~1 % over a minute, so one sequential run per setting cannot tell
# a 0.5 % difference from the drift
ROUNDS = 3
runs = {m: [] for m in SETTINGS}
splits, sizes = {}, {}
for r in range(ROUNDS):
    for name, setting in SETTINGS.items():
        setup(setting)
        ms = rate()
        runs[name].append(ms)
        print(f"round {r} closure {name:4s} {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s", flush=True)
        if r == ROUNDS - 1:
            splits[name] = split()
            _, losses = eng.closure(x, cw, sw, tvw)
            sizes[name] = (losses.cpu().numpy()[:-1].reshape(levels, 4), eng.matting_losses().cpu().numpy())
for name, v in runs.items():
    mean = sum(v) / len(v)
    ratios = [a / b for a, b in zip(runs["off"], v)]        # rate vs the term-off closure of the same round
    print(f"closure {name:4s} mean {mean:7.3f} ms/closure  {1e3 / mean:6.1f} it/s  spread over the rounds {(max(v) - min(v)) / mean:6.2%}  "
          f"rate vs off per round " + " ".join(f"{q:6.4f}x" for q in ratios) + f"  (mean {sum(ratios) / len(ratios):6.4f}x)", flush=True)
off_other = splits["off"][3]
for name, sp in splits.items():
    print(f"timed closure {name:4s}: " + "  ".join(f"{cls} {ms:7.3f} ms / {n} launches" for cls, (ms, n) in zip(CLASSES, sp))
          + f"  | the term's kernels: {sp[3][0] - off_other[0]:6.3f} ms / {sp[3][1] - off_other[1]} launches", flush=True)
rows, mat = sizes["on"]
for l in range(levels):
    h, w = eng.level_shape(l)
    print(f"magnitudes level {l} ({h}x{w}): total without the term {sizes['off'][0][l, 0]:.4e}  mat {mat[l]:.4e}  "
          f"(gamma for 10 % of the level total: {0.1 * sizes['off'][0][l, 0] / mat[l]:.3e})", flush=True)
eng.reset_matting()
eng.close()
