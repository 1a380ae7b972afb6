"""GPU: closure rate of the L=2 benchmark job (bench.build_job) with the moment loss (nst_job_set_moments) off, with both
terms on every style map, with the "mean" term beside a centred Gram, and the centred Gram alone (what that pair is compared
with), alternated three times in one process; and the per-class kernel time and launch count of one timed closure of each
(nst_last_closure_class: the channel-sums, finish and fold kernels are class 3).
    python tools/time_moments.py [reps=200]"""
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
# (moment weight of the mean term, of the deviation term, Gram shift)
SETTINGS = {"off": (None, None, None), "both": (1e3, 1e3, None), "centred": (None, None, "mean"), "mean+centred": (1e3, None, "mean")}


def setup(setting):
    wm, ws, shift = setting
    eng.set_gram_shift(shift)
    eng.set_moments(wm, ws)
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
splits, rows, moms = {}, {}, {}
for r in range(ROUNDS):
    for name, setting in SETTINGS.items():
        setup(setting)
        ms = rate()
        runs[name].append(ms)
        print(f"round {r} closure {name:12s} {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s", flush=True)
        if r == ROUNDS - 1:
            splits[name] = split()
            _, losses = eng.closure(x, cw, sw, tvw)
            rows[name] = losses.cpu().numpy()[:-1].reshape(levels, 4)
            moms[name] = eng.moment_losses().cpu().numpy()
for name, v in runs.items():
    mean = sum(v) / len(v)
    ratios = [a / b for a, b in zip(runs["off"], v)]        # rate vs the plain closure of the same round
    print(f"closure {name:12s} mean {mean:7.3f} ms/closure  {1e3 / mean:6.1f} it/s  spread over the rounds {(max(v) - min(v)) / mean:6.2%}  "
          f"rate vs off per round " + " ".join(f"{q:6.4f}x" for q in ratios) + f"  (mean {sum(ratios) / len(ratios):6.4f}x)", flush=True)
ratios = [a / b for a, b in zip(runs["centred"], runs["mean+centred"])]
print("closure mean+centred vs centred per round " + " ".join(f"{q:6.4f}x" for q in ratios) + f"  (mean {sum(ratios) / len(ratios):6.4f}x)", flush=True)
off = splits["off"]
for name, sp in splits.items():
    print(f"timed closure {name:12s}: " + "  ".join(f"{cls} {ms:7.3f} ms / {n} launches" for cls, (ms, n) in zip(CLASSES, sp))
          + f"  | vs off: gram {sp[1][0] - off[1][0]:+6.3f} ms, other {sp[3][0] - off[3][0]:+6.3f} ms / {sp[3][1] - off[3][1]:+d} launches", flush=True)
for name, r in rows.items():
    print(f"level totals {name:12s}: " + "  ".join(f"level {l} {r[l, 0]:.4e}" for l in range(levels))
          + "  | sum(mean_i + std_i): " + "  ".join(f"{moms[name][l].sum():.3f}" for l in range(levels)), flush=True)
eng.reset_moments()
eng.reset_gram_shift()
eng.close()
