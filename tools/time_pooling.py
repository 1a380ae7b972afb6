"""GPU: closure rate of the L=2 benchmark job (bench.build_job) under max and under average pooling
(nst_job_set_pooling), alternated three times in one process, and the per-class split of one timed closure of each
(nst_last_closure_class: 3x3 convolutions, Gram, conv1_1, everything else).
    python tools/time_pooling.py [reps=200]"""
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


def setup(mode):
    eng.set_pooling(mode)
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
        torch.cuda.synchronize()
        return [eng.last_closure_class(k)[:2] for k in range(4)]
    finally:
        eng.set_timing(0)


# the modes alternated, ROUNDS times over: a box drifts by ~1 % over a minute, so one sequential run per mode cannot tell a
# 0.5 % difference from the drift
ROUNDS = 3
runs = {m: [] for m in ("max", "avg")}
splits = {}
for r in range(ROUNDS):
    for mode in runs:
        setup(mode)
        ms = rate()
        runs[mode].append(ms)
        print(f"round {r} closure {mode:4s} {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s", flush=True)
        if r == ROUNDS - 1:
            splits[mode] = split()
for mode, v in runs.items():
    mean = sum(v) / len(v)
    ratios = [a / b for a, b in zip(runs["max"], v)]        # rate vs max of the same round
    print(f"closure {mode:4s} mean {mean:7.3f} ms/closure  {1e3 / mean:6.1f} it/s  spread over the rounds {(max(v) - min(v)) / mean:6.2%}  "
          f"rate vs max per round " + " ".join(f"{q:6.4f}x" for q in ratios) + f"  (mean {sum(ratios) / len(ratios):6.4f}x)", flush=True)
for mode, sp in splits.items():
    print(f"timed closure {mode:4s}: " + "  ".join(f"{name} {ms:7.3f} ms / {n} launches" for name, (ms, n) in zip(CLASSES, sp)), flush=True)
eng.set_pooling("max")
eng.close()
