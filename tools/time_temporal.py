"""GPU: closure rate of the L=3 benchmark job (bench.build_job) with the temporal term (nst_level_set_anchor) off and on,
alternated three times in one process; the streaming-class kernel time of one timed closure of each (nst_last_closure_class 3:
the term's two kernels per level are the difference to the term-off closure) and the term's magnitude beside the level totals
for a shifted-frame example - the anchor of every level is the benchmark's start image moved 8 pixels to the right by
nst_warp_bilinear (a constant integer backward flow), the weights its valid plane - so that a weight can be picked:
gamma = share * total / tmp gives the term that share of a level total.
    python tools/time_temporal.py [reps=200]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from artstyletransfer_amd import video

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
CLASSES = ("conv3x3", "gram", "conv1_1", "other")
SETTINGS = {"off": None, "on": 1.0}
for l in range(levels):
    eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))

# the shifted-frame example: the start image as the previous result, the next frame moved 8 pixels to the right
h0, w0 = eng.level_shape(0)
flow = torch.zeros((2, h0, w0), dtype=torch.float32, device=x.device)
flow[0] = -8.0
start_hwc = torch.from_numpy(host[2]).cuda()
warped, valid = eng.warp_bilinear(start_hwc.permute(2, 0, 1).contiguous(), flow)
omega = warped.permute(1, 2, 0).contiguous()
anchors = video.level_anchors(eng, omega, levels)
weights = video.level_weights(valid, levels)
print(f"shifted-frame example: {h0}x{w0}, backward flow (-8, 0), valid plane {float(valid.mean()):.4f} ones", flush=True)


def setup(gamma):
    if gamma:
        for l in range(levels):
            eng.set_anchor(l, anchors[l], weights[l], gamma=gamma)
    else:
        eng.clear_anchor()


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
    for name, gamma in SETTINGS.items():
        setup(gamma)
        ms = rate()
        runs[name].append(ms)
        print(f"round {r} closure {name:4s} {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s", flush=True)
        if r == ROUNDS - 1:
            splits[name] = split()
            _, losses = eng.closure(x, cw, sw, tvw)
            sizes[name] = (losses.cpu().numpy()[:-1].reshape(levels, 4), eng.temporal_losses().cpu().numpy())
for name, v in runs.items():
    mean = sum(v) / len(v)
    ratios = [a / b for a, b in zip(runs["off"], v)]        # rate vs the term-off closure of the same round
    print(f"closure {name:4s} mean {mean:7.3f} ms/closure  {1e3 / mean:6.1f} it/s  spread over the rounds {(max(v) - min(v)) / mean:6.2%}  "
          f"rate vs off per round " + " ".join(f"{q:6.4f}x" for q in ratios) + f"  (mean {sum(ratios) / len(ratios):6.4f}x)", flush=True)
off_other = splits["off"][3]
for name, sp in splits.items():
    print(f"timed closure {name:4s}: " + "  ".join(f"{cls} {ms:7.3f} ms / {n} launches" for cls, (ms, n) in zip(CLASSES, sp))
          + f"  | the term's kernels: {sp[3][0] - off_other[0]:6.3f} ms / {sp[3][1] - off_other[1]} launches", flush=True)
rows, tmp = sizes["on"]
for l in range(levels):
    h, w = eng.level_shape(l)
    off = sizes["off"][0][l]
    print(f"magnitudes level {l} ({h}x{w}): total without the term {off[0]:.4e} = {cw:g} x content {off[1]:.4e} + {sw:g} x style {off[2]:.4e} "
          f"+ {tvw:g} x tv {off[3]:.4e};  tmp {tmp[l]:.4e}  (gamma for 10 % of the level total: {0.1 * off[0] / tmp[l]:.3e})", flush=True)
bytes_moved = sum(4 * ((3 + 3 + 1) * 2 + 3 + 3) * eng.level_shape(l)[0] * eng.level_shape(l)[1] for l in range(levels))
print(f"bytes of the two passes over the {levels} levels (y, a, c read twice, the gradient read and written): {bytes_moved / 1e9:.3f} GB", flush=True)
eng.clear_anchor()
eng.close()
