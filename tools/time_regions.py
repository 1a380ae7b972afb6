"""GPU: closure rate of the L=2 benchmark job (bench.build_job) without guidance (R = 0) and under spatial control with
R = 1, 2, 4 regions (nst_level_set_guidance: soft vertical bands that overlap), each measured in one process, and the Gram
class of one timed closure of each (nst_last_closure_class / nst_last_closure_launches: the guided Gram partials and the
guided backward launches are Gram-class launches; a guided backward launch is one whose FLOPs are R times its map's Gram).
    python tools/time_regions.py [reps=100]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
CLASSES = ("conv3x3", "gram", "conv1_1", "other")
MAP_C = (64, 128, 256, 512, 512)          # channels of the default style maps
MAP_S = (0, 1, 2, 3, 4)


def bands(r, h, w):
    """R soft vertical bands: raised-cosine bumps that overlap their neighbours (R = 1: ones)."""
    if r == 1:
        return np.ones((1, h, w), np.float32)
    xs = (np.arange(w, dtype=np.float64) + 0.5) / w
    out = [np.clip(1.0 - np.abs(xs - (k + 0.5) / r) * r * 0.75, 0.0, 1.0) for k in range(r)]
    return np.ascontiguousarray(np.broadcast_to(np.stack(out)[:, None, :], (r, h, w)), dtype=np.float32)


def setup(r):
    eng.clear_guidance()
    for l in range(levels):
        if r == 0:
            eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))
        else:
            eng.set_guidance(l, torch.from_numpy(bands(r, *cl[l].shape[:2])).cuda())
            eng.set_targets_guided(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]), torch.from_numpy(bands(r, *sl[l].shape[:2])).cuda())


def rate():
    for _ in range(5):
        eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        eng.closure(x, cw, sw, tvw)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def halves():
    """Mean milliseconds of the forward half (Grams and loss row: the guided Gram partials live here) and of the backward half
    (the guided backward launches live here) of the closure, an event pair around each."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for _ in range(3):
        eng.closure_forward(x, cw, sw, tvw)
        eng.closure_backward(x, cw, sw, tvw)
    torch.cuda.synchronize()
    for a, b, c in ev:
        a.record(); eng.closure_forward(x, cw, sw, tvw); b.record(); eng.closure_backward(x, cw, sw, tvw); c.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b, _ in ev) / reps, sum(b.elapsed_time(c) for _, b, c in ev) / reps


def split():
    eng.set_timing(2)
    try:
        eng.closure(x, cw, sw, tvw)
        torch.cuda.synchronize()
        return [eng.last_closure_class(k) for k in range(4)]
    finally:
        eng.set_timing(0)


base = None
base_halves = None
for r in (0, 1, 2, 4):
    setup(r)
    ms = rate()
    base = base or ms
    # algorithmic work of the guided kernels: 2 N C^2 R per map for the Gram partials and as much for the backward
    work = sum(2.0 * (cl[l].shape[0] >> s) * (cl[l].shape[1] >> s) * c * c * max(r, 1) for l in range(levels) for c, s in zip(MAP_C, MAP_S))
    sp = split()
    fwd, bwd = halves()
    base_halves = base_halves or (fwd, bwd)
    print(f"R = {r}: {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s  {ms / base:5.2f}x the unguided closure;  Gram partials "
          f"{work / 1e9:7.1f} GFLOP" + (f", guided backward {work / 1e9:7.1f} GFLOP" if r else "") + ";  timed closure: " +
          "  ".join(f"{name} {t:7.3f} ms / {n} launches / {fl / 1e9:7.1f} GFLOP" for name, (t, n, fl) in zip(CLASSES, sp)) +
          f";  halves: forward {fwd:7.3f} ms (+{fwd - base_halves[0]:6.3f} over R = 0: the guided Gram partials, finish passes and fold), "
          f"backward {bwd:7.3f} ms (+{bwd - base_halves[1]:6.3f}: the guided backward launches in place of the second K sources)", flush=True)
eng.clear_guidance()
eng.close()
