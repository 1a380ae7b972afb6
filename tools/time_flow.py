"""GPU: the time of one optical flow (StyleEngine.flow_estimate, multi-scale Horn-Schunck with warping at the default
parameters) at the benchmark job's top-level size, 1024x1536, and at 512x768, beside the estimate from bytes; and each
stage's share, from the stage entry points run scale by scale as the driver runs them (every one of these calls ends in a
device synchronise, so a host clock around it measures the kernels plus one synchronise; the sweeps are timed `iterations`
at a call, as the driver launches them).  The frame pair is a synthetic image and itself moved by (3, 1) pixels.
    python tools/time_flow.py [reps=5] [out=profiles/r17_flow.txt]
The figures replace the section between the two marker lines of `out` (the rest of the file is kept).
    python tools/time_flow.py [reps=5] [out=profiles/r18_flow_tvl1.txt] tvl1
times TV-L1 instead (flow_modes.TVL1Params at the defaults; an iteration moves fifteen planes in one launch), beside
Horn-Schunck in the same run, and the iterations of the top scale from their stage entry point."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from artstyletransfer_amd import synthetic
from artstyletransfer_amd.engine import StyleEngine, flow_workspace
from artstyletransfer_amd.flow_modes import FlowParams

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
TVL1 = len(sys.argv) > 3 and sys.argv[3] == "tvl1"
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                            "r18_flow_tvl1.txt" if TVL1 else "r17_flow.txt")
BEGIN, END = "== timing (tools/time_flow.py) ==", "== end of timing =="
HBM = 6.3e12          # achievable bytes per second of the MI355X's HBM: the yardstick of the estimate from bytes
P = FlowParams()
eng = StyleEngine(synthetic.vgg19_weights(), 0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def clock(f, n=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n, r


def time_tvl1(h, w, planes):
    """One TV-L1 flow beside one Horn-Schunck flow, and the iterations of the top scale."""
    from artstyletransfer_amd.engine import flow_tvl1_workspace
    from artstyletransfer_amd.flow_modes import TVL1Params
    T = TVL1Params()
    floats, scales = flow_tvl1_workspace(h, w, T.scales)
    sizes = [(h, w)]
    for _ in range(1, scales):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    px = sum(a * b for a, b in sizes)
    it_bytes = 4 * 15 * px * T.warps * T.iterations
    launches = 2 * (scales - 1) + 1 + scales + scales * T.warps * (1 + T.iterations) + (scales - 1)
    say(f"{h}x{w} TV-L1: {scales} scales, workspace {4 * floats / 1e6:.1f} MB; {T.warps * T.iterations} iterations per scale, {launches} launches; "
        f"bytes of the iterations {it_bytes / 1e9:.2f} GB = {1e3 * it_bytes / HBM:.2f} ms at {HBM / 1e12:.1f} TB/s (the fifteen planes of the top "
        f"scale are {4 * 15 * h * w / 1e6:.0f} MB: they fit the 256 MiB Infinity Cache)")
    for name, par in (("Horn-Schunck", None), ("TV-L1", T)):
        clock(lambda: eng.flow_estimate(planes[0], planes[1], par), 2)                     # warm-up
        runs = [clock(lambda: eng.flow_estimate(planes[0], planes[1], par))[0] for _ in range(reps)]
        flow = eng.flow_estimate(planes[0], planes[1], par)
        inner = flow[:, h // 8: -h // 8, w // 8: -w // 8]
        say(f"{h}x{w} {name}: one flow {1e3 * np.mean(runs):.2f} ms (mean of {reps}; min {1e3 * min(runs):.2f}, max {1e3 * max(runs):.2f}); "
            f"inner mean flow ({float(inner[0].mean()):.3f}, {float(inner[1].mean()):.3f}) px for a true (3, 1)")
    f = eng.flow_estimate(planes[0], planes[1], T)
    ix, iy, rho = eng.flow_linearize(planes[0], planes[1], f)
    dual = torch.zeros((4, h, w), dtype=torch.float32, device="cuda")
    eng.flow_tvl1_iterations(ix, iy, rho, f, dual, T.lambda_, T.theta, T.tau, T.iterations)
    dt, _ = clock(lambda: eng.flow_tvl1_iterations(ix, iy, rho, f, dual, T.lambda_, T.theta, T.tau, T.iterations), reps)
    say(f"{h}x{w} TV-L1: a top-scale iteration {1e6 * dt / T.iterations:.1f} us ({T.iterations} at a call, one synchronise) = "
        f"{4 * 15 * h * w / (dt / T.iterations) / 1e12:.2f} TB/s over its fifteen planes")
    small = [torch.zeros(k + sizes[-1], dtype=torch.float32, device="cuda") for k in ((), (), (), (2,), (4,))]
    eng.flow_tvl1_iterations(*small, T.lambda_, T.theta, T.tau, T.iterations)
    dt, _ = clock(lambda: eng.flow_tvl1_iterations(*small, T.lambda_, T.theta, T.tau, T.iterations), reps)
    say(f"{h}x{w} TV-L1: an iteration of the coarsest scale {sizes[-1]} {1e6 * dt / T.iterations:.1f} us: what a launch costs")


for h, w in ((1024, 1536), (512, 768)):
    img = synthetic.image(h, w, seed=1)
    planes = [eng.luminance(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()).reshape(h, w)
              for a in (img, np.roll(img, (1, 3), axis=(0, 1)))]
    if TVL1:
        time_tvl1(h, w, planes)
        continue
    floats, scales = flow_workspace(h, w, P.scales)
    sizes = [(h, w)]
    for _ in range(1, scales):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    # the estimate from bytes, written down before measuring: a sweep moves 7 planes (u, v, Ix, Iy, rho in, u', v' out), a
    # linearisation 7 (from, to, u, v in; Ix, Iy, rho out; the taps of `to` come from cache), at every scale
    px = sum(a * b for a, b in sizes)
    sweep_bytes = 4 * 7 * px * P.warps * P.iterations
    lin_bytes = 4 * 7 * px * P.warps
    say(f"{h}x{w}: {scales} scales, workspace {4 * floats / 1e6:.1f} MB; {P.warps * P.iterations} sweeps and {P.warps} linearisations per scale; "
        f"bytes: sweeps {sweep_bytes / 1e9:.2f} GB + linearisations {lin_bytes / 1e9:.3f} GB = {1e3 * (sweep_bytes + lin_bytes) / HBM:.2f} ms at "
        f"{HBM / 1e12:.1f} TB/s (the seven planes of the top scale are {4 * 7 * h * w / 1e6:.0f} MB: they fit the 256 MiB Infinity Cache)")
    clock(lambda: eng.flow_estimate(planes[0], planes[1]), 2)                     # warm-up
    t, flow = clock(lambda: eng.flow_estimate(planes[0], planes[1]), reps)
    inner = flow[:, h // 8: -h // 8, w // 8: -w // 8]
    launches = 2 * (scales - 1) + scales * P.warps * (1 + P.iterations) + (scales - 1) + 1
    say(f"{h}x{w}: one flow {1e3 * t:.2f} ms (mean of {reps}; {launches} launches, {1e6 * t / launches:.1f} us per launch); "
        f"inner mean flow ({float(inner[0].mean()):.3f}, {float(inner[1].mean()):.3f}) px for a true (3, 1)")
    # the stages, scale by scale
    A, B = [planes[0]], [planes[1]]
    cost = {"reduce": 0.0, "linearise": 0.0, "sweeps": 0.0, "prolong": 0.0}
    for s in range(1, scales):
        for pyr in (A, B):
            eng.flow_reduce(pyr[-1])
            dt, r = clock(lambda: eng.flow_reduce(pyr[-1]), reps)
            cost["reduce"] += dt
            pyr.append(r)
    top_sweeps = 0.0
    f = torch.zeros((2,) + sizes[-1], dtype=torch.float32, device="cuda")
    for s in range(scales - 1, -1, -1):
        eng.flow_linearize(A[s], B[s], f)
        dt, (ix, iy, rho) = clock(lambda: eng.flow_linearize(A[s], B[s], f), reps)
        cost["linearise"] += P.warps * dt
        eng.flow_sweeps(ix, iy, rho, f, P.alpha, P.iterations)
        dt, g = clock(lambda: eng.flow_sweeps(ix, iy, rho, f, P.alpha, P.iterations), reps)
        cost["sweeps"] += P.warps * dt
        if s == 0:
            top_sweeps = dt / P.iterations
        if s > 0:
            eng.flow_prolong(g, *sizes[s - 1])
            dt, f = clock(lambda: eng.flow_prolong(g, *sizes[s - 1]), reps)
            cost["prolong"] += dt
    total = sum(cost.values())
    say(f"{h}x{w}: stages (entry points, one synchronise per call): " + ", ".join(f"{k} {1e3 * v:.2f} ms ({v / total:.1%})" for k, v in cost.items())
        + f"; a top-scale sweep {1e6 * top_sweeps:.1f} us = {4 * 7 * h * w / top_sweeps / 1e12:.2f} TB/s over its seven planes")
eng.close()

old = open(out_path).read() if os.path.exists(out_path) else ""
if BEGIN in old and END in old:
    new = old[:old.index(BEGIN)] + "\n".join([BEGIN] + lines + [END]) + old[old.index(END) + len(END):]
else:
    new = old + ("\n" if old and not old.endswith("\n") else "") + "\n".join([BEGIN] + lines + [END]) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(new)
