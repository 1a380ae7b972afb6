"""GPU: what the long-term anchor adds to a frame's set-up (video.neural_style_transfer_video_long_term) at the benchmark
job's top-level size, 1024x1536: per offset in use two optical flows, the flow weights and a warp, then one fold
(StyleEngine.anchor_fold) - timed for the offsets (1), (1,2) and (1,2,4) under both estimators, the six variants alternated
three times in one process; and the fold launch alone, beside the estimate from bytes.  The frames are a synthetic image moved
by (3, 1) pixels per frame; the earlier results are other synthetic images (the set-up does not look at what they show).
    python tools/time_long_term.py [reps=3] [out=profiles/r19_long_term.txt]
The figures replace the section between the two marker lines of `out` (the rest of the file is kept)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from artstyletransfer_amd import synthetic, video
from artstyletransfer_amd.engine import StyleEngine
from artstyletransfer_amd.flow_modes import FlowParams, TVL1Params

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                            "r19_long_term.txt")
BEGIN, END = "== timing (tools/time_long_term.py) ==", "== end of timing =="
HBM = 6.3e12          # achievable bytes per second of the MI355X's HBM: the yardstick of the estimate from bytes
H, W, C_ = 1024, 1536, 3
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


img = synthetic.image(H, W, seed=1)
# frame i - j for j = 0, 1, 2, 4: the image moved back by j steps of (3, 1) pixels
planes = {j: eng.luminance(torch.from_numpy(np.ascontiguousarray(np.roll(img, (-j, -3 * j), axis=(0, 1)), dtype=np.float32)).cuda()).reshape(H, W)
          for j in (0, 1, 2, 4)}
results = {j: torch.from_numpy(np.ascontiguousarray(synthetic.image(H, W, seed=10 + j), dtype=np.float32)).cuda().permute(2, 0, 1).contiguous()
           for j in (1, 2, 4)}


def setup(offsets, params):
    """The device work of the driver's start callable for one frame, the luminance planes in hand."""
    back, forw = [], []
    for j in offsets:
        back.append(eng.flow_estimate(planes[0], planes[j], params))
        forw.append(eng.flow_estimate(planes[j], planes[0], params))
    omega, c, _ = video.long_term_anchor(eng, [results[j] for j in offsets], back, forw)
    omega = omega.permute(1, 2, 0).contiguous()
    return video.level_anchors(eng, omega, 3, False), video.level_weights(c, 3)


variants = [(name, par, offs) for offs in ((1,), (1, 2), (1, 2, 4)) for name, par in (("Horn-Schunck", FlowParams()), ("TV-L1", TVL1Params()))]
for _, par, offs in variants[:2]:
    setup(offs, par)                                                        # warm-up: both estimators once
times = {(name, offs): [] for name, _, offs in variants}
for _ in range(reps):
    for name, par, offs in variants:
        times[(name, offs)].append(clock(lambda: setup(offs, par))[0])
say(f"{H}x{W}, three levels: a frame's set-up on the device (per offset two flows, flow weights, a warp; one fold; the level anchors and "
    f"weights), {reps} rounds over the six variants in one process:")
for name, _, offs in variants:
    t = times[(name, offs)]
    say(f"  {name:12s} offsets {offs}: {1e3 * np.mean(t):8.2f} ms (min {1e3 * min(t):.2f}, max {1e3 * max(t):.2f})")

# the fold alone: (J + 1)(C + 1) planes plus the J planes of parts when they are asked for
for J in (1, 2, 3, 8):
    src = [torch.rand((C_, H, W), device="cuda") for _ in range(J)]
    wts = [(torch.rand((H, W), device="cuda") > 0.3).float() for _ in range(J)]
    mixed = [torch.rand((H, W), device="cuda") for _ in range(J)]
    for what, planes_w in (("weights of 0 and 1", wts), ("fractional weights", mixed)):
        eng.anchor_fold(src, planes_w)
        dt, _ = clock(lambda: eng.anchor_fold(src, planes_w), 20)
        nbytes = 4 * (J + 1) * (C_ + 1) * H * W
        say(f"  fold alone J={J}, {what}: {1e6 * dt:.1f} us a call (20 calls, one synchronise; torch allocates the outputs); {nbytes / 1e6:.0f} MB "
            f"if every plane is read = {1e6 * nbytes / HBM:.1f} us at {HBM / 1e12:.1f} TB/s -> {nbytes / dt / 1e12:.2f} TB/s")
eng.close()

old = open(out_path).read() if os.path.exists(out_path) else ""
if BEGIN in old and END in old:
    new = old[:old.index(BEGIN)] + "\n".join([BEGIN] + lines + [END]) + old[old.index(END) + len(END):]
else:
    new = old + ("\n" if old and not old.endswith("\n") else "") + "\n".join([BEGIN] + lines + [END]) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
open(out_path, "w").write(new)
