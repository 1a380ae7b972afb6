"""GPU: closure time of the L=2 benchmark job (bench.build_job, levels 1024x1536, 512x768, 256x384) with the MRF term
(nst_level_set_patches) off, on relu4_1 at style strides 1 and 2 on every level, and on relu3_1 + relu4_1 on the two lower
levels only, alternated in one process; the search launches of one timed closure of each setting (an event pair around the
key clear, the search kernel and the decode: timing mode 2, read through nst_dump_last_closure) with the achieved TF/s -
algorithmic (2 n m 9 C) and executed on the matrix pipe (three fp16 MFMAs per product block: three times that); and the whole
nst_patch_match call (scratch allocation, dictionary preparation, absmax, search, decode, synchronise) on random maps of the
benchmark job's sizes.
    python tools/time_mrf.py [reps=20]"""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
R41 = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
R31_41 = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0)
# (weights, stride, levels that carry the term)
SETTINGS = {"off": (None, 1, ()), "relu4_1 stride 1, every level": (R41, 1, (0, 1, 2)), "relu4_1 stride 2, every level": (R41, 2, (0, 1, 2)),
            "relu3_1 + relu4_1 stride 1, levels 1 and 2": (R31_41, 1, (1, 2))}


def setup(setting):
    w, stride, on = setting
    eng.clear_patches()
    for l in on:
        eng.set_patches(l, eng.prepare_img(sl[l]), w, stride)


def rate(n):
    for _ in range(2):
        eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        eng.closure(x, cw, sw, tvw)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def search_launches():
    """(h, w, C, m, ms) of every search launch of one timed closure: the lines of nst_dump_last_closure (stderr) whose layer
    tag is 100 + map index."""
    eng.set_timing(2)
    try:
        eng.closure(x, cw, sw, tvw)
        eng.closure(x, cw, sw, tvw)
        torch.cuda.synchronize()
        sys.stderr.flush()
        with tempfile.TemporaryFile(mode="w+") as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                eng.lib.nst_dump_last_closure(eng.ctx)
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            text = tmp.read()
    finally:
        eng.set_timing(0)
    out = []
    for m in re.finditer(r"cls 3 +(\d+)x(\d+) +cin +(\d+) cout +(\d+) taps 9 layer +(1\d\d) +([0-9.]+) ms", text):
        out.append(tuple(int(v) for v in m.groups()[:4]) + (float(m.group(6)),))
    return out


for l in range(levels):
    eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))
ROUNDS = 3
runs = {m: [] for m in SETTINGS}
for r in range(ROUNDS):
    for name, setting in SETTINGS.items():
        setup(setting)
        runs[name].append(rate(reps if name == "off" else max(reps // 4, 3)))
kernels = {}
for name, setting in SETTINGS.items():
    if name != "off":
        setup(setting)
        kernels[name] = search_launches()
eng.clear_patches()
for name, ms in runs.items():
    print(f"closure, {name}: " + ", ".join(f"{v:.2f}" for v in ms) + f" ms (median {sorted(ms)[len(ms) // 2]:.2f})", flush=True)
for name, recs in kernels.items():
    for h, w, c, m, ms in recs:
        n = (h - 2) * (w - 2)
        flop = 2.0 * n * m * 9 * c
        print(f"search launch in the closure, {name}: map {h}x{w}x{c}, n = {n}, m = {m}, K = {9 * c}: {ms:.3f} ms, "
              f"{flop / ms / 1e9:.1f} TF/s algorithmic, {3 * flop / ms / 1e9:.1f} TF/s executed f16", flush=True)
print(f"context bytes with the term cleared: {eng.bytes()}", flush=True)

# the whole nst_patch_match call
g = torch.Generator(device="cuda").manual_seed(1)
for what, (h, w, c, stride) in {"relu4_1 of 1024x1536, stride 1": (128, 192, 512, 1), "relu4_1 of 1024x1536, stride 2": (128, 192, 512, 2),
                                "relu4_1 of 512x768, stride 1": (64, 96, 512, 1), "relu4_1 of 256x384, stride 1": (32, 48, 512, 1),
                                "relu3_1 of 512x768, stride 1": (128, 192, 256, 1), "relu3_1 of 256x384, stride 1": (64, 96, 256, 1),
                                "relu2_1 of 256x384, stride 1": (128, 192, 128, 1)}.items():
    f = torch.relu(torch.randn((h, w, c), generator=g, device="cuda") * 3.0 - 1.0)
    fs = torch.relu(torch.randn((h, w, c), generator=g, device="cuda") * 3.0 - 1.0)
    eng.patch_match(f, fs, stride)
    torch.cuda.synchronize()
    n_rep = 3
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n_rep):
        eng.patch_match(f, fs, stride)
    t1.record(); torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / n_rep
    n = (h - 2) * (w - 2)
    m = ((h - 3) // stride + 1) * ((w - 3) // stride + 1)
    flop = 2.0 * n * m * 9 * c
    print(f"nst_patch_match call, {what}: n = {n}, m = {m}, K = {9 * c}: {ms:.2f} ms, {flop / ms / 1e9:.1f} TF/s algorithmic, "
          f"{3 * flop / ms / 1e9:.1f} TF/s executed f16", flush=True)
