"""GPU: the relaxed EMD term (nst_level_set_remd) on the L=2 benchmark job (bench.build_job, levels 1024x1536, 512x768, 256x384).
1. the two search launches of every weighted map - relu2_1 (C = 128), relu3_1 (256), relu4_1 (512) of every level - at 4096 and
   16384 samples a side, inside one timed closure (an event pair around each direction's key clear, search kernel and decode:
   timing mode 2, read through nst_dump_last_closure; layer tag 200 + map for direction A, 210 + map for direction B):
   milliseconds and TF/s, algorithmic (2 n m C) and executed on the matrix pipe (three fp16 MFMAs per product block);
2. the other passes, as whole stand-alone calls on random maps of the same sizes: nst_remd_match (scratch, absmax, norms and
   pack of both sides, both searches, synchronise) and nst_remd_term (norms, value, gradient);
3. the closure with the term off and on, alternated in one process.
    python tools/time_remd.py [reps=20]          (profiles/r24_remd.txt keeps its output)"""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from artstyletransfer_amd import remd_modes

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
W = (0.0, 1.0, 1.0, 1.0, 0.0, 0.0)
SETTINGS = {"off": None, "relu2_1 + relu3_1 + relu4_1, 4096 samples, every level": 4096,
            "relu2_1 + relu3_1 + relu4_1, 16384 samples, every level": 16384}


def setup(samples):
    eng.clear_remd()
    if samples is None:
        return
    shapes = [tuple(t.shape[:2]) for t in cl]
    sshapes = [tuple(t.shape[:2]) for t in sl]
    strides = remd_modes.level_strides((W, samples, 1e-5, None), shapes, sshapes)
    for l in range(levels):
        eng.set_remd(l, eng.prepare_img(sl[l]), W, strides[l][0], strides[l][1])


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
    """(n, m, C, direction, ms) of every search launch of one timed closure: the lines of nst_dump_last_closure (stderr) whose
    layer tag is 200 + map (direction A) or 210 + map (direction B); they carry n as h x w = n x 1 and m as cout."""
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
    for m in re.finditer(r"cls 3 +(\d+)x1 +cin +(\d+) cout +(\d+) taps 1 layer +(2[01]\d) +([0-9.]+) ms", text):
        n, c, mm, tag = (int(v) for v in m.groups()[:4])
        out.append((n, mm, c, "A" if tag < 210 else "B", float(m.group(5))))
    return out


for l in range(levels):
    eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))
ROUNDS = 3
runs = {m: [] for m in SETTINGS}
for r in range(ROUNDS):
    for name, samples in SETTINGS.items():
        setup(samples)
        runs[name].append(rate(reps if name == "off" else max(reps // 2, 3)))
kernels = {}
for name, samples in SETTINGS.items():
    if samples is not None:
        setup(samples)
        kernels[name] = search_launches()
        print(f"context bytes, {name}: {eng.bytes()}", flush=True)
eng.clear_remd()
print(f"context bytes with the term cleared: {eng.bytes()}", flush=True)
for name, ms in runs.items():
    print(f"closure, {name}: " + ", ".join(f"{v:.2f}" for v in ms) + f" ms (median {sorted(ms)[len(ms) // 2]:.2f})", flush=True)
for name, recs in kernels.items():
    for n, m, c, d, ms in recs:
        flop = 2.0 * n * m * c
        print(f"search launch in the closure, {name}: direction {d}, C = {c}, n = {n}, m = {m}: {ms:.3f} ms, "
              f"{flop / ms / 1e9:.1f} TF/s algorithmic, {3 * flop / ms / 1e9:.1f} TF/s executed f16", flush=True)


def timed(fn, n_rep=5):
    fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n_rep):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n_rep


# the stand-alone calls on random maps of the benchmark job's top level
g = torch.Generator(device="cuda").manual_seed(1)
for samples in (4096, 16384):
    for what, (h, w, c) in {"relu2_1 of 1024x1536": (512, 768, 128), "relu3_1 of 1024x1536": (256, 384, 256),
                            "relu4_1 of 1024x1536": (128, 192, 512)}.items():
        f = torch.relu(torch.randn((h, w, c), generator=g, device="cuda") * 3.0 - 1.0)
        fs = torch.relu(torch.randn((h, w, c), generator=g, device="cuda") * 3.0 - 1.0)
        s = remd_modes.stride_for(h, w, samples)
        n = remd_modes.samples_of(h, w, s)
        nna, nnb = eng.remd_match(f, fs, s, s)
        ms_match = timed(lambda: eng.remd_match(f, fs, s, s))
        ms_term = {sd: timed(lambda: eng.remd_term(f, fs, nna, nnb, s, s, side=sd)) for sd in (0, 1)}
        flop = 2.0 * 2.0 * n * n * c
        print(f"stand-alone, {what}, {samples} samples (stride {s}, n = m = {n}): nst_remd_match {ms_match:.3f} ms "
              f"({3 * flop / ms_match / 1e9:.1f} TF/s executed f16 over the whole call); nst_remd_term (norms, value, gradient) side A "
              f"{ms_term[0]:.3f} ms, side B {ms_term[1]:.3f} ms", flush=True)
