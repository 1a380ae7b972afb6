"""GPU: the self-similarity term (nst_level_set_selfsim) on the L=2 benchmark job (bench.build_job, levels 1024x1536, 512x768,
256x384).
1. the launches of every weighted map - relu2_1 (C = 128), relu3_1 (256), relu4_1 and conv4_2 (512) of the top level - at 1024
   and 4096 samples, inside one timed closure (timing mode 2, read through nst_dump_last_closure; layer tag 220 + map: the
   matrix kernel; 240 + map: column sums, value and decision pass; 230 + map: W, U and the fp32 gradient product):
   milliseconds, and for the matrix kernel TF/s, algorithmic (2 n n C) and executed on the matrix pipe (three fp16 MFMAs per
   product block), for the gradient product TF/s of fp32 work (2 n n C);
2. a device copy of the same bytes as the n x n passes stream (D, the content's D, the signs), for comparison;
3. the closure with the term off and on the content map at 1024 and 4096 samples, alternated in one process;
4. the term's value on the job's start image and the weight that makes it a tenth of each level total;
5. the same launches at n = 4096 exactly for C = 128, 256 and 512: a one-level 512x512 job on seeded noise images, whose
   relu2_1, relu3_1, relu4_1 and conv4_2 have 4096 samples at strides 4, 2, 1 and 1.
    python tools/time_selfsim.py [reps=20]          (profiles/r25_selfsim.txt keeps its output)"""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from artstyletransfer_amd import selfsim_modes

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
CONTENT = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
FOUR = (0.0, 1.0, 1.0, 1.0, 1.0, 0.0)
SETTINGS = {"off": None, "conv4_2, 1024 samples, every level": (CONTENT, 1024), "conv4_2, 4096 samples, every level": (CONTENT, 4096)}


def setup(setting, only_levels=None):
    eng.clear_selfsim()
    if setting is None:
        return
    w, samples = setting
    shapes = [tuple(t.shape[:2]) for t in cl]
    strides = selfsim_modes.level_strides((w, samples, 1e-5, only_levels), shapes)
    for l in range(levels):
        if strides[l] is not None:
            eng.set_selfsim(l, eng.prepare_img(cl[l]), w, strides[l])


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


def term_launches():
    """(tag, n, cin, cout, ms) of every tagged launch group of one timed closure: the lines of nst_dump_last_closure (stderr)
    whose layer tag is 220 .. 245."""
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
    for m in re.finditer(r"cls 3 +(\d+)x1 +cin +(\d+) cout +(\d+) taps 1 layer +(2[234]\d) +([0-9.]+) ms", text):
        n, cin, cout, tag = (int(v) for v in m.groups()[:4])
        out.append((tag, n, cin, cout, float(m.group(5))))
    return out


for l in range(levels):
    eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))
ROUNDS = 3
runs = {m: [] for m in SETTINGS}
for r in range(ROUNDS):
    for name, setting in SETTINGS.items():
        setup(setting)
        runs[name].append(rate(reps if name == "off" else max(reps // 2, 3)))
setup(None)
base = eng.bytes()
for name, setting in SETTINGS.items():
    if setting is not None:
        setup(setting)
        print(f"context bytes, {name}: {eng.bytes()} (term cleared: {base})", flush=True)
for name, ms in runs.items():
    print(f"closure, {name}: " + ", ".join(f"{v:.2f}" for v in ms) + f" ms (median {sorted(ms)[len(ms) // 2]:.2f})", flush=True)

# the kernels: four maps of the top level, so that C = 128, 256 and 512 are met at both sample counts
for samples in (1024, 4096):
    setup((FOUR, samples), only_levels=[0])
    for tag, n, cin, cout, ms in term_launches():
        i = tag % 10
        if tag < 230:
            flop = 2.0 * n * n * cin
            print(f"matrix kernel, {samples} samples, map {i}: C = {cin}, n = {n}: {ms:.3f} ms, {flop / ms / 1e9:.1f} TF/s algorithmic, "
                  f"{3 * flop / ms / 1e9:.1f} TF/s executed f16", flush=True)
        elif tag < 240:
            flop = 2.0 * n * n * cout
            print(f"gradient (W, U, fp32 product, scatter), {samples} samples, map {i}: C = {cout}, n = {n}: {ms:.3f} ms, "
                  f"{flop / ms / 1e9:.1f} TF/s fp32 over the whole group", flush=True)
        else:
            nbytes = 13.0 * n * n           # D read twice (column sums, value), the content's D once, the signs written
            print(f"n x n passes (column sums, value and decisions), {samples} samples, map {i}: n = {n}: {ms:.3f} ms, "
                  f"{nbytes / ms / 1e6:.0f} GB/s of {nbytes / 1e6:.1f} MB", flush=True)
    n = selfsim_modes.samples_of(128, 192, selfsim_modes.stride_for(128, 192, samples))
    a = torch.empty(13 * n * n // 2, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(10):
        b.copy_(a)
    t1.record(); torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / 10
    print(f"device copy moving the same {13.0 * n * n / 1e6:.1f} MB, read plus written (n = {n}): {ms:.3f} ms, {13.0 * n * n / ms / 1e6:.0f} GB/s",
          flush=True)

# magnitudes on the start image
setup((CONTENT, 1024))
_, rows = eng.closure(x, cw, sw, tvw)
rows = rows.cpu().numpy()[:-1].reshape(levels, 4)
vals = eng.selfsim_losses().cpu().numpy()
for l in range(levels):
    rest = float(rows[l, 0]) - float(vals[l, 4])
    print(f"level {l}: selfsim of conv4_2 at 1024 samples {vals[l, 4]:.5f}; level total without the term {rest:.4e}; the weight that makes "
          f"the term a tenth of the total: {rest / 9.0 / max(float(vals[l, 4]), 1e-30):.3e}", flush=True)
eng.clear_selfsim()

# n = 4096 exactly: a 512x512 one-level job (relu2_1 256x256 / 4, relu3_1 128x128 / 2, relu4_1 and conv4_2 64x64 / 1)
g = torch.Generator(device="cuda").manual_seed(1)
sq = [(torch.rand((512, 512, 3), generator=g, device="cuda") * 255.0).contiguous() for _ in range(3)]
eng.configure(1, 512, 512)
eng.set_targets(0, eng.prepare_img(sq[0]), eng.prepare_img(sq[1]))
x = eng.prepare_img(sq[2])
eng.set_selfsim(0, eng.prepare_img(sq[0]), FOUR, (1, 4, 2, 1, 1, 1))
for tag, n, cin, cout, ms in term_launches():
    i = tag % 10
    if tag < 230:
        flop = 2.0 * n * n * cin
        print(f"512x512 job, matrix kernel, map {i}: C = {cin}, n = {n}: {ms:.3f} ms, {flop / ms / 1e9:.1f} TF/s algorithmic, "
              f"{3 * flop / ms / 1e9:.1f} TF/s executed f16", flush=True)
    elif tag < 240:
        flop = 2.0 * n * n * cout
        print(f"512x512 job, gradient (W, U, fp32 product, scatter), map {i}: C = {cout}, n = {n}: {ms:.3f} ms, "
              f"{flop / ms / 1e9:.1f} TF/s fp32 over the whole group", flush=True)
    else:
        print(f"512x512 job, n x n passes, map {i}: n = {n}: {ms:.3f} ms, {13.0 * n * n / ms / 1e6:.0f} GB/s of {13.0 * n * n / 1e6:.1f} MB", flush=True)
eng.clear_selfsim()
