"""GPU: the long-range style term, xcorr (nst_level_set_xcorr) on the L=2 benchmark job (bench.build_job, levels 1024x1536,
512x768, 256x384).
1. the closure with the term off and with the default maps (relu2_1, relu3_1, relu4_1) and shifts ((2,0) (0,2) (4,0) (0,4) (8,0)
   (0,8)) on every level, alternated three times in one process;
2. the value launches (every (level, map, shift) of the closure: partial products and finish, layer tag 250 of a timed
   closure);
3. the gradient launch of every weighted map of every level (layer tag 260 + map): milliseconds and the share of the 157 TF
   fp32-MFMA peak its 2 N C 2 C |D| FLOP reach;
4. the stand-alone statistic of one and of six shifts beside the stand-alone Gram (nst_gram, which also transposes its planar
   input) per map of the top level, events around the calls: the expectation to test is about twice a Gram per shift - all tile
   pairs plus a second staged operand.
    python tools/time_xcorr.py [reps=20]          (profiles/r26_xcorr.txt keeps its output)"""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from artstyletransfer_amd import xcorr_modes

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
W = (0.0, 1.0, 1.0, 1.0, 0.0, 0.0)
SHIFTS = xcorr_modes.normalize_shifts(xcorr_modes.DEFAULT_SHIFTS)
PEAK_F32_MFMA = 157e12
MAPS = {1: (128, 1), 2: (256, 2), 3: (512, 3)}          # map index -> (channels, scale)


def setup(on):
    eng.clear_xcorr()
    if on:
        for l in range(levels):
            eng.set_xcorr(l, eng.prepare_img(sl[l]), W, xcorr_modes.DEFAULT_SHIFTS)


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


def timed(fn, n=10):
    fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def term_launches():
    """(tag, t0, cin, cout, ms) of every tagged launch group of one timed closure: the lines of nst_dump_last_closure (stderr)
    whose layer tag is 250 .. 265."""
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
    for m in re.finditer(r"cls 3 +(\d+)x1 +cin +(\d+) cout +(\d+) taps 1 layer +(2[56]\d) +([0-9.]+) ms", text):
        n, cin, cout, tag = (int(v) for v in m.groups()[:4])
        out.append((tag, n, cin, cout, float(m.group(5))))
    return out


for l in range(levels):
    eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))
ROUNDS = 3
runs = {"off": [], "on": []}
for r in range(ROUNDS):
    for name in runs:
        setup(name == "on")
        runs[name].append(rate(reps if name == "off" else max(reps // 2, 3)))
setup(False)
base = eng.bytes()
setup(True)
print(f"context bytes with the term on every level: {eng.bytes()} (term cleared: {base})", flush=True)
for name, ms in runs.items():
    print(f"closure, term {name}: " + ", ".join(f"{v:.2f}" for v in ms) + f" ms (median {sorted(ms)[len(ms) // 2]:.2f})", flush=True)

# the launches inside a timed closure
shapes = [tuple(t.shape[:2]) for t in cl]
pair_flop = sum(2.0 * ((h >> sc) - dy) * ((w >> sc) - dx) * c * c for (h, w) in shapes for (c, sc) in MAPS.values() for dx, dy in SHIFTS)
launches = term_launches()
value = [(n, ms) for tag, n, _, _, ms in launches if tag == 250]
ms = sum(v[1] for v in value)
print(f"value launches (partial products + finish), {sum(v[0] for v in value)} items in {len(value)} launch(es): " +
      " + ".join(f"{v[1]:.3f}" for v in value) + f" = {ms:.3f} ms, {pair_flop / ms / 1e9:.1f} TF/s algorithmic, "
      f"{3 * pair_flop / ms / 1e9:.1f} TF/s executed f16", flush=True)
total = 0.0
for tag, n, cin, cout, ms in launches:
    if tag == 250:
        continue
    flop = 2.0 * n * cin * cout
    total += ms
    print(f"gradient launch, map {tag - 260}: N = {n}, K = {cin}, C = {cout}: {ms:.3f} ms, {flop / ms / 1e9:.1f} TF/s fp32 = "
          f"{flop / ms / 1e9 / (PEAK_F32_MFMA / 1e12):.1%} of the fp32-MFMA peak", flush=True)
print(f"gradient launches together: {total:.3f} ms", flush=True)
eng.clear_xcorr()

# the plain Gram batch of the same maps beside the stand-alone statistic, per map of the top level
h, w = shapes[0]
g = torch.Generator(device="cuda").manual_seed(1)
for i, (c, sc) in MAPS.items():
    f = torch.relu(torch.randn((h >> sc, w >> sc, c), generator=g, device="cuda")).contiguous()
    planar = f.permute(2, 0, 1).unsqueeze(0).contiguous()
    t_gram = timed(lambda: eng.gram(planar))
    for shifts in (((2, 0),), SHIFTS):
        t = timed(lambda: eng.xcorr(f, shifts))
        print(f"stand-alone, map {i} ({h >> sc}x{w >> sc}x{c}): nst_gram {t_gram:.3f} ms (with its transpose and absmax pass); nst_xcorr of "
              f"{len(shifts)} shift(s) {t:.3f} ms (with its absmax pass and scratch): {(t / t_gram):.2f} Grams", flush=True)
