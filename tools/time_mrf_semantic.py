"""GPU: what the semantic guidance of the MRF term (nst_level_set_patch_guidance) costs.  The L=2 benchmark job
(bench.build_job, levels 1024x1536, 512x768, 256x384) carries the term on relu4_1 of every level and on relu3_1 of the two
lower levels, which gives the search launches of DESIGN 4.16: n = m = 23 940 at K = 4608 and at K = 2304, n = m = 5828 (K = 4608
and 2304) and n = m = 1380.  Guided (four vertical bands, gamma = 1) and unguided closures are alternated in one process; of
each round one timed closure of each kind (an event pair around the key clear, the search kernel and the decode: timing mode
2, read through nst_dump_last_closure) gives the search launches (layer tag 100 + map index) and, guided, the rp passes (tag
200 + map index); the achieved TF/s are algorithmic (2 n m 9 C) and executed on the matrix pipe (three times that).
    python tools/time_mrf_semantic.py [rounds=4] [reps=5]"""
import os, re, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
levels = 3
eng, x_rgb, cfg, host = bench.build_job(levels, 0, 0)
cl = [torch.from_numpy(a).cuda() for a in host[0]]
sl = [torch.from_numpy(a).cuda() for a in host[1]]
x = eng.prepare_img(torch.from_numpy(host[2]).cuda())
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
R41 = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
R31_41 = (0.0, 0.0, 1.0, 1.0, 0.0, 0.0)
REGIONS, GAMMA = 4, 1.0


def bands(h, w):
    label = np.arange(w) * REGIONS // w
    planes = np.broadcast_to(label[None, None, :] == np.arange(REGIONS)[:, None, None], (REGIONS, h, w))
    return torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32)).cuda()


def setup(guided):
    for l in range(levels):
        eng.set_patches(l, eng.prepare_img(sl[l]), R41 if l == 0 else R31_41, 1)
        if guided:
            eng.set_patch_guidance(l, bands(*cl[l].shape[:2]), bands(*sl[l].shape[:2]), GAMMA)


def rate(n):
    eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        eng.closure(x, cw, sw, tvw)
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def launches():
    """{(tag // 100, h, w, C): (ms, m)} of one timed closure: tag 1xx the search launches (m: the dictionary's entries), 2xx
    the rp passes."""
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
    out = {}
    for m in re.finditer(r"cls 3 +(\d+)x(\d+) +cin +(\d+) cout +(\d+) taps 9 layer +([12]\d\d) +([0-9.]+) ms", text):
        h, w, c, entries, tag = (int(v) for v in m.groups()[:5])
        out[(tag // 100, h, w, c)] = (float(m.group(6)), entries)
    return out


for l in range(levels):
    eng.set_targets(l, eng.prepare_img(cl[l]), eng.prepare_img(sl[l]))
closure_ms = {False: [], True: []}
search = {False: {}, True: {}}
rp, dict_entries = {}, {}
for r in range(rounds):
    for guided in (False, True):
        setup(guided)
        closure_ms[guided].append(rate(reps))
        for (kind, h, w, c), (ms, entries) in launches().items():
            (search[guided] if kind == 1 else rp).setdefault((h, w, c), []).append(ms)
            if kind == 1:
                dict_entries[(h, w, c)] = entries
eng.clear_patches()


def spread(v):
    return f"{min(v):.3f} .. {max(v):.3f} (median {sorted(v)[len(v) // 2]:.3f})"


for guided in (False, True):
    print(f"closure, {'guided' if guided else 'unguided'}: " + ", ".join(f"{v:.2f}" for v in closure_ms[guided]) + " ms", flush=True)
for key in sorted(search[False], key=lambda k: -(k[0] * k[1] * k[2])):
    h, w, c = key
    n = (h - 2) * (w - 2)
    m = dict_entries[key]
    un, gd = search[False][key], search[True][key]
    mu, mg = sorted(un)[len(un) // 2], sorted(gd)[len(gd) // 2]
    flop = 2.0 * n * m * 9 * c
    print(f"search launch, map {h}x{w}x{c}, n = {n}, m = {m}, K = {9 * c}: unguided {spread(un)} ms = {flop / mu / 1e9:.1f} TF/s algorithmic, "
          f"{3 * flop / mu / 1e9:.1f} executed f16; guided {spread(gd)} ms = {flop / mg / 1e9:.1f} / {3 * flop / mg / 1e9:.1f} TF/s; guided / "
          f"unguided (medians) {mg / mu:.4f}, spread of the unguided runs {(max(un) - min(un)) / mu:.2%}; rp pass {spread(rp[key])} ms", flush=True)
    print("    rounds: unguided " + ", ".join(f"{v:.3f}" for v in un) + "; guided " + ", ".join(f"{v:.3f}" for v in gd), flush=True)
