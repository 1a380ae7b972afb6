"""GPU: set-up time of the targets of the L=2 benchmark job (bench.build_job: 1024x1536 + 512x768 + 256x384, style pyramids
of the same sizes) - all levels through set_targets (nst_level_set_targets) and through set_targets_blend
(nst_level_set_targets_blend) with K = 1, 2, 3 style images, synchronised wall time, median of `reps` after one warm-up.
Run from a checkout without set_targets_blend it reports set_targets alone (the same-box comparison with the parent
commit: alternate the two checkouts).
    python tools/time_style_blend.py [reps=5]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from artstyletransfer_amd import device_image, synthetic

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
levels = 3
eng, x, cfg, host = bench.build_job(levels, 0, 0)
cl = [eng.prepare_img(torch.from_numpy(a).cuda()) for a in host[0]]
styles = [[eng.prepare_img(torch.from_numpy(a).cuda()) for a in host[1]]]
H, W = host[1][0].shape[:2]
for seed in (4, 6):          # two further style images of the bench job's size
    sd = device_image.upload(eng, synthetic.image(H, W, seed=seed))
    styles.append([eng.prepare_img(t) for t in device_image.pyramid(eng, sd, levels)])


def timed(fn):
    ms = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[1:])
    return ms[len(ms) // 2], ms[0], ms[-1]


def plain():
    for l in range(levels):
        eng.set_targets(l, cl[l], styles[0][l])


def blend(k):
    def run():
        for l in range(levels):
            eng.set_targets_blend(l, cl[l], [s[l] for s in styles[:k]], [1.0] * k)
    return run


rows = [("set_targets", plain)]
if hasattr(eng, "set_targets_blend"):
    rows += [(f"set_targets_blend K={k}", blend(k)) for k in (1, 2, 3)]
for name, fn in rows:
    med, lo, hi = timed(fn)
    print(f"{name:24s} {med:8.2f} ms  (min {lo:.2f}, max {hi:.2f}; {levels} levels, median of {reps})", flush=True)
eng.close()
