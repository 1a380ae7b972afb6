"""GPU: closure rate of the L=2 benchmark job (bench.build_job) for the default feature maps and for other taps
(nst_job_set_taps): the forward stops, and the backward starts, at the deepest map in use.
    python tools/time_taps.py [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench

# (label, content index, style indices): the default, then the cases of tests/golden/make_fixtures_taps.py (a), (b)
CASES = (("default c4 s[0,1,2,3,5]", 4, [0, 1, 2, 3, 5]), ("(a) c1 s[0,1]", 1, [0, 1]), ("(b) c2 s[2,3]", 2, [2, 3]),
         ("relu4_1 top: c3 s[0,1,2,3]", 3, [0, 1, 2, 3]))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
levels = 3
eng, x, cfg, host = bench.build_job(levels, 0, 0)
content_levels, style_levels = host[0], host[1]
cw, sw, tvw = cfg.content_weight, cfg.style_weight, cfg.tv_weight
base = None
for label, c, s in CASES:
    eng.set_taps(c, s)
    for l in range(levels):
        eng.set_targets(l, eng.prepare_img(torch.from_numpy(content_levels[l]).cuda()),
                        eng.prepare_img(torch.from_numpy(style_levels[l]).cuda()))
    for _ in range(10):
        eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        eng.closure(x, cw, sw, tvw)
    t1.record(); torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / reps
    eng.set_timing(2)
    eng.closure(x, cw, sw, tvw)
    torch.cuda.synchronize()
    n3 = eng.last_closure_class(0)[1]
    eng.set_timing(0)
    base = base or ms
    print(f"{label:28s} {ms:7.3f} ms/closure  {1e3 / ms:6.1f} it/s  3x3 launches {n3:2d}  time saved {1 - ms / base:6.1%}")
eng.close()
