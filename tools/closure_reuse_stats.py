"""Evaluated / served closures (nst_opt_closure_stats) of the job bench.py measures (L = 2), L-BFGS with max_eval 1 and 26,
over 220 counted closures driven as bench.py drives them (JobLoop), closure reuse on (the default)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NST_SYNTHETIC_WEIGHTS", "1")

import torch  # noqa: E402

import bench  # noqa: E402
from artstyletransfer_amd.engine import PixelOptimizer  # noqa: E402

for max_eval in (1, 26):
    eng, x, cfg, _ = bench.build_job(3, 0, 0)
    opt = PixelOptimizer(eng, "lbfgs", 10.0, max_eval)
    job = bench.JobLoop(eng, x, opt, (cfg.content_weight, cfg.style_weight, cfg.tv_weight))
    eng.closure(x, cfg.content_weight, cfg.style_weight, cfg.tv_weight)
    torch.cuda.synchronize()
    job.split = 2 if max_eval == 1 else 0
    done, _ = job.run(220)
    ev, sv = opt.closure_stats()
    print(json.dumps({"max_eval": max_eval, "closures_counted": done, "optimizer_steps": job.opt_steps,
                      "accepted_steps": job.accepted, "evaluated": ev, "served": sv}), flush=True)
    opt.close()
    eng.close()
