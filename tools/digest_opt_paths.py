"""GPU: a sha256 per result of the optimiser driver (csrc/nst_opt.cpp) through the public engine API, on the 35x51 two-level
synthetic job of tests/hip_helpers.setup: Adam with and without loss rows, L-BFGS at max_eval 1, at max_eval 26 under lr 1
(steps are taken and the history grows; both direction forms) and - at lr 100, where trial points are rejected - at
max_eval 4 under every combination of its switches (lbfgs_gram, closure reuse, lazy backward), the
level-sharded driver through the reduce hook and through the C communicator (a world of one), a step of the luminance job,
and the update arithmetic alone (nst_lbfgs_direction, nst_adam_step).  A driver line digests x after every step, every
nst_step_info field, the loss rows, nst_opt_history, nst_opt_closure_stats and nst_opt_backward_stats; stderr says which
branches each job took (accepted steps, pairs held, closures served, forward halves skipped).
Two builds of the library (NST_LIB names the other one, as tools/ab_bench.sh uses it) drive the same launches with the same
operands when every line agrees:  python tools/digest_opt_paths.py > a.txt; NST_LIB=/path/libnst_hip.so python tools/digest_opt_paths.py > b.txt"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from artstyletransfer_amd import host_image, synthetic
from artstyletransfer_amd.engine import Communicator, PixelOptimizer, StyleEngine
from hip_helpers import CW, SW, TVW, dev, levels, setup
from oracle import cpu_ref

H, W, NLEV = 35, 51, 2
WEIGHTS = synthetic.vgg19_weights(bias_std=2.0)
CONTENT, STYLE = levels(H, W, NLEV, 1), levels(H, W, NLEV, 2)
START = (0.6 * CONTENT[0] + 0.4 * STYLE[0]).astype(np.float32)


def line(name, h):
    print(f"{name:52s} {h.hexdigest()}", flush=True)


def rgb_job(e):
    setup(e, CONTENT, STYLE)
    return dev(cpu_ref.prepare_img(START))


def luminance_job(e):
    e.configure(NLEV, H, W)
    e.set_color("luminance")
    alpha, beta = host_image.luminance_params(host_image.color_stats(CONTENT[0]), host_image.color_stats(STYLE[0]))
    for l in range(NLEV):
        e.set_targets(l, dev(torch.from_numpy(host_image.luminance(CONTENT[l]))),
                      dev(torch.from_numpy(host_image.luminance(STYLE[l], alpha, beta))))
    return dev(torch.from_numpy(host_image.luminance(START)).reshape(1, 1, H, W))


class NoPeers:
    """torch.distributed's all_reduce for a world of one: the sum over the ranks is what the rank holds."""

    class ReduceOp:
        SUM = None

    @staticmethod
    def all_reduce(t, op=None, group=None):
        return None


def drive(name, kind, lr, max_eval, steps, job=rgb_job, want_losses=True, prepare=None, **options):
    e = StyleEngine(WEIGHTS, 0, **options)
    opt = None
    try:
        x = job(e)
        opt = PixelOptimizer(e, kind, lr, max_eval)
        if prepare:
            prepare(opt)
        h = hashlib.sha256()
        accepted = ""
        for _ in range(steps):
            info, rows = opt.step(x, CW, SW, TVW, want_losses=want_losses)
            accepted += str(info.accepted)
            torch.cuda.synchronize()
            h.update(np.ascontiguousarray(x.cpu().numpy()).tobytes())
            h.update(np.array([info.closures, info.total_closures, info.accepted, info.history], dtype=np.int32).tobytes())
            h.update(np.array([info.loss, info.lr, info.t], dtype=np.float32).tobytes())     # (NaN loss: the same bits)
            if rows is not None:
                h.update(np.ascontiguousarray(rows).tobytes())
            h.update(np.array(opt.history() + opt.closure_stats() + opt.backward_stats(), dtype=np.int64).tobytes())
        line(name, h)
        # (stderr: which branches the job took - not part of the digest lines)
        print(f"  {name}: accepted {accepted}, (pairs, n_iter) {opt.history()}, (evaluated, served) {opt.closure_stats()}, "
              f"(forward only, skipped) {opt.backward_stats()}", file=sys.stderr, flush=True)
    finally:
        if opt is not None:
            opt.close()
        e.close()


drive("adam, 6 steps, loss rows", "adam", 10.0, 1, 6)
drive("adam, 6 steps, no loss rows", "adam", 10.0, 1, 6, want_losses=False)
drive("lbfgs max_eval 1, 8 steps", "lbfgs", 10.0, 1, 8)
drive("lbfgs max_eval 26 lr 1, 12 steps", "lbfgs", 1.0, 26, 12)              # steps that are taken: the history grows
drive("lbfgs max_eval 26 lr 1, lbfgs_gram off", "lbfgs", 1.0, 26, 12, lbfgs_gram=False)
drive("lbfgs max_eval 4 lr 100, 8 steps", "lbfgs", 100.0, 4, 8)
drive("lbfgs max_eval 4 lr 100, lbfgs_gram off", "lbfgs", 100.0, 4, 8, lbfgs_gram=False)
drive("lbfgs max_eval 4 lr 100, reuse off", "lbfgs", 100.0, 4, 8, prepare=lambda o: o.set_closure_reuse(False))
drive("lbfgs max_eval 4 lr 100, lazy off", "lbfgs", 100.0, 4, 8, prepare=lambda o: o.set_lazy_backward(False))
drive("lbfgs max_eval 4 lr 100, reuse and lazy off", "lbfgs", 100.0, 4, 8,
      prepare=lambda o: (o.set_closure_reuse(False), o.set_lazy_backward(False)))
drive("lbfgs max_eval 4 lr 100, sharded, reduce hook", "lbfgs", 100.0, 4, 8, prepare=lambda o: o.shard_levels(0, 1, NoPeers))
drive("adam, sharded, reduce hook, no loss rows", "adam", 10.0, 1, 6, want_losses=False,
      prepare=lambda o: o.shard_levels(0, 1, NoPeers))
comm = Communicator(0, 0, 1, Communicator.unique_id())
try:
    drive("lbfgs max_eval 4 lr 100, sharded, C communicator", "lbfgs", 100.0, 4, 8, prepare=lambda o: o.shard_levels_comm(comm))
    drive("adam, sharded, C communicator", "adam", 10.0, 1, 6, prepare=lambda o: o.shard_levels_comm(comm))
finally:
    comm.close()
drive("lbfgs max_eval 4, luminance job, 1 step", "lbfgs", 10.0, 4, 1, job=luminance_job)
drive("adam, luminance job, 1 step", "adam", 10.0, 1, 1, job=luminance_job)

# ---- the update arithmetic alone, at a length with a scalar tail (n mod 4 = 1)
N = 3 * 53 * 37 + 2
e = StyleEngine(WEIGHTS, 0)
try:
    gen = torch.Generator().manual_seed(7)
    grad = torch.randn(N, generator=gen)
    ss = [torch.randn(N, generator=gen) * 0.1 for _ in range(7)]
    ys = [2.0 * s + 0.03 * torch.randn(N, generator=gen) for s in ss]      # positive y.s
    for m in (0, 1, 7):
        ro = [float(1.0 / y.dot(s)) for y, s in zip(ys[:m], ss[:m])]
        h_diag = float(ys[m - 1].dot(ss[m - 1]) / ys[m - 1].dot(ys[m - 1])) if m else 1.0
        for form in (0, 1):
            d = e.lbfgs_direction(dev(grad), [dev(t) for t in ys[:m]], [dev(t) for t in ss[:m]], ro, h_diag, form)
            torch.cuda.synchronize()
            h = hashlib.sha256(np.ascontiguousarray(d.cpu().numpy()).tobytes())
            line(f"lbfgs_direction m={m} form={form} n={N}", h)
    x, mom, var = dev(torch.randn(N, generator=gen) * 50), dev(torch.randn(N, generator=gen) * 0.5), dev(torch.rand(N, generator=gen) * 4)
    e.adam_step(x, dev(grad * 3), mom, var, 7, 9.93)
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (x, mom, var):
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    line(f"adam_step k=7 n={N}", h)
    h = hashlib.sha256(np.array([e.bytes()], dtype=np.int64).tobytes())
    line("nst_ctx_bytes after the standalone calls", h)
finally:
    e.close()
