"""GPU: a sha256 per job of the image the host layers between Config and the engine produce - the five device jobs of
tools/job_transcript.py (between them every optional setting of job_settings.SETTINGS), each through _make_job after two
Adam steps and after one L-BFGS step, and one 256x384 one-level job through the public neural_style_transfer() generator
with laplacian_weight, gram_shift="mean" and moment_weight set (every yielded image, two Adam steps and one L-BFGS step).
Two trees drive the engine with the same calls and operands when every line agrees - run it in both in one visit of one
box and compare:  python tools/digest_job_paths.py > a.txt   (the digests are not goldens: they depend on the build)."""
import asyncio
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
from artstyletransfer_amd import config, neural_nets, synthetic
from artstyletransfer_amd import neural_style_transfer as impl
from job_transcript import jobs

CW, SW, TVW = 1e3, 4e5, 1e2


def line(name, h):
    print(f"{name:64s} {h.hexdigest()}", flush=True)


def device_job(name, optimizer, steps, style, content, init, settings):
    job = impl._make_job(torch.device("cuda", 0), optimizer, style, content, init, 10.0, **settings)
    try:
        h = hashlib.sha256()
        for _ in range(steps):
            job.step(CW, SW, TVW)
            job.snapshot(0)()
            h.update(np.ascontiguousarray(job.image(0)).tobytes())
        line(f"{name}: {optimizer}, {steps} step(s)", h)
    finally:
        job.close()


def public_job(optimizer, iters):
    cfg = config.Config(levels_num=1, iters_num=iters, optimizer=optimizer)
    pair = impl.ContentStylePair(("c", synthetic.image(256, 384, 1)), ("s", synthetic.image(256, 384, 2)))

    async def run():
        h = hashlib.sha256()
        async for percent, img in impl.neural_style_transfer(
                pair, cfg.content_weight, cfg.style_weight, cfg.tv_weight, cfg.optimizer, cfg.model, "content", cfg.iters_num,
                cfg.levels_num, cfg.noise_factor, cfg.noise_levels, cfg.noise_levels_central_amplitude,
                cfg.noise_levels_peripheral_amplitude, cfg.noise_levels_dispersion, laplacian_weight=50.0, gram_shift="mean",
                moment_weight=1e3):
            h.update(np.array([percent], dtype=np.float64).tobytes())
            h.update(np.ascontiguousarray(img).tobytes())
        return h

    line(f"neural_style_transfer() 256x384, laplacian + gram_shift + moments: {optimizer}, {iters} step(s)", asyncio.run(run()))


neural_nets.set_weights(synthetic.vgg19_weights(bias_std=2.0))
for job_name, (style, content, init, settings) in jobs().items():
    device_job(job_name, "adam", 2, style, content, init, settings)
    device_job(job_name, "lbfgs", 1, style, content, init, settings)
public_job("adam", 2)
public_job("lbfgs", 1)
