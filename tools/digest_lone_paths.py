"""GPU: a sha256 per result of the calls that launch one image or one map at a time - the per-level closure (plain, a guided
level of R = 2, a centred Gram shift, moments), nst_vgg_features and its backward, nst_gram / nst_gram_shifted /
nst_guided_gram_backward on a 64- and a 256-channel map, and the stripe closure's window_begin sums - on small synthetic jobs.
Two builds of the library (NST_LIB names the other one, as tools/ab_bench.sh uses it) compute the same results exactly when
every line agrees:  python tools/digest_lone_paths.py > a.txt; NST_LIB=/path/libnst_hip.so python tools/digest_lone_paths.py > b.txt"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from artstyletransfer_amd import synthetic
from artstyletransfer_amd.engine import StyleEngine
from oracle import cpu_ref

CW, SW, TVW = 1e3, 4e5, 1e2
H, W, NLEV, HS, WS = 70, 52, 2, 48, 80
WEIGHTS = synthetic.vgg19_weights(bias_std=2.0)


def dev(t):
    return t.contiguous().to("cuda:0")


def prep(img):
    return dev(cpu_ref.prepare_img(img))


def digest(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    print(f"{name:44s} {h.hexdigest()}", flush=True)


def ramps(r, h, w):
    """(r, h, w) guidance planes in [0.75, 1] (the two pixels of the smallest map in use must carry a mass sum t^2 of at least
    1): plane 0 rises from left to right, plane 1 falls, ..."""
    x = torch.linspace(0.0, 0.25, w).repeat(h, 1)
    return dev(torch.stack([0.75 + x if k % 2 == 0 else 1.0 - x for k in range(r)]))


content = [synthetic.image(H >> l, W >> l, seed=1) for l in range(NLEV)]
style = [synthetic.image(HS >> l, WS >> l, seed=2) for l in range(NLEV)]
x = prep((0.6 * content[0] + 0.4 * synthetic.image(H, W, seed=9)).astype(np.float32))


def closure(name, prepare=None, guided=False, **options):
    e = StyleEngine(WEIGHTS, 0, batched=False, **options)
    try:
        e.configure(NLEV, H, W)
        if prepare:
            prepare(e)
        for l in range(NLEV):
            if guided:          # (the levels of one closure are all guided or all unguided)
                e.set_guidance(l, ramps(2, H >> l, W >> l))
                e.set_targets_guided(l, prep(content[l]), prep(style[l]), ramps(2, HS >> l, WS >> l))
            else:
                e.set_targets(l, prep(content[l]), prep(style[l]))
        g, rows = e.closure(x, CW, SW, TVW)
        torch.cuda.synchronize()
        digest(name, g, rows)
    finally:
        e.close()


closure("per-level closure")
closure("per-level closure, 16-row bands", h2_band_rows=16)
closure("per-level closure, guided level R=2", guided=True)
closure("per-level closure, centred Gram shift", prepare=lambda e: e.set_gram_shift("mean"))
closure("per-level closure, Gram shift 0.5", prepare=lambda e: e.set_gram_shift(0.5))
closure("per-level closure, moments", prepare=lambda e: e.set_moments(1e3, 1e3))

e = StyleEngine(WEIGHTS, 0)
try:
    feats = e.vgg_features(x)
    torch.cuda.synchronize()
    digest("vgg_features", *feats)
    gen = torch.Generator().manual_seed(3)
    gouts = [dev(torch.randn(f.shape, generator=gen)) for f in feats]
    digest("vgg_features_backward", e.vgg_features_backward(x, gouts))
    for c, hh, ww in ((64, 70, 52), (256, 35, 27)):
        f = dev(torch.randn((1, c, hh, ww), generator=gen).abs())
        tag = f"C={c} {hh}x{ww}"
        digest(f"gram {tag}", e.gram(f))
        digest(f"gram_shifted centred {tag}", *e.gram_shifted(f, center=True))
        digest(f"gram_shifted -0.25 {tag}", *e.gram_shifted(f, shift=-0.25))
        n = hh * ww
        fn = dev(f.reshape(c, n).t())
        planes = dev(torch.rand((2, n), generator=gen))
        s_mats = dev(torch.randn((2, c, c), generator=gen) * 1e-3)
        digest(f"guided_gram_backward {tag}", e.guided_gram_backward(fn, planes, s_mats))
    # the stripe closure: rows [16, 64) of a 96-row image, seen through an 80-row stripe
    e.configure(1, 80, 52)
    stripe = synthetic.image(80, 52, seed=4)
    e.set_targets(0, prep(stripe), prep(style[0]))
    xs = prep((0.6 * stripe + 0.4 * synthetic.image(80, 52, seed=5)).astype(np.float32))
    digest("window_begin sums", e.window_begin(xs, 16, 48, 96))
finally:
    e.close()
