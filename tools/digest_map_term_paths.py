"""GPU: a sha256 per case of what the closure makes of the per-map terms (MRF, histogram loss, relaxed EMD) - over two
consecutive closures the gradient, the loss rows, patch_losses(), histogram_losses(), remd_losses() and the launch record
(nst_last_closure_launches: class, tags and kernel shapes in launch order; it holds no times).  The cases, all on a synthetic
64x96 two-level job and each on the batched and on the per-level engine: the default taps with the terms on maps 2 and 3;
taps (4, 0x3F) with all three on map 4, the content map; taps (2, {0,1,2,3}) with all three on map 3, the top of the chain;
average pooling with luminance; the terms on level 1 only (on the batched engine also each level mask alone and the two
halves); the MRF term with semantic guidance, R = 2.  Two builds compute the same when every line agrees - run it under both
in one visit of one box and compare:
    python tools/digest_map_term_paths.py > a.txt;  NST_LIB=/path/to/other/libnst_hip.so python tools/digest_map_term_paths.py > b.txt
(the digests are not goldens: they depend on the build)."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from artstyletransfer_amd import synthetic
from artstyletransfer_amd.engine import StyleEngine

CW, SW, TVW = 1e3, 4e5, 1e2
H, W, HS, WS = 64, 96, 70, 110
W_MRF, W_HIST, W_REMD = (0, 0, 400.0, 200.0, 0, 0), (0, 0, 0, 5000.0, 0, 0), (0, 0, 7e4, 7e4, 0, 0)


def on_map(i, v):
    return tuple(v if k == i else 0.0 for k in range(6))


def images(channels):
    """(content, style) per level and the start image, prepared: RGB, or one plane 255 Y in luminance mode."""
    def prep(e, a):
        t = e.prepare_img(torch.from_numpy(a).cuda())
        return t if channels == 3 else (t * torch.tensor([0.299, 0.587, 0.114], device="cuda").view(1, 3, 1, 1)).sum(1, keepdim=True) + 110.0
    return lambda e: ([(prep(e, synthetic.image(H >> l, W >> l, 1 + l)), prep(e, synthetic.image(HS >> l, WS >> l, 11 + l))) for l in range(2)],
                      prep(e, synthetic.image(H, W, 21)))


def bands(r, h, w):
    label = np.arange(w) * r // w
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(label[None, None, :] == np.arange(r)[:, None, None], (r, h, w)),
                                                 dtype=np.float32)).cuda()


def digest(name, e, x, run):
    h = hashlib.sha256()
    e.set_timing(2)
    for _ in range(2):
        for t in run(e, x):
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
        for t in (e.patch_losses(), e.histogram_losses(), e.remd_losses()):
            h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
        h.update(repr([sorted(d.items()) for d in e.last_closure_launches()]).encode())
    e.set_timing(0)
    print(f"{name:88s} {h.hexdigest()}", flush=True)


def whole(e, x):
    return e.closure(x, CW, SW, TVW)


def masked(mask):
    return lambda e, x: e.closure_levels(x, CW, SW, TVW, mask)


def halves(e, x):
    losses = e.closure_forward(x, CW, SW, TVW)
    return e.closure_backward(x, CW, SW, TVW), losses


def case(name, e, taps=None, pooling=None, luminance=False, mrf=None, hist=None, remd=None, levels=(0, 1), guided=0, runs=None):
    e.configure(2, H, W)
    try:
        if taps:
            e.set_taps(*taps)
        if pooling:
            e.set_pooling(pooling)
        if luminance:
            e.set_color("luminance")
        lv, x = images(1 if luminance else 3)(e)
        for l, (c, s) in enumerate(lv):
            e.set_targets(l, c, s)
        for l in levels:
            s = lv[l][1]
            if mrf:
                e.set_patches(l, s, mrf, 1)
                if guided:
                    e.set_patch_guidance(l, bands(guided, H >> l, W >> l), bands(guided, HS >> l, WS >> l), 2.0)
            if hist:
                e.set_histograms(l, s, hist)
            if remd:
                e.set_remd(l, s, remd, 1, 1)
        for what, run in (runs or {"closure": whole}).items():
            digest(f"{name}: {what}", e, x, run)
    finally:
        e.reset_job_settings()


weights = synthetic.vgg19_weights(bias_std=2.0)
for walker, batched in (("batched", True), ("per-level", False)):
    e = StyleEngine(weights, 0, batched=batched)
    try:
        case(f"{walker}, default taps, MRF 2+3, hist 3, EMD 2+3", e, mrf=W_MRF, hist=W_HIST, remd=W_REMD)
        case(f"{walker}, taps (4, 0x3F), all three on map 4 (content)", e, taps=(4, [0, 1, 2, 3, 4, 5]),
             mrf=on_map(4, 200.0), hist=on_map(4, 5000.0), remd=on_map(4, 7e4))
        case(f"{walker}, taps (2, 0..3), all three on map 3 (top)", e, taps=(2, [0, 1, 2, 3]),
             mrf=on_map(3, 200.0), hist=on_map(3, 5000.0), remd=on_map(3, 7e4))
        case(f"{walker}, avg pooling + luminance, all three", e, pooling="avg", luminance=True, mrf=W_MRF, hist=W_HIST, remd=W_REMD)
        runs = {"closure": whole}
        if batched:
            runs.update({"level mask 1": masked(1), "level mask 2": masked(2), "forward + backward halves": halves})
        case(f"{walker}, terms on level 1 only", e, mrf=W_MRF, hist=W_HIST, remd=W_REMD, levels=(1,), runs=runs)
        case(f"{walker}, MRF with semantic guidance, R = 2", e, mrf=W_MRF, guided=2)
    finally:
        e.close()
