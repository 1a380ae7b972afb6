"""Generate tests/golden/taps_*.npz by running the REFERENCE's LossBuilder / Vgg19 with feature maps other than its
default ones (content_feature_maps_index, style_feature_maps_indices, Vgg19(use_relu=...)).

Run only in the build container (needs the reference tree, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fixtures_taps.py [--only NAME]

Same stand-ins, synthetic weights and pyramid rule as make_fixtures.py (imported from there).  Every closure case is a
2-level 64x96 pyramid with the inputs of closure_64x96_L1 and holds the total, the per-level rows, the gradient of the
weighted sum and the gradient of each term alone.  Fixtures hold data only.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_fixtures import _levels, cpu_ref, import_reference, install_standins, save, summarize  # noqa: E402

# name -> (content index, style indices, use_relu)
CASES = {
    "shallow": (1, [0, 1], True),           # (a) deepest map relu2_1: forward / backward truncated at conv2_1
    "same": (2, [2, 3], True),              # (b) content and Gram on relu3_1
    "c5s4": (5, [4], True),                 # (c) Gram of conv4_2, content at relu5_1
    "prerelu": (4, [0, 1, 2, 3, 5], False),  # (d) use_relu=False: map 5 is conv5_1 before its ReLU
    "c0s3": (0, [3], True),                 # (e) content on relu1_1: injected into conv1_2's input-gradient launch
}
WEIGHTS = ((1e3, 4e5, 1e2), {"c": (1e3, 0.0, 0.0), "s": (0.0, 4e5, 0.0), "tv": (0.0, 0.0, 1e2)})


def _closure(ref_nn, ref_nst, cidx, sidx, use_relu, content_levels, style_levels, x_img, cw, sw, tvw):
    """Teacher-forced closure through the reference's LossBuilder with the given taps (one call, no optimiser)."""
    with contextlib.redirect_stdout(io.StringIO()):
        net = ref_nn.Vgg19(requires_grad=False, show_progress=False, use_relu=use_relu).eval()
    builders = [ref_nst.LossBuilder(cidx, sidx, ref_nst.prepare_img(c, "cpu"), ref_nst.prepare_img(s, "cpu"),
                                    net, cw, sw, tvw) for c, s in zip(content_levels, style_levels)]
    x = ref_nst.prepare_img(x_img, "cpu").requires_grad_(True)
    levels, total, rows = [x], None, []
    for i, b in enumerate(builders):
        if i > 0:
            p = levels[i - 1]
            levels.append(torch.nn.functional.interpolate(p, size=(p.shape[2] // 2, p.shape[3] // 2), mode="bicubic"))
        t, c, s, tv = b.build(levels[i])
        total = t if total is None else 1.0 * total + t
        rows.append([float(t), float(c), float(s), float(tv)])
    total.backward()
    return float(total), np.array(rows, dtype=np.float64), x.grad.detach().numpy()


def fx_case(name, ref_nn, ref_nst):
    cidx, sidx, use_relu = CASES[name]
    cl = _levels(64, 96, 2, seed=1)
    sl = _levels(64, 96, 2, seed=2)
    x_img = (0.6 * cl[0] + 0.4 * cpu_ref.synthetic_image(64, 96, seed=9)).astype(np.float32)
    total, rows, grad = _closure(ref_nn, ref_nst, cidx, sidx, use_relu, cl, sl, x_img, *WEIGHTS[0])
    terms = {}
    for tag, wts in WEIGHTS[1].items():
        t, _, g = _closure(ref_nn, ref_nst, cidx, sidx, use_relu, cl, sl, x_img, *wts)
        terms[f"grad_{tag}"] = g
        terms[f"total_{tag}"] = np.float64(t)
    save(f"taps_{name}_64x96_L1", content0=cl[0], content1=cl[1], style0=sl[0], style1=sl[1], x_img=x_img,
         content_index=np.int64(cidx), style_indices=np.array(sidx, dtype=np.int64), use_relu=np.int64(use_relu),
         total=np.float64(total), rows=rows, grad=grad, **terms)


def fx_vgg_prerelu(ref_nn, ref_nst):
    """Vgg19(use_relu=False) forward on a (1,3,48,80) input: its attributes and the six maps (summaries; the small
    conv5_1 map whole, its negative entries included)."""
    with contextlib.redirect_stdout(io.StringIO()):
        net = ref_nn.Vgg19(requires_grad=False, show_progress=False, use_relu=False).eval()
    img = cpu_ref.synthetic_image(48, 80, seed=3)
    x = ref_nst.prepare_img(img, "cpu")
    with torch.no_grad():
        outs = net(x)
    arrays = {"img": img, "layer_names": np.array(list(net.layer_names)), "offset": np.int64(net.offset),
              "content_index": np.int64(net.content_feature_maps_index),
              "style_indices": np.array(net.style_feature_maps_indices, dtype=np.int64),
              "fields": np.array(list(type(outs)._fields))}
    for i, o in enumerate(outs):
        arrays[f"out{i}"] = summarize(o, seed=100 + i)
        arrays[f"min{i}"] = np.float64(o.min())
    arrays["out5_full"] = outs[5].numpy()
    save("taps_vgg_prerelu_48x80", **arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    weights = cpu_ref.synthetic_vgg19_weights(bias_std=cpu_ref.TEST_BIAS_STD)     # as make_fixtures.py
    install_standins(weights)
    _, ref_nn, ref_nst = import_reference()
    for name in list(CASES) + ["vgg_prerelu"]:
        if args.only and name not in args.only:
            continue
        print(f"== {name}")
        if name == "vgg_prerelu":
            fx_vgg_prerelu(ref_nn, ref_nst)
        else:
            fx_case(name, ref_nn, ref_nst)


if __name__ == "__main__":
    main()
