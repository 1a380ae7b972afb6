"""Generate tests/golden/pool_avg_*.npz by running the REFERENCE's Vgg19 / LossBuilder / prepare_img, unmodified, on a network
whose pooling layers were swapped: every torch.nn.MaxPool2d child of the constructed network's six slices is replaced by
torch.nn.AvgPool2d(kernel_size=2, stride=2) - the customary way this switch is made in this family of code.

Run only in the build container (needs the reference tree, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fixtures_pool.py [--only NAME]

Same stand-ins, synthetic weights and pyramid rule as make_fixtures.py (imported from there).  The closure cases hold the
total, the per-level rows, the gradient of the weighted sum and the gradient of each term alone.  Fixtures hold data only.
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

# name -> (content index, style indices, use_relu, (h, w), levels, style size or None = the content's)
CASES = {
    "64x96_L1": (4, [0, 1, 2, 3, 5], True, (64, 96), 2, None),            # default taps, inputs of closure_64x96_L1
    "shallow_64x96_L1": (1, [0, 1], True, (64, 96), 2, None),             # truncated pass with one pool
    "prerelu_64x96_L1": (4, [0, 1, 2, 3, 5], False, (64, 96), 2, None),   # use_relu=False
    "50x76_L0": (4, [0, 1, 2, 3, 5], True, (50, 76), 1, (44, 58)),        # odd sizes: dropped last row / column (closure_50x76_L0)
}
WEIGHTS = ((1e3, 4e5, 1e2), {"c": (1e3, 0.0, 0.0), "s": (0.0, 4e5, 0.0), "tv": (0.0, 0.0, 1e2)})


def avg_pooled(net):
    """The network with every MaxPool2d child of its six slices replaced by AvgPool2d(2, 2)."""
    swapped = 0
    for k in range(1, 7):
        sl = getattr(net, f"slice{k}")
        for name, child in list(sl.named_children()):
            if isinstance(child, torch.nn.MaxPool2d):
                setattr(sl, name, torch.nn.AvgPool2d(kernel_size=2, stride=2))
                swapped += 1
    assert swapped == 4, swapped
    return net


def _net(ref_nn, use_relu):
    with contextlib.redirect_stdout(io.StringIO()):
        return avg_pooled(ref_nn.Vgg19(requires_grad=False, show_progress=False, use_relu=use_relu).eval())


def _closure(ref_nn, ref_nst, cidx, sidx, use_relu, content_levels, style_levels, x_img, cw, sw, tvw):
    """Teacher-forced closure through the reference's LossBuilder on the avg-pool network (one call, no optimiser)."""
    net = _net(ref_nn, use_relu)
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
    cidx, sidx, use_relu, (h, w), nlev, style_hw = CASES[name]
    if nlev == 1:       # the inputs of closure_50x76_L0
        cl = [cpu_ref.synthetic_image(h, w, seed=1)]
        sl = [cpu_ref.synthetic_image(*style_hw, seed=2)]
        x_img = (0.5 * cl[0] + 0.5 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32)
    else:               # the inputs of closure_64x96_L1
        cl = _levels(h, w, nlev, seed=1)
        sl = _levels(h, w, nlev, seed=2)
        x_img = (0.6 * cl[0] + 0.4 * cpu_ref.synthetic_image(h, w, seed=9)).astype(np.float32)
    total, rows, grad = _closure(ref_nn, ref_nst, cidx, sidx, use_relu, cl, sl, x_img, *WEIGHTS[0])
    terms = {}
    for tag, wts in WEIGHTS[1].items():
        t, _, g = _closure(ref_nn, ref_nst, cidx, sidx, use_relu, cl, sl, x_img, *wts)
        terms[f"grad_{tag}"] = g
        terms[f"total_{tag}"] = np.float64(t)
    images = {}
    for i in range(nlev):
        images[f"content{i}"] = cl[i]
        images[f"style{i}"] = sl[i]
    save(f"pool_avg_{name}", x_img=x_img, content_index=np.int64(cidx), style_indices=np.array(sidx, dtype=np.int64),
         use_relu=np.int64(use_relu), levels=np.int64(nlev), total=np.float64(total), rows=rows, grad=grad, **images, **terms)


def fx_vgg(ref_nn, ref_nst):
    """The avg-pool Vgg19 forward on the (1,3,48,80) input of vgg_48x80: the six maps (summaries as there, the two
    smallest whole)."""
    net = _net(ref_nn, True)
    img = cpu_ref.synthetic_image(48, 80, seed=3)
    x = ref_nst.prepare_img(img, "cpu")
    with torch.no_grad():
        outs = net(x)
    arrays = {"img": img, "layer_names": np.array(list(net.layer_names))}
    for i, o in enumerate(outs):
        arrays[f"out{i}"] = summarize(o, seed=100 + i)
    arrays["out5_full"] = outs[5].numpy()
    arrays["out4_full"] = outs[4].numpy()
    save("pool_avg_vgg_48x80", **arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    weights = cpu_ref.synthetic_vgg19_weights(bias_std=cpu_ref.TEST_BIAS_STD)     # as make_fixtures.py
    install_standins(weights)
    _, ref_nn, ref_nst = import_reference()
    for name in list(CASES) + ["vgg_48x80"]:
        if args.only and name not in args.only:
            continue
        print(f"== {name}")
        if name == "vgg_48x80":
            fx_vgg(ref_nn, ref_nst)
        else:
            fx_case(name, ref_nn, ref_nst)


if __name__ == "__main__":
    main()
