"""Per-layer style weights (the w_l of Gatys, Ecker & Bethge 2016) and the blend of several style images (jcjohnson's
-style_blend_weights; per map, the scale control of Gatys et al. 2017, "Controlling Perceptual Factors in Neural Style
Transfer"): validation and normalisation, kept free of torch so that config.py can validate with them.  include/nst_hip.h
has the definitions (nst_job_set_style_weights, nst_level_set_targets_blend); map indices are Vgg19.layer_names', 0..5."""
from __future__ import annotations

import math

import numpy as np

from .taps import DEFAULT_STYLE_INDICES, NUM_MAPS, map_index

MAX_STYLES = 8            # NST_MAX_STYLES
UNIT_WEIGHTS = (1.0,) * NUM_MAPS
_NO_INDEX = f"style layer weights: expected a map index 0..{NUM_MAPS - 1} or a name, got {{key!r}}"
_MAP_TEXTS = ("style layer weights: {key!r} is not a feature map name", _NO_INDEX, _NO_INDEX)


def _weight(v, what):
    if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what}: expected a number, got {v!r}")
    v = float(v)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"{what}: {v!r} is not a finite number >= 0")
    if v > 0.0 and np.float32(v) == 0.0 or not math.isfinite(float(np.float32(v))):
        raise ValueError(f"{what}: {v!r} is not representable in float32")
    return v


def check_style_layer_weights(weights, style_indices=None, use_relu=None):
    """The six layer weights as a tuple of floats from a sequence of 6 numbers or a dict {map index or name: weight}
    (maps not named get 1); None = all ones.  ValueError for a wrong length, a negative or non-finite entry, an unknown
    key, or when no map of `style_indices` (None: the reference's style set) has a positive weight."""
    if weights is None:
        return UNIT_WEIGHTS
    if isinstance(weights, dict):
        w = list(UNIT_WEIGHTS)
        for key, v in weights.items():
            w[map_index(key, use_relu, _MAP_TEXTS)] = _weight(v, f"style layer weight of {key!r}")
    else:
        if isinstance(weights, (str, bytes)) or not hasattr(weights, "__len__"):
            raise ValueError(f"style layer weights: expected {NUM_MAPS} numbers or a dict, got {weights!r}")
        if len(weights) != NUM_MAPS:
            raise ValueError(f"style layer weights: expected {NUM_MAPS} numbers (one per feature map), got {len(weights)}")
        w = [_weight(v, f"style layer weight {i}") for i, v in enumerate(weights)]
    style = DEFAULT_STYLE_INDICES if style_indices is None else tuple(style_indices)
    if not any(w[i] > 0.0 for i in style):
        raise ValueError(f"style layer weights: no map of the style set {list(style)} has a positive weight")
    return tuple(w)


def is_unit(weights) -> bool:
    return weights is None or tuple(float(v) for v in weights) == UNIT_WEIGHTS


def check_style_blend(blend, k, style_indices=None):
    """The K x 6 blend matrix (tuple of K tuples of 6 floats) of K style images from K numbers (the same weight on every
    map) or a K x 6 array; None = all ones (an even blend).  ValueError when K is not 1..MAX_STYLES or does not match
    `blend`, for a negative or non-finite entry, and when a map of `style_indices` (None: the reference's style set) has
    an all-zero column."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_STYLES:
        raise ValueError(f"style blend: the number of style images must be 1..{MAX_STYLES}, got {k!r}")
    k = int(k)
    if blend is None:
        rows = [[1.0] * NUM_MAPS for _ in range(k)]
    else:
        if isinstance(blend, (str, bytes, dict)) or not hasattr(blend, "__len__"):
            raise ValueError(f"style blend: expected {k} numbers or a {k} x {NUM_MAPS} array, got {blend!r}")
        if len(blend) != k:
            raise ValueError(f"style blend: {len(blend)} rows for {k} style image(s)")
        rows = []
        for r, row in enumerate(blend):
            if hasattr(row, "__len__") and not isinstance(row, (str, bytes)):
                if len(row) != NUM_MAPS:
                    raise ValueError(f"style blend: row {r} has {len(row)} entries, expected {NUM_MAPS}")
                rows.append([_weight(v, f"style blend [{r}][{i}]") for i, v in enumerate(row)])
            else:
                rows.append([_weight(row, f"style blend [{r}]")] * NUM_MAPS)
    style = DEFAULT_STYLE_INDICES if style_indices is None else tuple(style_indices)
    for i in style:
        if not sum(np.float32(row[i]) for row in rows) > 0.0:
            raise ValueError(f"style blend: no style image has a positive weight on map {i}")
    return tuple(tuple(row) for row in rows)


def normalized_blend(blend) -> np.ndarray:
    """b^[k][i] = B[k][i] / sum_k B[k][i] of a checked K x 6 matrix: fp64 quotients of the float32 entries, cast to
    float32 - what nst_level_set_targets_blend forms.  An all-zero column (a map outside the style set) stays zero."""
    b = np.asarray(blend, dtype=np.float32).astype(np.float64)
    col = b.sum(axis=0)
    return np.where(col > 0.0, b / np.where(col > 0.0, col, 1.0), 0.0).astype(np.float32)
