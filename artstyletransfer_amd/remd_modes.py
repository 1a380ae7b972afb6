"""The relaxed EMD style term: two-way nearest-neighbour matching, by cosine, of the feature vectors of a tapped map and of
the style's map, both sampled on a stride grid - Kolkin, Salavon & Shakhnarovich, "Style Transfer by Relaxed Optimal Transport
and Self-Similarity" (STROTSS, CVPR 2019); see nst_level_set_remd in include/nst_hip.h.  The one normaliser of the term
(neural_style_transfer_remd(), NeuralStyleTransfer.set_relaxed_emd, StyleEngine.set_remd), kept free of torch: everything
here raises ValueError before any GPU work."""
import math
import numbers

from . import map_term_modes as _terms
from .map_term_modes import MAX_LEVELS, _weight  # noqa: F401
from .mrf_modes import MAP_SCALE
from .taps import NUM_MAPS

DEFAULT_SAMPLES = 4096          # a setting, not a measurement: the search costs n m C, so cost grows with its square
DEFAULT_EPSILON = 1e-5
MAX_STRIDE = 256
DEFAULT_MAPS = (1, 2, 3)        # relu2_1, relu3_1 and relu4_1: what a plain number weighs
_WORDS = _terms.words("remd_weight", "remd_levels", DEFAULT_MAPS, "none of relu2_1, relu3_1, relu4_1 (indices 1, 2, 3)")


def check_samples(samples=DEFAULT_SAMPLES):
    if isinstance(samples, bool) or not isinstance(samples, numbers.Integral) or int(samples) < 1:
        raise ValueError(f"remd_samples must be an integer >= 1, not {samples!r}")
    return int(samples)


def check_epsilon(epsilon=DEFAULT_EPSILON):
    if isinstance(epsilon, bool) or not isinstance(epsilon, numbers.Real) or not math.isfinite(float(epsilon)) or not float(epsilon) > 0.0:
        raise ValueError(f"remd_epsilon must be a finite number > 0, not {epsilon!r}")
    return float(epsilon)


def check_stride(stride, what="stride"):
    if isinstance(stride, bool) or not isinstance(stride, numbers.Integral) or not 1 <= int(stride) <= MAX_STRIDE:
        raise ValueError(f"{what} must be an integer 1..{MAX_STRIDE}, not {stride!r}")
    return int(stride)


def check_strides(strides, what="strides"):
    """Six strides by map index: one integer 1..256 for all, or six of them."""
    if isinstance(strides, numbers.Integral) and not isinstance(strides, bool):
        return (check_stride(strides, what),) * NUM_MAPS
    try:
        items = list(strides)
    except TypeError:
        raise ValueError(f"{what}: expected an integer or {NUM_MAPS} integers, got {strides!r}") from None
    if len(items) != NUM_MAPS:
        raise ValueError(f"{what}: expected {NUM_MAPS} integers (one per feature map), got {len(items)}")
    return tuple(check_stride(s, f"{what} entry {i}") for i, s in enumerate(items))


def samples_of(hm, wm, stride):
    """The number of samples of an hm x wm map on the stride grid: the pixels (a s, b s)."""
    return ((int(hm) - 1) // stride + 1) * ((int(wm) - 1) // stride + 1)


def stride_for(hm, wm, samples=DEFAULT_SAMPLES):
    """The smallest stride s >= 1 with samples_of(hm, wm, s) <= samples; ValueError if that needs s > 256."""
    samples = check_samples(samples)
    hm, wm = int(hm), int(wm)
    if hm < 1 or wm < 1:
        raise ValueError(f"a map of {hm}x{wm} has no samples")
    for s in range(1, MAX_STRIDE + 1):
        if samples_of(hm, wm, s) <= samples:
            return s
    raise ValueError(f"remd_samples={samples}: a map of {hm}x{wm} needs a stride above {MAX_STRIDE}")


def normalize_weights(value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index (map_term_modes.normalize_weights has the forms of `value`); a plain number weighs
    those of relu2_1, relu3_1 and relu4_1 - indices 1, 2, 3 - that are style maps of the job."""
    return _terms.normalize_weights(_WORDS, value, style_indices, use_relu)


def normalize_levels(levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices (map_term_modes.normalize_levels)."""
    return _terms.normalize_levels(_WORDS, levels, levels_num)


def normalize_remd(remd_weight=None, remd_samples=DEFAULT_SAMPLES, remd_epsilon=DEFAULT_EPSILON, remd_levels=None, style_indices=None,
                   use_relu=None, levels_num=None):
    """(weights, samples, epsilon, levels) - six weights by map index, the most samples per side and map, epsilon and the
    levels (None: all) - or None when the term is off (None, 0, all zeros).  Everything is validated, the off setting
    included."""
    samples = check_samples(remd_samples)
    eps = check_epsilon(remd_epsilon)
    levels = normalize_levels(remd_levels, levels_num)
    w = normalize_weights(remd_weight, style_indices, use_relu)
    if all(v == 0.0 for v in w):
        return None
    return w, samples, eps, levels


def check_exclusive(setting, regions=None, stripes: bool = False, extra_styles=None) -> None:
    """The term does not combine with several style images (the union of the styles' samples is a follow-up), with spatial
    control (guided levels) or with stripe sharding."""
    _terms.check_exclusive(_WORDS, setting, regions, stripes, extra_styles)


def level_strides(setting, level_shapes, style_shapes):
    """Per level of the job, None (the level does not carry the term) or (image strides, style strides): six each by map
    index, stride_for() of the weighted maps (1 for the others).  `level_shapes`, `style_shapes`: (h, w) of the level image and
    of the level's style image, in StyleEngine's numbering; a map of index i has (h >> MAP_SCALE[i]) x (w >> MAP_SCALE[i])
    pixels.  ValueError when a level lies outside the job, a weighted map pools to nothing, or a map needs a stride above
    256."""
    if setting is None:
        return [None] * len(level_shapes)
    w, samples, _, levels = setting
    for lv in (() if levels is None else levels):
        if lv >= len(level_shapes):
            raise ValueError(f"remd_levels: level {lv} is outside the job's {len(level_shapes)} levels")
    out = []
    for lv, (shape, sshape) in enumerate(zip(level_shapes, style_shapes)):
        if levels is not None and lv not in levels:
            out.append(None)
            continue
        strides = []
        for what, (h, ww) in (("image", shape), ("style image", sshape)):
            row = []
            for i, wi in enumerate(w):
                if not wi > 0.0:
                    row.append(1)
                    continue
                hm, wm = int(h) >> MAP_SCALE[i], int(ww) >> MAP_SCALE[i]
                if hm < 1 or wm < 1:
                    raise ValueError(f"remd_weight: map {i} of the {what} of level {lv} ({h}x{ww}) pools to nothing")
                row.append(stride_for(hm, wm, samples))
            strides.append(tuple(row))
        out.append((strides[0], strides[1]))
    return out
