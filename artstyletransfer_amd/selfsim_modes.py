"""The self-similarity content term: the pattern of pairwise cosine distances between sampled positions of a tapped map must
be that of the content image's map - the content half of Kolkin, Salavon & Shakhnarovich, "Style Transfer by Relaxed Optimal
Transport and Self-Similarity" (STROTSS, CVPR 2019); see nst_level_set_selfsim in include/nst_hip.h.  The one normaliser of
the term (neural_style_transfer_selfsim(), NeuralStyleTransfer.set_self_similarity, StyleEngine.set_selfsim), kept free of
torch: everything here raises ValueError before any GPU work."""
import math
import numbers

from . import map_term_modes as _terms
from .mrf_modes import MAP_SCALE
from .remd_modes import MAX_STRIDE, check_stride, check_strides, samples_of  # noqa: F401
from .taps import DEFAULT_CONTENT_INDEX, DEFAULT_STYLE_INDICES

DEFAULT_SAMPLES = 1024          # the paper's sample count: a setting, not a measurement
MAX_SAMPLES = 4096              # the term keeps n x n arrays
DEFAULT_EPSILON = 1e-5


def _words(content_index):
    # (map_term_modes says "<name>: <no_default> is <role> of the job <maps>" when a bare number finds none of default_maps)
    return _terms.words("selfsim_weight", "selfsim_levels", (content_index,), f"not even the content map (index {content_index})", "a map")


def check_samples(samples=DEFAULT_SAMPLES):
    if isinstance(samples, bool) or not isinstance(samples, numbers.Integral) or not 1 <= int(samples) <= MAX_SAMPLES:
        raise ValueError(f"selfsim_samples must be an integer 1..{MAX_SAMPLES}, not {samples!r}")
    return int(samples)


def check_epsilon(epsilon=DEFAULT_EPSILON):
    if isinstance(epsilon, bool) or not isinstance(epsilon, numbers.Real) or not math.isfinite(float(epsilon)) or not float(epsilon) > 0.0:
        raise ValueError(f"selfsim_epsilon must be a finite number > 0, not {epsilon!r}")
    return float(epsilon)


def stride_for(hm, wm, samples=DEFAULT_SAMPLES):
    """The smallest stride s >= 1 with samples_of(hm, wm, s) <= samples; ValueError if that needs s > 256."""
    samples = check_samples(samples)
    hm, wm = int(hm), int(wm)
    if hm < 1 or wm < 1:
        raise ValueError(f"a map of {hm}x{wm} has no samples")
    for s in range(1, MAX_STRIDE + 1):
        if samples_of(hm, wm, s) <= samples:
            return s
    raise ValueError(f"selfsim_samples={samples}: a map of {hm}x{wm} needs a stride above {MAX_STRIDE}")


def used_maps(content_index=None, style_indices=None):
    """The maps a job uses, or None when neither is known: its content map and its style maps."""
    if content_index is None and style_indices is None:
        return None
    content = DEFAULT_CONTENT_INDEX if content_index is None else int(content_index)
    style = DEFAULT_STYLE_INDICES if style_indices is None else style_indices
    return tuple(sorted({content} | {int(i) for i in style}))


def normalize_weights(value=None, content_index=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index (map_term_modes.normalize_weights has the forms of `value`); a plain number weighs the
    job's content map.  Unlike the style terms a weight may sit on any map the job uses: its content map or a style map."""
    content = DEFAULT_CONTENT_INDEX if content_index is None else int(content_index)
    used = used_maps(content_index, style_indices)
    if used is None and isinstance(value, numbers.Real) and not isinstance(value, bool):
        used = (content,)               # (a bare number on a job whose maps are not known yet: the content map is always one)
    return _terms.normalize_weights(_words(content), value, used, use_relu)


def normalize_levels(levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices (map_term_modes.normalize_levels)."""
    return _terms.normalize_levels(_words(DEFAULT_CONTENT_INDEX), levels, levels_num)


def normalize_selfsim(selfsim_weight=None, selfsim_samples=DEFAULT_SAMPLES, selfsim_epsilon=DEFAULT_EPSILON, selfsim_levels=None,
                      content_index=None, style_indices=None, use_relu=None, levels_num=None):
    """(weights, samples, epsilon, levels) - six weights by map index, the most samples per map, epsilon and the levels (None:
    all) - or None when the term is off (None, 0, all zeros).  Everything is validated, the off setting included."""
    samples = check_samples(selfsim_samples)
    eps = check_epsilon(selfsim_epsilon)
    levels = normalize_levels(selfsim_levels, levels_num)
    w = normalize_weights(selfsim_weight, content_index, style_indices, use_relu)
    if all(v == 0.0 for v in w):
        return None
    return w, samples, eps, levels


def check_exclusive(setting, regions=None, stripes: bool = False, extra_styles=None) -> None:
    """The term does not combine with several style images, with spatial control (guided levels) or with stripe sharding."""
    _terms.check_exclusive(_words(DEFAULT_CONTENT_INDEX), setting, regions, stripes, extra_styles)


def level_strides(setting, level_shapes):
    """Per level of the job, None (the level does not carry the term) or six strides by map index: stride_for() of the weighted
    maps (1 for the others).  `level_shapes`: (h, w) of the level image, in StyleEngine's numbering; a map of index i has
    (h >> MAP_SCALE[i]) x (w >> MAP_SCALE[i]) pixels.  ValueError when a level lies outside the job, a weighted map pools to
    nothing, or a map needs a stride above 256."""
    if setting is None:
        return [None] * len(level_shapes)
    w, samples, _, levels = setting
    for lv in (() if levels is None else levels):
        if lv >= len(level_shapes):
            raise ValueError(f"selfsim_levels: level {lv} is outside the job's {len(level_shapes)} levels")
    out = []
    for lv, (h, ww) in enumerate(level_shapes):
        if levels is not None and lv not in levels:
            out.append(None)
            continue
        row = []
        for i, wi in enumerate(w):
            if not wi > 0.0:
                row.append(1)
                continue
            hm, wm = int(h) >> MAP_SCALE[i], int(ww) >> MAP_SCALE[i]
            if hm < 1 or wm < 1:
                raise ValueError(f"selfsim_weight: map {i} of level {lv} ({h}x{ww}) pools to nothing")
            row.append(stride_for(hm, wm, samples))
        out.append(tuple(row))
    return out
