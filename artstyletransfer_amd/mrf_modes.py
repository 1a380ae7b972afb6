"""The MRF style term: every 3x3 patch of a feature map pulled towards its nearest neighbour among the style's patches of
the same map - Li & Wand, "Combining Markov Random Fields and Convolutional Neural Networks for Image Synthesis" (CVPR
2016), the loss of CNNMRF and neural-doodle; see nst_level_set_patches in include/nst_hip.h.  The one normaliser of the
term (neural_style_transfer_mrf(), NeuralStyleTransfer.set_patch_match, StyleEngine.set_patches), kept free of torch:
everything here raises ValueError before any GPU work."""
import math
import numbers

from . import map_term_modes as _terms
from .map_term_modes import MAX_LEVELS, _weight  # noqa: F401

DEFAULT_EPSILON = 1e-5
DEFAULT_STRIDE = 1
MAX_STRIDE = 8
LI_WAND_MAPS = (2, 3)           # relu3_1 and relu4_1: the layers of the paper
MAP_SCALE = (0, 1, 2, 3, 3, 4)  # log2 of the spatial divisor of each map
MIN_MAP = 3                     # a map below 3x3 has no patch
_WORDS = _terms.words("mrf_weight", "mrf_levels", LI_WAND_MAPS, "neither relu3_1 nor relu4_1 (indices 2 and 3)")


def check_epsilon(epsilon=DEFAULT_EPSILON):
    if isinstance(epsilon, bool) or not isinstance(epsilon, numbers.Real):
        raise ValueError(f"mrf_epsilon must be a finite number > 0, not {epsilon!r}")
    e = float(epsilon)
    if not math.isfinite(e) or not e > 0.0:
        raise ValueError(f"mrf_epsilon must be a finite number > 0, not {epsilon!r}")
    return e


def check_stride(stride=DEFAULT_STRIDE):
    if isinstance(stride, bool) or not isinstance(stride, numbers.Integral) or not 1 <= int(stride) <= MAX_STRIDE:
        raise ValueError(f"mrf_stride must be an integer 1..{MAX_STRIDE}, not {stride!r}")
    return int(stride)


def normalize_weights(value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index (map_term_modes.normalize_weights has the forms of `value`); a plain number weighs
    those of relu3_1 and relu4_1 - indices 2 and 3, Li & Wand's layers - that are style maps of the job."""
    return _terms.normalize_weights(_WORDS, value, style_indices, use_relu)


def normalize_levels(levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices (map_term_modes.normalize_levels)."""
    return _terms.normalize_levels(_WORDS, levels, levels_num)


def normalize_mrf(mrf_weight=None, mrf_stride=DEFAULT_STRIDE, mrf_epsilon=DEFAULT_EPSILON, mrf_levels=None, style_indices=None,
                  use_relu=None, levels_num=None):
    """(weights, stride, epsilon, levels) - six weights by map index, the style stride, epsilon and the levels (None: all) -
    or None when the term is off (None, 0, all zeros).  Everything is validated, the off setting included."""
    stride = check_stride(mrf_stride)
    eps = check_epsilon(mrf_epsilon)
    levels = normalize_levels(mrf_levels, levels_num)
    w = normalize_weights(mrf_weight, style_indices, use_relu)
    if all(v == 0.0 for v in w):
        return None
    return w, stride, eps, levels


def check_exclusive(setting, regions=None, stripes: bool = False, extra_styles=None) -> None:
    """The term does not combine with several style images (the union of dictionaries is a follow-up), with spatial
    control (guided levels) or with stripe sharding."""
    _terms.check_exclusive(_WORDS, setting, regions, stripes, extra_styles)


def check_sizes(setting, level_shapes, style_shapes) -> None:
    """Every weighted map is at least 3x3 on every chosen level, on the level image and on the level's style image.
    `level_shapes`, `style_shapes`: (h, w) per level, in StyleEngine's numbering."""
    if setting is None:
        return
    w, _, _, levels = setting
    for lv in (range(len(level_shapes)) if levels is None else levels):
        if lv >= len(level_shapes):
            raise ValueError(f"mrf_levels: level {lv} is outside the job's {len(level_shapes)} levels")
        for i, wi in enumerate(w):
            if not wi > 0.0:
                continue
            for what, (h, ww) in (("image", level_shapes[lv]), ("style image", style_shapes[lv])):
                if (int(h) >> MAP_SCALE[i]) < MIN_MAP or (int(ww) >> MAP_SCALE[i]) < MIN_MAP:
                    raise ValueError(f"mrf_weight: map {i} of the {what} of level {lv} ({h}x{ww}) pools below {MIN_MAP}x{MIN_MAP}")


DEFAULT_SEMANTIC_WEIGHT = 1.0


def normalize_semantic(content=None, style=None, weight=DEFAULT_SEMANTIC_WEIGHT):
    """The semantic maps that steer the patch search (neural-doodle; nst_level_set_patch_guidance in include/nst_hip.h) ->
    (content stack (R,H,W), style stack (R,Hs,Ws), weight), float32 stacks as regions.normalize_regions makes them, or None
    when off: both maps None, or a weight of 0.  Each map is an integer label map (H,W) with labels 0..R-1 or a float stack
    (R,H,W) in [0,1], at any resolution.  Everything is validated, the off setting included.
    ValueError for a malformed map, one map without the other, mismatched R, or a weight that is not a finite number >= 0."""
    from . import regions as _regions
    w = _weight(weight, "semantic_weight")
    if content is None and style is None:
        return None
    if content is None or style is None:
        raise ValueError("semantic_content and semantic_style go together: one was given without the other")
    c = _regions.normalize_regions(content, "semantic_content")
    s = _regions.normalize_regions(style, "semantic_style")
    if c.shape[0] != s.shape[0]:
        raise ValueError(f"semantic_content has {c.shape[0]} regions, semantic_style {s.shape[0]}")
    if w == 0.0:
        return None
    return c, s, w


def semantic_level_planes(setting, level_shapes, style_shapes, levels=None):
    """The stacks of normalize_semantic resized (regions.resize_nearest) to every chosen level of each pyramid: a list, by
    level, of (content planes (R,h,w), style planes (R,hs,ws)) or None for a level that does not carry the term."""
    from . import regions as _regions
    c, s, _ = setting
    out = []
    for lv, ((h, w), (hs, ws)) in enumerate(zip(level_shapes, style_shapes)):
        if levels is not None and lv not in levels:
            out.append(None)
        else:
            out.append((_regions.resize_nearest(c, int(h), int(w)), _regions.resize_nearest(s, int(hs), int(ws))))
    return out
