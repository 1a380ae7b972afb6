"""The long-range style term ("xcorr"): the cross-correlation of a tapped map with a spatially shifted copy of itself,
G_d = sum_p F(p + d) F(p)^T, is held to the style's for a handful of shifts d beside the ordinary Gram matrix - Berger &
Memisevic, "Incorporating Long-Range Consistency in CNN-based Texture Generation" (ICLR 2017); see nst_level_set_xcorr in
include/nst_hip.h.  (The name "Gram shift" is taken by the activation shift of gram_modes.)  The one normaliser of the term
(neural_style_transfer_xcorr(), NeuralStyleTransfer.set_shifted_gram, StyleEngine.set_xcorr), kept free of torch: everything
here raises ValueError before any GPU work."""
import numbers

from . import map_term_modes as _terms
from .mrf_modes import MAP_SCALE

DEFAULT_SHIFTS = (2, 4, 8)      # a setting, not a measurement: the axis shifts by 2, 4 and 8 map pixels
MAX_SHIFT = 64
MAX_SHIFTS = 16                 # after expansion
DEFAULT_MAPS = (1, 2, 3)        # relu2_1, relu3_1 and relu4_1: what a plain number weighs
_WORDS = _terms.words("xcorr_weight", "xcorr_levels", DEFAULT_MAPS, "none of relu2_1, relu3_1, relu4_1 (indices 1, 2, 3)")


def _component(v, item):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) <= MAX_SHIFT:
        raise ValueError(f"xcorr_shifts: {item!r} is not an integer 0..{MAX_SHIFT} or a pair (dx, dy) of them")
    return int(v)


def normalize_shifts(shifts=DEFAULT_SHIFTS):
    """The tuple of distinct shifts (dx, dy), dx, dy in 0..64 and not both 0, at most 16 of them.  `shifts`: a collection whose
    items are an int k >= 1 - the two axis shifts (k, 0) and (0, k) - or a pair (dx, dy), which passes through; a lone int is a
    collection of one."""
    if isinstance(shifts, numbers.Integral) and not isinstance(shifts, bool):
        shifts = (shifts,)
    if shifts is None or isinstance(shifts, (str, bytes, dict, set, frozenset, bool, numbers.Number)):
        raise ValueError(f"xcorr_shifts: expected a collection of integers or (dx, dy) pairs, got {shifts!r}")
    try:
        items = list(shifts)
    except TypeError:
        raise ValueError(f"xcorr_shifts: expected a collection of integers or (dx, dy) pairs, got {shifts!r}") from None
    out = []
    for item in items:
        if isinstance(item, numbers.Integral) and not isinstance(item, bool):
            k = _component(item, item)
            new = [(k, 0), (0, k)]
        else:
            if isinstance(item, (str, bytes, dict, set, frozenset, bool, numbers.Number)) or item is None:
                raise ValueError(f"xcorr_shifts: {item!r} is not an integer 0..{MAX_SHIFT} or a pair (dx, dy) of them")
            try:
                pair = list(item)
            except TypeError:
                raise ValueError(f"xcorr_shifts: {item!r} is not an integer 0..{MAX_SHIFT} or a pair (dx, dy) of them") from None
            if len(pair) != 2:
                raise ValueError(f"xcorr_shifts: {item!r} is not an integer 0..{MAX_SHIFT} or a pair (dx, dy) of them")
            new = [(_component(pair[0], item), _component(pair[1], item))]
        for d in new:
            if d == (0, 0):
                raise ValueError(f"xcorr_shifts: {item!r} is the zero shift (that statistic is the Gram matrix)")
            if d in out:
                raise ValueError(f"xcorr_shifts: the shift {d} appears twice")
            out.append(d)
    if not out:
        raise ValueError("xcorr_shifts: the collection is empty")
    if len(out) > MAX_SHIFTS:
        raise ValueError(f"xcorr_shifts: {len(out)} shifts after expansion, at most {MAX_SHIFTS}")
    return tuple(out)


def normalize_weights(value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index (map_term_modes.normalize_weights has the forms of `value`); a plain number weighs
    those of relu2_1, relu3_1 and relu4_1 - indices 1, 2, 3 - that are style maps of the job."""
    return _terms.normalize_weights(_WORDS, value, style_indices, use_relu)


def normalize_levels(levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices (map_term_modes.normalize_levels)."""
    return _terms.normalize_levels(_WORDS, levels, levels_num)


def normalize_xcorr(xcorr_weight=None, xcorr_shifts=DEFAULT_SHIFTS, xcorr_levels=None, style_indices=None, use_relu=None, levels_num=None):
    """(weights, shifts, levels) - six weights by map index, the expanded shifts and the levels (None: all) - or None when the
    term is off (None, 0, all zeros).  Everything is validated, the off setting included."""
    shifts = normalize_shifts(xcorr_shifts)
    levels = normalize_levels(xcorr_levels, levels_num)
    w = normalize_weights(xcorr_weight, style_indices, use_relu)
    if all(v == 0.0 for v in w):
        return None
    return w, shifts, levels


def check_exclusive(setting, regions=None, stripes: bool = False, extra_styles=None) -> None:
    """The term does not combine with several style images, with spatial control (guided levels) or with stripe sharding."""
    _terms.check_exclusive(_WORDS, setting, regions, stripes, extra_styles)


def check_map(hm, wm, shifts, what="map"):
    """ValueError unless every shift leaves a pair on an hm x wm map: dx < wm and dy < hm."""
    for dx, dy in shifts:
        if dx >= int(wm) or dy >= int(hm):
            raise ValueError(f"xcorr_shifts: the shift ({dx}, {dy}) is not smaller than the {what} ({hm}x{wm})")


def level_carries(setting, level_shapes, style_shapes):
    """Per level of the job, whether it carries the term.  `level_shapes`, `style_shapes`: (h, w) of the level image and of the
    level's style image, in StyleEngine's numbering; a map of index i has (h >> MAP_SCALE[i]) x (w >> MAP_SCALE[i]) pixels.
    ValueError when a level lies outside the job, or a shift is not smaller than a weighted map of a carrying level, of either
    image."""
    if setting is None:
        return [False] * len(level_shapes)
    w, shifts, levels = setting
    for lv in (() if levels is None else levels):
        if lv >= len(level_shapes):
            raise ValueError(f"xcorr_levels: level {lv} is outside the job's {len(level_shapes)} levels")
    out = []
    for lv, (shape, sshape) in enumerate(zip(level_shapes, style_shapes)):
        on = levels is None or lv in levels
        out.append(on)
        if not on:
            continue
        for what, (h, ww) in (("image", shape), ("style image", sshape)):
            for i, wi in enumerate(w):
                if wi > 0.0:
                    check_map(int(h) >> MAP_SCALE[i], int(ww) >> MAP_SCALE[i], shifts, f"map {i} of the {what} of level {lv}")
    return out
