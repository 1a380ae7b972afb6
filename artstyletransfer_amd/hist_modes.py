"""The histogram loss: every channel of a tapped feature map remapped so that its histogram becomes the style's, and the map
pulled towards its remap - Risser, Wilmot & Barnes, "Stable and Controllable Neural Texture Synthesis and Style Transfer
Using Histogram Losses" (2017); see nst_level_set_histograms in include/nst_hip.h.  The one normaliser of the term
(neural_style_transfer_hist(), NeuralStyleTransfer.set_histogram_loss, StyleEngine.set_histograms), kept free of torch:
everything here raises ValueError before any GPU work."""
import math
import numbers

from .taps import DEFAULT_STYLE_INDICES, NUM_MAPS, map_index, map_index_texts

_MAP_TEXTS = map_index_texts("hist_weight")
DEFAULT_BINS = 256
MIN_BINS = 2
MAX_BINS = 1024
RISSER_MAPS = (0, 3)            # relu1_1 and relu4_1: the layers of the paper
MAX_LEVELS = 8


def _weight(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    w = float(v)
    if not math.isfinite(w) or w < 0.0:
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    return w


def check_bins(bins=DEFAULT_BINS):
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral) or not MIN_BINS <= int(bins) <= MAX_BINS:
        raise ValueError(f"hist_bins must be an integer {MIN_BINS}..{MAX_BINS}, not {bins!r}")
    return int(bins)


def normalize_weights(value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index of Vgg19.layer_names.  `value`: None or 0 (zeros); a number (that weight on those of
    relu1_1 and relu4_1 - indices 0 and 3, Risser's layers - that are style maps of the job; an error when there are none);
    a sequence of six numbers; or a dict {map index or name: number} (the rest 0).  `style_indices`: the job's style maps
    (None: the reference's 0, 1, 2, 3, 5 for a number, and a sequence or a dict is not checked against it); `use_relu`: the
    flavour whose map names a dict may use (None: either).
    ValueError for a negative or non-finite number, a wrong length, an unknown map, or a positive weight on a map that is
    not a style map of the job."""
    known = style_indices is not None
    style = sorted(DEFAULT_STYLE_INDICES) if not known else sorted({int(i) for i in style_indices})
    if value is None:
        return (0.0,) * NUM_MAPS
    if isinstance(value, (str, bytes, set, frozenset)):
        raise ValueError(f"hist_weight: expected a number, {NUM_MAPS} numbers or a dict, got {value!r}")
    if isinstance(value, (bool, numbers.Number)):
        w = _weight(value, "hist_weight")
        if w == 0.0:
            return (0.0,) * NUM_MAPS
        on = [i for i in RISSER_MAPS if i in style]
        if not on:
            raise ValueError(f"hist_weight: neither relu1_1 nor relu4_1 (indices 0 and 3) is a style map of the job {style}; "
                             f"give the weights by map")
        return tuple(w if i in on else 0.0 for i in range(NUM_MAPS))
    if isinstance(value, dict):
        ws = [0.0] * NUM_MAPS
        for key, v in value.items():
            ws[map_index(key, use_relu, _MAP_TEXTS)] = _weight(v, f"hist_weight of {key!r}")
    else:
        try:
            items = list(value)
        except TypeError:
            raise ValueError(f"hist_weight: expected a number, {NUM_MAPS} numbers or a dict, got {value!r}") from None
        if len(items) != NUM_MAPS:
            raise ValueError(f"hist_weight: expected {NUM_MAPS} numbers (one per feature map), got {len(items)}")
        ws = [_weight(v, f"hist_weight entry {i}") for i, v in enumerate(items)]
    for i, w in enumerate(ws):
        if known and w > 0.0 and i not in style:
            raise ValueError(f"hist_weight: map {i} has a positive weight but is not a style map of the job {style}")
    return tuple(ws)


def normalize_levels(levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices, as StyleEngine numbers them (0 = the full
    resolution).  `levels_num` (None: not checked beyond 0..7): the job's number of levels."""
    if levels is None:
        return None
    if isinstance(levels, (str, bytes, dict)) or isinstance(levels, (bool, numbers.Number)):
        raise ValueError(f"hist_levels: expected None or a collection of level indices, got {levels!r}")
    try:
        items = list(levels)
    except TypeError:
        raise ValueError(f"hist_levels: expected None or a collection of level indices, got {levels!r}") from None
    top = MAX_LEVELS if levels_num is None else int(levels_num)
    out = set()
    for v in items:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) < top:
            raise ValueError(f"hist_levels: {v!r} is not a level index 0..{top - 1}")
        out.add(int(v))
    if not out:
        raise ValueError("hist_levels: the collection is empty (None means every level)")
    return tuple(sorted(out))


def normalize_hist(weight=None, bins=DEFAULT_BINS, levels=None, style_indices=None, use_relu=None, levels_num=None):
    """(weights, bins, levels) - six weights by map index, the number of bins and the levels (None: all) - or None when the
    term is off (None, 0, all zeros).  Everything is validated, the off setting included."""
    bins = check_bins(bins)
    levels = normalize_levels(levels, levels_num)
    w = normalize_weights(weight, style_indices, use_relu)
    if all(v == 0.0 for v in w):
        return None
    return w, bins, levels


def check_exclusive(setting, regions=None, stripes: bool = False, extra_styles=None) -> None:
    """The term does not combine with several style images (a blend of histograms needs a common range: a follow-up), with
    spatial control (guided levels) or with stripe sharding."""
    if setting is None:
        return
    if extra_styles:
        raise ValueError("hist_weight cannot be combined with extra_styles")
    if regions is not None:
        raise ValueError("hist_weight cannot be combined with content_regions / style_regions")
    if stripes:
        raise ValueError("hist_weight cannot be combined with stripe sharding")
