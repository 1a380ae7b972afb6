"""The moment loss: the channel means and standard deviations of the style maps matched to the style's - the "BN statistics
matching" of Li, Wang, Liu & Hou, "Demystifying Neural Style Transfer" (2017), and the style loss of Huang & Belongie,
"Arbitrary Style Transfer in Real-time with Adaptive Instance Normalization" (2017); see nst_job_set_moments in
include/nst_hip.h.  One normaliser for every layer (Config, neural_style_transfer(), NeuralStyleTransfer, LossBuilder,
StyleEngine), kept free of torch so that config.py can validate with it: everything here raises ValueError before any GPU
work."""
import math
import numbers

from .taps import DEFAULT_STYLE_INDICES, NUM_MAPS, map_index, map_index_texts

_MAP_TEXTS = map_index_texts("moment_weight")
DEFAULT_EPSILON = 1e-5
TERMS = ("both", "mean", "std")


def _weight(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    w = float(v)
    if not math.isfinite(w) or w < 0.0:
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    return w


def check_epsilon(epsilon=DEFAULT_EPSILON):
    if isinstance(epsilon, bool) or not isinstance(epsilon, numbers.Real):
        raise ValueError(f"moment_epsilon must be a finite number > 0, not {epsilon!r}")
    e = float(epsilon)
    if not math.isfinite(e) or not e > 0.0:
        raise ValueError(f"moment_epsilon must be a finite number > 0, not {epsilon!r}")
    return e


def check_terms(terms="both"):
    if terms not in TERMS:
        raise ValueError(f"moment_terms must be one of {TERMS}, not {terms!r}")
    return terms


def normalize_weights(value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index of Vgg19.layer_names.  `value`: None or 0 (zeros); a number (that weight on every map
    of `style_indices`, the job's style maps - None: the reference's 0, 1, 2, 3, 5); a sequence of six numbers; or a dict
    {map index or name: number} (the rest 0).  `use_relu`: the flavour whose map names a dict may use (None: either).
    ValueError for a negative or non-finite number, a wrong length, an unknown map, or a positive weight on a map that is
    not in `style_indices` (None: not checked for a sequence or a dict)."""
    style = None if style_indices is None else sorted({int(i) for i in style_indices})
    if value is None:
        return (0.0,) * NUM_MAPS
    if isinstance(value, (str, bytes, set, frozenset)):
        raise ValueError(f"moment_weight: expected a number, {NUM_MAPS} numbers or a dict, got {value!r}")
    if isinstance(value, (bool, numbers.Number)):
        w = _weight(value, "moment_weight")
        on = DEFAULT_STYLE_INDICES if style is None else style
        return tuple(w if i in on else 0.0 for i in range(NUM_MAPS))
    if isinstance(value, dict):
        ws = [0.0] * NUM_MAPS
        for key, v in value.items():
            ws[map_index(key, use_relu, _MAP_TEXTS)] = _weight(v, f"moment_weight of {key!r}")
    else:
        try:
            items = list(value)
        except TypeError:
            raise ValueError(f"moment_weight: expected a number, {NUM_MAPS} numbers or a dict, got {value!r}") from None
        if len(items) != NUM_MAPS:
            raise ValueError(f"moment_weight: expected {NUM_MAPS} numbers (one per feature map), got {len(items)}")
        ws = [_weight(v, f"moment_weight entry {i}") for i, v in enumerate(items)]
    if style is not None:
        for i, w in enumerate(ws):
            if w > 0.0 and i not in style:
                raise ValueError(f"moment_weight: map {i} has a positive weight but is not a style map of the job {style}")
    return tuple(ws)


def normalize_moments(moment_weight=None, moment_terms="both", moment_epsilon=DEFAULT_EPSILON, style_indices=None, use_relu=None):
    """(mean_w, std_w, epsilon) - six weights of the mean term and six of the deviation term by map index, and epsilon - or
    None when the term is off (None, 0, all zeros).  `moment_weight`: as normalize_weights takes it; `moment_terms`: "both"
    (the weight on both terms), "mean" or "std" (on that term alone); `moment_epsilon` > 0.  Everything is validated, the
    off setting included."""
    terms = check_terms(moment_terms)
    eps = check_epsilon(moment_epsilon)
    w = normalize_weights(moment_weight, style_indices, use_relu)
    if all(v == 0.0 for v in w):
        return None
    zeros = (0.0,) * NUM_MAPS
    return (w if terms != "std" else zeros), (w if terms != "mean" else zeros), eps


def check_setting(mean_w, std_w, epsilon=DEFAULT_EPSILON, style_indices=None):
    """The explicit form (StyleEngine.set_moments): each of `mean_w`, `std_w` as normalize_weights takes it.  Returns
    (mean_w, std_w, epsilon) or None when every weight is 0."""
    eps = check_epsilon(epsilon)
    wm = normalize_weights(mean_w, style_indices)
    ws = normalize_weights(std_w, style_indices)
    if all(v == 0.0 for v in wm + ws):
        return None
    return wm, ws, eps


def check_exclusive(setting, regions=None, stripes: bool = False) -> None:
    """The moment loss does not combine with spatial control (guided levels) or with stripe sharding."""
    if setting is None:
        return
    if regions is not None:
        raise ValueError("moment_weight cannot be combined with content_regions / style_regions")
    if stripes:
        raise ValueError("moment_weight cannot be combined with stripe sharding")
