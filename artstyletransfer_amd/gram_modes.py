"""The Gram shift option: activation-shifted (Novak & Nikulin, "Improving the Neural Algorithm of Artistic Style", 2016)
and mean-centred (Li, Wang, Liu & Hou, "Demystifying Neural Style Transfer", 2017) style statistics, per feature map; see
nst_job_set_gram_shift in include/nst_hip.h.  One normaliser for every layer (Config, neural_style_transfer(),
NeuralStyleTransfer, LossBuilder, StyleEngine), kept free of torch so that config.py can validate with it: everything here
raises ValueError before any GPU work."""
import math
import numbers

from .taps import NUM_MAPS, map_index, map_index_texts

_MAP_TEXTS = map_index_texts("gram_shift")
MEAN = "mean"            # the spelling of a centred map


def _entry(v, what):
    """One map's setting -> (shift, centred)."""
    if isinstance(v, str):
        if v != MEAN:
            raise ValueError(f"{what} must be a finite number or {MEAN!r}, not {v!r}")
        return 0.0, True
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a finite number or {MEAN!r}, not {v!r}")
    s = float(v)
    if not math.isfinite(s):
        raise ValueError(f"{what} must be a finite number or {MEAN!r}, not {v!r}")
    return s, False


def normalize_gram_shift(value=None, use_relu=None):
    """(shift, center_mask) - six floats by map index of Vgg19.layer_names and the bit set of the centred maps, whose shift
    is 0 - or None when the option is off (None, 0, all zeros).  `value`: None; a number (that shift on every map); "mean"
    (every map centred); a sequence of six entries; or a dict {map index or name: entry} (the rest 0), an entry being a
    number or "mean".  `use_relu`: the flavour whose map names a dict may use (None: either).  ValueError for a non-finite
    number, another string, a wrong length or an unknown map."""
    if value is None:
        return None
    if isinstance(value, (str, numbers.Number)):
        entries = [_entry(value, "gram_shift")] * NUM_MAPS
    elif isinstance(value, dict):
        entries = [(0.0, False)] * NUM_MAPS
        for key, v in value.items():
            entries[map_index(key, use_relu, _MAP_TEXTS)] = _entry(v, f"gram_shift of {key!r}")
    else:
        if isinstance(value, (bytes, set, frozenset)):
            raise ValueError(f"gram_shift: expected a number, {MEAN!r}, {NUM_MAPS} entries or a dict, got {value!r}")
        try:
            items = list(value)
        except TypeError:
            raise ValueError(f"gram_shift: expected a number, {MEAN!r}, {NUM_MAPS} entries or a dict, got {value!r}") from None
        if len(items) != NUM_MAPS:
            raise ValueError(f"gram_shift: expected {NUM_MAPS} entries (one per feature map), got {len(items)}")
        entries = [_entry(v, f"gram_shift entry {i}") for i, v in enumerate(items)]
    shift = tuple(s for s, _ in entries)
    mask = sum(1 << i for i, (_, c) in enumerate(entries) if c)
    if mask == 0 and all(s == 0.0 for s in shift):
        return None
    return shift, mask


def check_exclusive(setting, regions=None, stripes: bool = False) -> None:
    """A non-trivial Gram shift does not combine with spatial control (guided Gram matrices) or with stripe sharding."""
    if setting is None:
        return
    if regions is not None:
        raise ValueError("gram_shift cannot be combined with content_regions / style_regions")
    if stripes:
        raise ValueError("gram_shift cannot be combined with stripe sharding")
