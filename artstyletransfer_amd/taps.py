"""Feature-map choice of a job (the reference's LossBuilder(content_feature_maps_index, style_feature_maps_indices, ...)
and Vgg19(use_relu=...), neural_style_transfer.py:41-82, neural_nets.py:17-28): validation and the C ABI's encoding."""
from __future__ import annotations

import numbers

# Vgg19.layer_names of the two flavours (neural_nets.py:20-25 of the reference)
LAYER_NAMES = {True: ("relu1_1", "relu2_1", "relu3_1", "relu4_1", "conv4_2", "relu5_1"),
               False: ("conv1_1", "conv2_1", "conv3_1", "conv4_1", "conv4_2", "conv5_1")}
DEFAULT_CONTENT_INDEX = 4
DEFAULT_STYLE_INDICES = (0, 1, 2, 3, 5)
NUM_MAPS = 6


def _tap_index(v, use_relu: bool, what: str) -> int:
    names = LAYER_NAMES[bool(use_relu)]
    if isinstance(v, str):
        if v not in names:
            raise ValueError(f"{what}: {v!r} is not one of the feature maps {list(names)} (use_relu={bool(use_relu)})")
        return names.index(v)
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"{what}: expected an index 0..5 or a name of {list(names)}, got {v!r}")
    if not 0 <= v < len(names):
        raise ValueError(f"{what}: index {v} is outside 0..{len(names) - 1}")
    return v


def normalize_taps(content_layer=None, style_layers=None, use_relu=True):
    """(content index, sorted tuple of distinct style indices) of Vgg19.layer_names from indices or names of the
    `use_relu` flavour; None = the reference's taps (content 4, style [0, 1, 2, 3, 5]).  The reference keeps the
    indices of enumerate(features) that are `in` its lists, so order and repeats do not matter.  Where the reference
    silently ignores an out-of-range index or divides by zero on an empty style list, this raises ValueError; so it
    does for a content index that is not a single int (or name)."""
    if not isinstance(use_relu, bool):
        raise ValueError(f"use_relu must be True or False, got {use_relu!r}")
    content = DEFAULT_CONTENT_INDEX if content_layer is None else _tap_index(content_layer, use_relu, "content layer")
    if style_layers is None:
        style = DEFAULT_STYLE_INDICES
    else:
        items = [style_layers] if isinstance(style_layers, (int, str)) else list(style_layers)
        style = tuple(sorted({_tap_index(v, use_relu, "style layer") for v in items}))
        if not style:
            raise ValueError("style layers: the set is empty (the reference divides by its length)")
    return content, style


def map_index_texts(name):
    """The wording of `map_index`'s three refusals that the settings keyed by map share (gram_shift, moment_weight)."""
    return (name + ": {key!r} is not one of the feature maps {names}",
            name + f": expected a map index 0..{NUM_MAPS - 1} or a map name, got {{key!r}}",
            name + f": map index {{key}} is outside 0..{NUM_MAPS - 1}")


def map_index(key, use_relu, what) -> int:
    """Index 0..5 of a map of Vgg19.layer_names from an index or a name of the `use_relu` flavour (None: either).  `what`:
    the texts of the three refusals - an unknown name, a key that is no index, an index out of range - as format strings
    of `key` and `names`; every setting words them its own way."""
    unknown, no_index, outside = what
    if isinstance(key, str):
        flavours = (LAYER_NAMES[True], LAYER_NAMES[False]) if use_relu is None else (LAYER_NAMES[bool(use_relu)],)
        for names in flavours:
            if key in names:
                return names.index(key)
        raise ValueError(unknown.format(key=key, names=[n for names in flavours for n in names]))
    if isinstance(key, bool) or not isinstance(key, numbers.Integral):
        raise ValueError(no_index.format(key=key))
    if not 0 <= int(key) < NUM_MAPS:
        raise ValueError(outside.format(key=key))
    return int(key)


def style_mask(style) -> int:
    """Bit i set for every style index i (nst_job_set_taps)."""
    return sum(1 << i for i in style)


def is_default(content: int, style, use_relu: bool) -> bool:
    return content == DEFAULT_CONTENT_INDEX and tuple(style) == DEFAULT_STYLE_INDICES and use_relu
