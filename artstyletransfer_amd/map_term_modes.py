"""What the settings of the per-map terms share - mrf_modes, hist_modes, remd_modes and selfsim_modes bind these to their own words: six
weights by map index of Vgg19.layer_names, the levels that carry the term, and what the term does not combine with.  Kept
free of torch: everything here raises ValueError before any GPU work."""
import math
import numbers
from typing import NamedTuple

from .taps import DEFAULT_STYLE_INDICES, NUM_MAPS, map_index, map_index_texts

MAX_LEVELS = 8


class Words(NamedTuple):
    """How a term's messages name it."""
    name: str               # the weight setting, "mrf_weight"
    levels_name: str        # the levels setting, "mrf_levels"
    default_maps: tuple     # the maps a plain number weighs
    no_default: str         # "... is a style map of the job": said when none of default_maps is one
    map_texts: tuple        # taps.map_index_texts(name)
    role: str = "a style map"   # what a weighted map must be: "... is not <role> of the job"


def words(name, levels_name, default_maps, no_default, role="a style map"):
    return Words(name, levels_name, tuple(default_maps), no_default, map_index_texts(name), role)


def _weight(v, what):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    w = float(v)
    if not math.isfinite(w) or w < 0.0:
        raise ValueError(f"{what} must be a finite number >= 0, not {v!r}")
    return w


def normalize_weights(t, value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index of Vgg19.layer_names.  `value`: None or 0 (zeros); a number (that weight on those of
    t.default_maps that are style maps of the job; an error when there are none); a sequence of six numbers; or a dict {map
    index or name: number} (the rest 0).  `style_indices`: the job's style maps (None: the reference's 0, 1, 2, 3, 5 for a
    number, and a sequence or a dict is not checked against it); `use_relu`: the flavour whose map names a dict may use (None:
    either).
    ValueError for a negative or non-finite number, a wrong length, an unknown map, or a positive weight on a map that is
    not a style map of the job."""
    known = style_indices is not None
    style = sorted(DEFAULT_STYLE_INDICES) if not known else sorted({int(i) for i in style_indices})
    if value is None:
        return (0.0,) * NUM_MAPS
    if isinstance(value, (str, bytes, set, frozenset)):
        raise ValueError(f"{t.name}: expected a number, {NUM_MAPS} numbers or a dict, got {value!r}")
    if isinstance(value, (bool, numbers.Number)):
        w = _weight(value, t.name)
        if w == 0.0:
            return (0.0,) * NUM_MAPS
        on = [i for i in t.default_maps if i in style]
        if not on:
            raise ValueError(f"{t.name}: {t.no_default} is {t.role} of the job {style}; give the weights by map")
        return tuple(w if i in on else 0.0 for i in range(NUM_MAPS))
    if isinstance(value, dict):
        ws = [0.0] * NUM_MAPS
        for key, v in value.items():
            ws[map_index(key, use_relu, t.map_texts)] = _weight(v, f"{t.name} of {key!r}")
    else:
        try:
            items = list(value)
        except TypeError:
            raise ValueError(f"{t.name}: expected a number, {NUM_MAPS} numbers or a dict, got {value!r}") from None
        if len(items) != NUM_MAPS:
            raise ValueError(f"{t.name}: expected {NUM_MAPS} numbers (one per feature map), got {len(items)}")
        ws = [_weight(v, f"{t.name} entry {i}") for i, v in enumerate(items)]
    for i, w in enumerate(ws):
        if known and w > 0.0 and i not in style:
            raise ValueError(f"{t.name}: map {i} has a positive weight but is not {t.role} of the job {style}")
    return tuple(ws)


def normalize_levels(t, levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices, as StyleEngine numbers them (0 = the full
    resolution).  `levels_num` (None: not checked beyond 0..7): the job's number of levels."""
    if levels is None:
        return None
    if isinstance(levels, (str, bytes, dict)) or isinstance(levels, (bool, numbers.Number)):
        raise ValueError(f"{t.levels_name}: expected None or a collection of level indices, got {levels!r}")
    try:
        items = list(levels)
    except TypeError:
        raise ValueError(f"{t.levels_name}: expected None or a collection of level indices, got {levels!r}") from None
    top = MAX_LEVELS if levels_num is None else int(levels_num)
    out = set()
    for v in items:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 0 <= int(v) < top:
            raise ValueError(f"{t.levels_name}: {v!r} is not a level index 0..{top - 1}")
        out.add(int(v))
    if not out:
        raise ValueError(f"{t.levels_name}: the collection is empty (None means every level)")
    return tuple(sorted(out))


def check_exclusive(t, setting, regions=None, stripes: bool = False, extra_styles=None) -> None:
    """A per-map term does not combine with several style images, with spatial control (guided levels) or with stripe
    sharding."""
    if setting is None:
        return
    if extra_styles:
        raise ValueError(f"{t.name} cannot be combined with extra_styles")
    if regions is not None:
        raise ValueError(f"{t.name} cannot be combined with content_regions / style_regions")
    if stripes:
        raise ValueError(f"{t.name} cannot be combined with stripe sharding")
