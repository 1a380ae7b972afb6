"""The histogram loss: every channel of a tapped feature map remapped so that its histogram becomes the style's, and the map
pulled towards its remap - Risser, Wilmot & Barnes, "Stable and Controllable Neural Texture Synthesis and Style Transfer
Using Histogram Losses" (2017); see nst_level_set_histograms in include/nst_hip.h.  The one normaliser of the term
(neural_style_transfer_hist(), NeuralStyleTransfer.set_histogram_loss, StyleEngine.set_histograms), kept free of torch:
everything here raises ValueError before any GPU work."""
import numbers

from . import map_term_modes as _terms
from .map_term_modes import MAX_LEVELS, _weight  # noqa: F401

DEFAULT_BINS = 256
MIN_BINS = 2
MAX_BINS = 1024
RISSER_MAPS = (0, 3)            # relu1_1 and relu4_1: the layers of the paper
_WORDS = _terms.words("hist_weight", "hist_levels", RISSER_MAPS, "neither relu1_1 nor relu4_1 (indices 0 and 3)")


def check_bins(bins=DEFAULT_BINS):
    if isinstance(bins, bool) or not isinstance(bins, numbers.Integral) or not MIN_BINS <= int(bins) <= MAX_BINS:
        raise ValueError(f"hist_bins must be an integer {MIN_BINS}..{MAX_BINS}, not {bins!r}")
    return int(bins)


def normalize_weights(value=None, style_indices=None, use_relu=None):
    """Six weights >= 0 by map index (map_term_modes.normalize_weights has the forms of `value`); a plain number weighs
    those of relu1_1 and relu4_1 - indices 0 and 3, Risser's layers - that are style maps of the job."""
    return _terms.normalize_weights(_WORDS, value, style_indices, use_relu)


def normalize_levels(levels=None, levels_num=None):
    """None (every level), or the sorted tuple of distinct level indices (map_term_modes.normalize_levels)."""
    return _terms.normalize_levels(_WORDS, levels, levels_num)


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
    _terms.check_exclusive(_WORDS, setting, regions, stripes, extra_styles)
