"""The Laplacian loss option (Li, Xu, Nikolova & He, "Laplacian-Steered Neural Style Transfer", ACM MM 2017): up to four
entries (pool size, weight), see nst_job_set_laplacian in include/nst_hip.h.  One normaliser for every layer (Config,
neural_style_transfer(), NeuralStyleTransfer, LossBuilder, StyleEngine), kept free of torch so that config.py can validate
with it: everything here raises ValueError before any GPU work."""
import math
import numbers
import operator

MAX_ENTRIES = 4          # NST_MAX_LAPLACIAN
MAX_POOL = 32
MIN_POOLED = 3           # the valid 3x3 stencil needs a pooled image of at least 3x3
DEFAULT_POOL = 4


def _as_list(value, what):
    """A number -> [number]; a sequence (list, tuple, numpy array) -> its items.  Strings, dicts, sets and None are refused."""
    if isinstance(value, (str, bytes, dict, set, frozenset)) or value is None:
        raise ValueError(f"{what} must be a number or a sequence of up to {MAX_ENTRIES} numbers, not {value!r}")
    if isinstance(value, numbers.Number):
        return [value], True
    try:
        items = list(value)
    except TypeError:
        raise ValueError(f"{what} must be a number or a sequence of up to {MAX_ENTRIES} numbers, not {value!r}") from None
    if not 1 <= len(items) <= MAX_ENTRIES:
        raise ValueError(f"{what} must have 1 .. {MAX_ENTRIES} entries, not {len(items)}")
    return items, False


def _pool(v):
    if isinstance(v, bool):
        raise ValueError(f"a Laplacian pool size must be an integer in 1 .. {MAX_POOL}, not {v!r}")
    try:
        p = operator.index(v)
    except TypeError:
        raise ValueError(f"a Laplacian pool size must be an integer in 1 .. {MAX_POOL}, not {v!r}") from None
    if not 1 <= p <= MAX_POOL:
        raise ValueError(f"a Laplacian pool size must be an integer in 1 .. {MAX_POOL}, not {v!r}")
    return p


def _weight(v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"a Laplacian weight must be a finite number >= 0, not {v!r}")
    w = float(v)
    if not math.isfinite(w) or w < 0.0:
        raise ValueError(f"a Laplacian weight must be a finite number >= 0, not {v!r}")
    return w


def normalize_laplacian(weight=None, pool=DEFAULT_POOL):
    """(pools, weights) - two tuples of equal length 1..4, ascending in the order given, zero-weight entries dropped - or
    None when the term is off (weight None, 0 or all zeros).  `weight` and `pool` are each a number or a sequence; a single
    weight goes with every pool size, a single pool size with a single weight.  ValueError for anything else: more than
    four entries, lengths that differ, a pool size that is no integer in 1..32, duplicate pool sizes, a negative or
    non-finite weight."""
    pools, _ = _as_list(pool, "laplacian_pool")
    pools = [_pool(p) for p in pools]
    if len(set(pools)) != len(pools):
        raise ValueError(f"laplacian_pool: the pool sizes must be distinct, got {tuple(pools)}")
    if weight is None:
        return None
    weights, scalar = _as_list(weight, "laplacian_weight")
    weights = [_weight(w) for w in weights]
    if scalar:
        weights = weights * len(pools)
    if len(weights) != len(pools):
        raise ValueError(f"laplacian_weight has {len(weights)} entries, laplacian_pool {len(pools)}")
    kept = [(p, w) for p, w in zip(pools, weights) if w > 0.0]
    if not kept:
        return None
    return tuple(p for p, _ in kept), tuple(w for _, w in kept)


def pooled_shape(h, w, level, pool):
    """(hk, wk) of pyramid level `level` of an (h, w) job under pool size `pool`: level sizes halve with floor, pooled sizes
    floor."""
    return (h >> level) // pool, (w >> level) // pool


def check_levels(pools, levels_num, h0, w0):
    """ValueError when some level of the job (levels_num levels, level 0 = (h0, w0), level l = previous // 2) pools to less
    than 3x3 under one of `pools`: what nst_job_set_laplacian refuses with NST_E_ARG, computed from the job geometry."""
    for level in range(int(levels_num)):
        for p in pools:
            hk, wk = pooled_shape(int(h0), int(w0), level, p)
            if hk < MIN_POOLED or wk < MIN_POOLED:
                raise ValueError(f"level {level} is too small for pool {p}: {h0 >> level}x{w0 >> level} pools to {hk}x{wk}, "
                                 f"the Laplacian needs at least {MIN_POOLED}x{MIN_POOLED}")
