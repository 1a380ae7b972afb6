"""The matting term option (Luan, Paris, Shechtman & Bala, "Deep Photo Style Transfer", CVPR 2017): a weight gamma and the
regulariser epsilon of the matting Laplacian, see nst_job_set_matting in include/nst_hip.h.  One normaliser for every layer
(Config, neural_style_transfer(), NeuralStyleTransfer, LossBuilder, StyleEngine), kept free of torch so that config.py can
validate with it: everything here raises ValueError before any GPU work."""
import math
import numbers

DEFAULT_EPSILON = 1e-7   # Luan's value
MIN_SIDE = 3             # one 3x3 window


def _number(v, what, positive):
    bound = "> 0" if positive else ">= 0"
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError(f"{what} must be a finite number {bound}, not {v!r}")
    x = float(v)
    if not math.isfinite(x) or x < 0.0 or (positive and x == 0.0):
        raise ValueError(f"{what} must be a finite number {bound}, not {v!r}")
    return x


def normalize_matting(weight=None, epsilon=DEFAULT_EPSILON):
    """(gamma, epsilon) as floats, or None when the term is off (weight None or 0).  ValueError for anything else: a weight
    that is no finite number >= 0 (as a float32: the C ABI takes one), an epsilon that is no finite number > 0.  The epsilon
    is checked even when the term is off; None stands for the default."""
    eps = DEFAULT_EPSILON if epsilon is None else _number(epsilon, "matting_epsilon", True)
    if weight is None:
        return None
    gamma = _number(weight, "matting_weight", False)
    if gamma > 3.4028234663852886e38:
        raise ValueError(f"matting_weight must fit a float32, not {weight!r}")
    if gamma == 0.0:
        return None
    return gamma, eps


def check_levels(levels_num, h0, w0):
    """ValueError when some level of the job (levels_num levels, level 0 = (h0, w0), level l = previous // 2) is smaller
    than one 3x3 window."""
    for level in range(int(levels_num)):
        h, w = int(h0) >> level, int(w0) >> level
        if h < MIN_SIDE or w < MIN_SIDE:
            raise ValueError(f"level {level} is {h}x{w}: the matting term needs at least {MIN_SIDE}x{MIN_SIDE}")
