"""The parameters of the two optical-flow estimators.  FlowParams: multi-scale Horn-Schunck with warping (nst_flow_estimate in
include/nst_hip.h) - the smoothness weight alpha, the pyramid scales, the warps per scale and the sweeps per warp.
TVL1Params: TV-L1 in its dual form on the same pyramid (nst_flow_tvl1_estimate) - the data weight lambda, the coupling theta,
the dual step tau, and the same three counts.  One normaliser each for every layer (video.neural_style_transfer_video,
StyleEngine.flow_estimate), kept free of torch like the other *_modes modules: everything here raises ValueError before any
GPU work."""
import math
import numbers
import struct
from typing import NamedTuple

MAX_SCALES = 12          # NST_MAX_FLOW_SCALES


class FlowParams(NamedTuple):
    """alpha: the smoothness weight, for images on the 0 ... 255 scale (IPOL's default); scales: pyramid scales, 0 = as many
    as fit (a scale exists while its smaller side is at least 8 pixels); warps: linearisations per scale; iterations: Jacobi
    sweeps per warp."""
    alpha: float = 15.0
    scales: int = 0
    warps: int = 5
    iterations: int = 50


def _float32(x):
    """x rounded to a float32, as a Python float; inf where it does not fit."""
    try:
        return struct.unpack("f", struct.pack("f", x))[0]
    except OverflowError:
        return math.inf


def _alpha_ok(alpha):
    """What the C ABI accepts: alpha as a float32 finite and > 0, alpha * alpha as a float32 a normal number (the sweep divides
    by the square alone where a pixel has no data term).  The product of two float32 is exact in a double, so rounding it once gives the fp32 product."""
    if not math.isfinite(alpha):
        return False
    a = _float32(alpha)
    return 0.0 < a < math.inf and 1.1754943508222875e-38 <= _float32(a * a) < math.inf


def _count(v, what, lowest, highest=2 ** 31 - 1):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not lowest <= int(v) <= highest:
        raise ValueError(f"{what} must be an integer in {lowest} .. {highest}, not {v!r}")
    return int(v)


def normalize_flow(value=None):
    """A FlowParams of plain Python numbers from None (the defaults), a FlowParams, or a tuple or dict of its fields.
    ValueError for anything else: an alpha that is no finite number > 0 (as a float32: the C ABI takes one), scales outside
    0 .. MAX_SCALES, warps or iterations below 1, an unknown field, a value of another type."""
    if value is None:
        value = FlowParams()
    elif isinstance(value, dict):
        unknown = set(value) - set(FlowParams._fields)
        if unknown:
            raise ValueError(f"flow parameters: unknown field(s) {sorted(unknown)}")
        value = FlowParams(**value)
    elif isinstance(value, tuple) and len(value) <= len(FlowParams._fields):
        value = FlowParams(*value)
    else:
        raise ValueError(f"flow parameters must be None, a FlowParams, or a tuple or dict of its fields, not {value!r}")
    alpha = value.alpha
    if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not _alpha_ok(float(alpha)):
        raise ValueError(f"flow alpha must be a finite number > 0 whose float32 square neither overflows nor is subnormal, not {alpha!r}")
    return FlowParams(float(alpha), _count(value.scales, "flow scales", 0, MAX_SCALES), _count(value.warps, "flow warps", 1),
                      _count(value.iterations, "flow iterations", 1))


class TVL1Params(NamedTuple):
    """lambda_: the weight of the data term, for images on the 0 ... 255 scale (IPOL's default; larger = less smooth); theta:
    the coupling of the two half-steps; tau: the step of the dual update; scales, warps, iterations: as FlowParams', the
    iterations being those of the dual scheme."""
    lambda_: float = 0.15
    theta: float = 0.3
    tau: float = 0.25
    scales: int = 0
    warps: int = 5
    iterations: int = 50


_NORMAL = 1.1754943508222875e-38      # the smallest normal float32


def _tvl1_ok(lambda_, theta, tau):
    """What the C ABI accepts: each as a float32 finite and > 0, and the constants of the iteration, lambda theta and tau / theta
    as float32, normal numbers.  Product and quotient of two float32 formed in a double and rounded once are the fp32 ones."""
    if not all(math.isfinite(x) for x in (lambda_, theta, tau)):
        return False
    l, t, s = _float32(lambda_), _float32(theta), _float32(tau)
    if not all(0.0 < x < math.inf for x in (l, t, s)):
        return False
    return all(_NORMAL <= _float32(x) < math.inf for x in (l * t, s / t))


def normalize_tvl1(value=None):
    """A TVL1Params of plain Python numbers from None (the defaults), a TVL1Params, or a dict of its fields.  ValueError for
    anything else (a FlowParams among them): lambda_, theta or tau no finite number > 0 as a float32, lambda_ theta or
    tau / theta no normal float32, scales outside 0 .. MAX_SCALES, warps or iterations below 1, an unknown field, a value of
    another type."""
    if value is None:
        value = TVL1Params()
    elif isinstance(value, dict):
        unknown = set(value) - set(TVL1Params._fields)
        if unknown:
            raise ValueError(f"TV-L1 flow parameters: unknown field(s) {sorted(unknown)}")
        value = TVL1Params(**value)
    elif not isinstance(value, TVL1Params):
        raise ValueError(f"TV-L1 flow parameters must be None, a TVL1Params, or a dict of its fields, not {value!r}")
    reals = (value.lambda_, value.theta, value.tau)
    if any(isinstance(x, bool) or not isinstance(x, numbers.Real) for x in reals) or not _tvl1_ok(*(float(x) for x in reals)):
        raise ValueError("TV-L1 flow lambda_, theta and tau must be finite numbers > 0 whose float32 product lambda_ theta and "
                         f"quotient tau / theta are normal numbers, not {reals!r}")
    return TVL1Params(float(value.lambda_), float(value.theta), float(value.tau), _count(value.scales, "flow scales", 0, MAX_SCALES),
                      _count(value.warps, "flow warps", 1), _count(value.iterations, "flow iterations", 1))
