"""The parameters of the optical-flow estimator (multi-scale Horn-Schunck with warping, see nst_flow_estimate in
include/nst_hip.h): the smoothness weight alpha, the pyramid scales, the warps per scale and the sweeps per warp.  One
normaliser for every layer (video.neural_style_transfer_video, StyleEngine.flow_estimate), kept free of torch like the other
*_modes modules: everything here raises ValueError before any GPU work."""
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
