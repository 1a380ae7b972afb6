"""Spatial control (Gatys et al. 2017, guided Gram matrices): the host side of `content_regions` / `style_regions` /
`region_weights`.  A region argument is an integer label map (H,W) with labels 0..R-1 or a float stack (R,H,W) in [0,1];
it is normalised to a float32 stack, resized to every pyramid level of its image on the host (nearest neighbour, pixel-centre
rule) and checked - R, value range, the mass of every region on every network scale - before any GPU work.  Pure numpy:
include/nst_hip.h (nst_level_set_guidance) has the definitions the device side implements."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_REGIONS = 4
NUM_SCALES = 5          # network scales 0..4 of the six feature maps
MAP_SCALE = (0, 1, 2, 3, 3, 4)   # network scale of each map of Vgg19.layer_names


def normalize_regions(regions, what: str = "regions") -> np.ndarray:
    """An integer label map (H,W) with labels 0..R-1 (every label present) or a float stack (R,H,W) in [0,1] -> the float32
    stack (R,H,W).  ValueError for any other shape or dtype, R outside 1..4, a label that is missing, a value outside
    [0,1] or non-finite."""
    a = np.asarray(regions)
    if a.dtype == bool or np.issubdtype(a.dtype, np.integer):
        if a.ndim != 2:
            raise ValueError(f"{what}: an integer label map has shape (H,W), got {a.shape}")
        a = a.astype(np.int64)
        if a.size == 0 or a.min() < 0:
            raise ValueError(f"{what}: labels are 0 .. R-1")
        r = int(a.max()) + 1
        if r > MAX_REGIONS:
            raise ValueError(f"{what}: {r} regions, at most {MAX_REGIONS}")
        missing = [k for k in range(r) if not (a == k).any()]
        if missing:
            raise ValueError(f"{what}: labels are 0 .. R-1 without gaps, {missing} do not occur")
        return np.stack([(a == k) for k in range(r)]).astype(np.float32)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"{what}: expected an integer label map (H,W) or a float stack (R,H,W), got dtype {a.dtype}")
    if a.ndim != 3:
        raise ValueError(f"{what}: a float stack has shape (R,H,W), got {a.shape}")
    if not 1 <= a.shape[0] <= MAX_REGIONS:
        raise ValueError(f"{what}: {a.shape[0]} regions, 1 .. {MAX_REGIONS} allowed")
    if a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"{what}: empty planes")
    if not np.isfinite(a).all() or a.min() < 0.0 or a.max() > 1.0:
        raise ValueError(f"{what}: values must be finite and in [0,1]")
    return np.ascontiguousarray(a, dtype=np.float32)


def nearest_index(size_dst: int, size_src: int) -> np.ndarray:
    """src = floor((dst + 0.5) * size_src / size_dst) for dst = 0 .. size_dst-1 (integer arithmetic: exact)."""
    d = np.arange(size_dst, dtype=np.int64)
    return np.minimum(((2 * d + 1) * size_src) // (2 * size_dst), size_src - 1)


def resize_nearest(stack: np.ndarray, h: int, w: int) -> np.ndarray:
    """(R,H,W) -> (R,h,w), nearest neighbour by the pixel-centre rule: keeps [0,1] and partitions."""
    if h < 1 or w < 1:
        raise ValueError("resize_nearest: empty target")
    ys = nearest_index(h, stack.shape[1])
    xs = nearest_index(w, stack.shape[2])
    return np.ascontiguousarray(stack[:, ys][:, :, xs], dtype=np.float32)


def pool_chain(stack: np.ndarray) -> List[np.ndarray]:
    """The guidance of the five network scales: the planes passed 0..4 times through the 2x2/2 mean pool (floor sizes, fp32,
    ((e00 + e01) + e10) + e11 times 1/4).  A scale that would be empty ends the list."""
    out = [np.ascontiguousarray(stack, dtype=np.float32)]
    for _ in range(NUM_SCALES - 1):
        t = out[-1]
        h, w = t.shape[1] // 2, t.shape[2] // 2
        if h < 1 or w < 1:
            break
        t = t[:, :2 * h, :2 * w]
        s = ((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + t[:, 1::2, 0::2]) + t[:, 1::2, 1::2]
        out.append((s * np.float32(0.25)).astype(np.float32))
    return out


def masses(stack: np.ndarray) -> np.ndarray:
    """n_r = sum_p t_r(p)^2 (fp64) of every scale: (scales, R)."""
    return np.array([[float((t[r].astype(np.float64) ** 2).sum()) for r in range(t.shape[0])] for t in pool_chain(stack)])


def check_masses(stack: np.ndarray, scales: Sequence[int], what: str) -> None:
    """ValueError when a region has a mass below 1 on one of `scales` (less than one pixel's worth of guidance)."""
    m = masses(stack)
    for s in sorted(set(scales)):
        if s >= m.shape[0]:
            raise ValueError(f"{what}: the image is too small for network scale {s}")
        for r in range(m.shape[1]):
            if not m[s, r] >= 1.0:
                raise ValueError(f"{what}: region {r} has mass {m[s, r]:.3g} < 1 at network scale {s} of a "
                                 f"{stack.shape[1]}x{stack.shape[2]} level")


def check_region_weights(weights, r: int) -> Tuple[float, ...]:
    """R numbers >= 0, finite, at least one positive; None: ones."""
    if weights is None:
        return (1.0,) * r
    w = [float(v) for v in np.asarray(weights, dtype=np.float64).reshape(-1)]
    if len(w) != r:
        raise ValueError(f"region_weights: {len(w)} weights for {r} regions")
    if any(not np.isfinite(v) or v < 0.0 for v in w):
        raise ValueError("region_weights must be finite and >= 0")
    if not any(v > 0.0 for v in w):
        raise ValueError("region_weights: at least one must be positive")
    return tuple(w)


def check_regions(content_regions, style_regions, region_weights=None):
    """The three arguments of a job -> (content stack, style stack, region weights), or None when no region is given.
    ValueError for one of the two without the other, region weights without regions, mismatched R, and whatever
    normalize_regions / check_region_weights refuse."""
    if content_regions is None and style_regions is None:
        if region_weights is not None:
            raise ValueError("region_weights without content_regions / style_regions")
        return None
    if content_regions is None or style_regions is None:
        raise ValueError("content_regions and style_regions go together: one was given without the other")
    c = normalize_regions(content_regions, "content_regions")
    s = normalize_regions(style_regions, "style_regions")
    if c.shape[0] != s.shape[0]:
        raise ValueError(f"content_regions has {c.shape[0]} regions, style_regions {s.shape[0]}")
    return c, s, check_region_weights(region_weights, c.shape[0])


def level_planes(stack: np.ndarray, shapes: Sequence[Tuple[int, int]], style_indices: Sequence[int], what: str) -> List[np.ndarray]:
    """The stack resized to every level shape (h,w), each checked for its masses on the scales of the style maps in use."""
    scales = [MAP_SCALE[i] for i in style_indices]
    out = []
    for h, w in shapes:
        t = resize_nearest(stack, int(h), int(w))
        check_masses(t, scales, what)
        out.append(t)
    return out


def check_exclusive(regions, extra_styles=None, stripes: bool = False) -> None:
    """Guidance does not combine with several style images or with stripe sharding."""
    if regions is None:
        return
    if extra_styles is not None and len(extra_styles) > 0:
        raise ValueError("content_regions / style_regions cannot be combined with extra_styles")
    if stripes:
        raise ValueError("content_regions / style_regions cannot be combined with stripe sharding")
