"""The local accuracy statistic of the fp64 comparisons (CPU only: numpy / torch).

A whole-map norm averages a local defect away: a launch that drops the 2^-11-weighted cross products of the f16x2 arithmetic
on one halo column, in one partial tile, in one 32-channel chunk or in one wave's output channels is still right to ~2^-12
THERE, and after the division by the norm of the whole map it sits under every bound the closure tests use (2e-5).  So the
error is also taken per class of entries that a launch treats alike, and the worst class is what is bounded.

For a map `got` (C, H, W) and its fp64 truth `ref`:
  - every error is normalised by the rms of `ref` over the WHOLE map - the f16x2 error scales with the tensor (one power-of-two
    scale per operand tensor), not with the entry, and a dead channel must not divide by zero;
  - the error of a class is the rms of got - ref over the class, divided by that whole-map rms;
  - four families of classes: rows; columns; groups of 32 channels (each channel of a 3-channel image gradient); blocks of
    4 rows x 16 columns aligned at the origin, over all channels - the finest tile grid any launch uses: the 8- and 16-row
    conv_h2 tiles and Winograd's 8 x 16 tiles are unions of them (16 x 16 pixel blocks on an image gradient);
  - a partial edge block is a class of its own; a class of fewer than MIN_CLASS = 64 entries is merged into its neighbour;
  - the statistic of a family is the MAXIMUM over its classes; the whole-map value ("map") is a fifth statistic.

assert_locally_as_accurate bounds every statistic of the device's map by max(factor x the same statistic of a torch-fp32
evaluation of the same expression on the same inputs, floor)."""
import numpy as np

from hip_helpers import report

FAMILIES = ("rows", "columns", "channels", "blocks")
MIN_CLASS = 64
CHANNEL_GROUP = 32
BLOCK = (4, 16)                  # rows x columns, feature maps
IMAGE_BLOCK = (16, 16)           # image gradients
FACTOR, FLOOR = 4.0, 5e-7        # the project's standing factor for pieces (remd, histogram); test_closure_accuracy_vs_fp64_truth's floor
# The forward launches of conv_mode="bf16x3" (conv_bf3.hip), every family and the whole map alike.  Its six product chains go
# into ONE fp32 accumulator, so every chain's addition - also that of the 2^-16-small ones - rounds at the accumulator's
# magnitude: six roundings where an fp32 matrix instruction has one.  The CPU model (test_local_accuracy_host.py:
# test_bf16x3_factor_is_twice_what_the_model_predicts) in the kernel's K order, each K = 16 matrix instruction rounding into the
# accumulator after each K = 8 half, gives 3.4e-7, 4.9e-7, 6.7e-7 and 9.9e-7 at K = 576, 1152, 2304 and 4608 - the device
# measures 3.5e-7, 5.3e-7, 7.3e-7 and 1.0e-6 - which at K = 4608 is 5.5x torch-fp32 in the worst family.  The factor is twice
# that; no factor may pass 16, which the planted defects of the model all stand above.
BF16X3_FORWARD_FACTOR = 11.0
MAX_FACTOR = 16.0


def _bounds(n, step):
    return list(range(0, n, step)) + [n]


def _merge_run(bounds, per_unit):
    """Boundaries of a 1-D family whose classes have `per_unit` entries per index: classes below MIN_CLASS are merged with
    the classes after them until the minimum holds, a short last class into the one before it."""
    out = [bounds[0]]
    for b in bounds[1:]:
        if (b - out[-1]) * per_unit >= MIN_CLASS or b == bounds[-1]:
            out.append(b)
    if len(out) > 2 and (out[-1] - out[-2]) * per_unit < MIN_CLASS:
        del out[-2]
    return out


def _drop_smallest(bounds):
    seg = np.diff(bounds)
    i = int(np.argmin(seg))
    del bounds[i if i > 0 else i + 1]


def _block_bounds(C, H, W, bh, bw):
    """Row and column boundaries of the block grid: partial edge blocks stay classes of their own unless they hold fewer than
    MIN_CLASS entries - then the shorter (relative to the block) of the smallest row / column segment joins its neighbour."""
    rb, cb = _bounds(H, bh), _bounds(W, bw)
    while C * int(np.diff(rb).min()) * int(np.diff(cb).min()) < MIN_CLASS:
        can_r, can_c = len(rb) > 2, len(cb) > 2
        if not (can_r or can_c):
            break
        if can_r and (not can_c or int(np.diff(rb).min()) * bw <= int(np.diff(cb).min()) * bh):
            _drop_smallest(rb)
        else:
            _drop_smallest(cb)
    return rb, cb


def _labels(bounds):
    lab = np.zeros(bounds[-1], np.int64)
    for k in range(len(bounds) - 1):
        lab[bounds[k]:bounds[k + 1]] = k
    return lab


def class_grid(shape, image=False):
    """family -> boundaries of its classes for a (C, H, W) map: 'rows', 'columns', 'channels' one list each, 'blocks' a
    (row boundaries, column boundaries) pair.  Asserts that every class holds at least MIN_CLASS entries."""
    C, H, W = shape
    bh, bw = IMAGE_BLOCK if image else BLOCK
    grid = {"rows": _merge_run(_bounds(H, 1), C * W), "columns": _merge_run(_bounds(W, 1), C * H),
            "channels": _merge_run(_bounds(C, 1 if image else CHANNEL_GROUP), H * W), "blocks": _block_bounds(C, H, W, bh, bw)}
    sizes = class_sizes(shape, image, grid)
    for fam in FAMILIES:
        assert sizes[fam].min() >= MIN_CLASS, (fam, shape, int(sizes[fam].min()))
        assert sizes[fam].sum() == C * H * W, (fam, shape)
    return grid


def class_sizes(shape, image=False, grid=None):
    """family -> entries per class (blocks: a 2-D array, block rows x block columns)."""
    C, H, W = shape
    if grid is None:
        grid = class_grid(shape, image)
    rb, cb = grid["blocks"]
    return {"rows": np.diff(grid["rows"]) * C * W, "columns": np.diff(grid["columns"]) * C * H,
            "channels": np.diff(grid["channels"]) * H * W, "blocks": C * np.outer(np.diff(rb), np.diff(cb))}


def _as_map(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = a.astype(np.float64)
    if a.ndim == 4:
        assert a.shape[0] == 1, a.shape
        a = a[0]
    assert a.ndim == 3, a.shape
    return a


def local_errors(got, ref, image=False):
    """family -> the error of every class (rms of got - ref over the class / rms of ref over the whole map; blocks as a 2-D
    array), and 'map' -> the whole-map value."""
    got, ref = _as_map(got), _as_map(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = float(np.sqrt(np.mean(ref * ref)))
    assert scale > 0 and np.isfinite(scale)
    grid = class_grid(ref.shape, image)
    sizes = class_sizes(ref.shape, image, grid)
    sq = (got - ref) ** 2
    rb, cb = grid["blocks"]
    rl, cl = _labels(rb), _labels(cb)
    sums = {"rows": np.bincount(_labels(grid["rows"]), sq.sum(axis=(0, 2))),
            "columns": np.bincount(_labels(grid["columns"]), sq.sum(axis=(0, 1))),
            "channels": np.bincount(_labels(grid["channels"]), sq.sum(axis=(1, 2))),
            "blocks": np.bincount((rl[:, None] * (len(cb) - 1) + cl[None, :]).ravel(), sq.sum(axis=0).ravel(),
                                  minlength=(len(rb) - 1) * (len(cb) - 1)).reshape(len(rb) - 1, len(cb) - 1)}
    out = {fam: np.sqrt(sums[fam] / sizes[fam]) / scale for fam in FAMILIES}
    out["map"] = float(np.sqrt(sq.mean())) / scale
    return out


def local_stats(got, ref, image=False):
    """The five statistics: family -> (largest class error, index of that class), 'map' -> (whole-map error, None)."""
    errs = local_errors(got, ref, image)
    out = {"map": (errs["map"], None)}
    for fam in FAMILIES:
        e = errs[fam]
        i = np.unravel_index(int(np.argmax(e)), e.shape)
        out[fam] = (float(e[i]), tuple(int(k) for k in i) if len(i) > 1 else int(i[0]))
    return out


def assert_locally_as_accurate(got, ref64, ref32, what, factor=FACTOR, floor=FLOOR, image=False):
    """Every statistic of `got` against the fp64 truth `ref64` is at most max(factor x the same statistic of `ref32` - a
    torch-fp32 evaluation of the same expression on the same inputs -, floor).  `factor`: one number, or family -> number
    (families left out: FACTOR).  Reports every ratio; returns family -> (device statistic, torch-fp32 statistic)."""
    dev_s, t32_s = local_stats(got, ref64, image), local_stats(ref32, ref64, image)
    bad, parts, out = [], [], {}
    for fam in ("map",) + FAMILIES:
        f = factor.get(fam, FACTOR) if isinstance(factor, dict) else factor
        assert f <= MAX_FACTOR, (fam, f)
        (d, where), (t, _) = dev_s[fam], t32_s[fam]
        out[fam] = (d, t)
        ratio = f"{d / t:.2f}x" if t > 0 else "-"
        parts.append(f"{fam} {d:.2e} / {t:.2e} = {ratio}" + ("" if where is None else f" @{where}"))
        if not d <= max(f * t, floor):
            bad.append((fam, where, d, t, f))
    report(f"local accuracy {what}: device / torch-fp32 vs fp64 - " + ", ".join(parts))
    assert not bad, (what, bad)
    return out
