"""The histogram loss restated in numpy (include/nst_hip.h has the definition): what the kernels of csrc/histogram.hip are held
to.  Range and bin run in numpy float32, one rounding per operation, so the counts and the fractions f are the device's bits.
The tables come from exact integers (int64: the products N Ns of every map the suite uses stay far below 2^63) and float64.
Remap, value and gradient are float64."""
import numpy as np


def canon(a):
    """-0 counts as +0 (the device's range keys)."""
    return (np.asarray(a, np.float32) + np.float32(0.0)).astype(np.float32)


def bin_scale(lo, hi, bins):
    """scale_c of the definition, 0 for a flat channel."""
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    flat = hi == lo
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (np.float64(bins) / np.where(flat, 1.0, hi64 - lo64)).astype(np.float32)
    return np.where(flat, np.float32(0.0), s).astype(np.float32)


def bins_of(f, lo, hi, bins):
    """f (N,C) float32 -> (b (N,C) int32, fr (N,C) float32, flat (C,) bool)."""
    f = np.asarray(f, np.float32)
    scale = bin_scale(lo, hi, bins)
    x = ((f - lo[None, :]).astype(np.float32) * scale[None, :]).astype(np.float32)
    b = np.clip(x.astype(np.int32), 0, bins - 1)
    fr = np.minimum(np.float32(1.0), (x - b.astype(np.float32)).astype(np.float32))
    return b, fr, hi == lo


def range_counts(f, bins):
    """f (N,C) float32 -> (lo_hi (C,2) float32, counts (C,B) int64); a flat channel counts nothing."""
    f = np.asarray(f, np.float32)
    lo, hi = canon(f.min(axis=0)), canon(f.max(axis=0))
    b, _, flat = bins_of(f, lo, hi, bins)
    c = f.shape[1]
    counts = np.zeros((c, bins), np.int64)
    for ch in range(c):
        if not flat[ch]:
            counts[ch] = np.bincount(b[:, ch], minlength=bins)
    return np.stack([lo, hi], axis=1), counts


def tables(counts, n, s_lo_hi, s_counts, ns, bins):
    """ends (C,B,2) float32: start_b and end_b of every non-empty image bin, zeros at the empty ones."""
    c = counts.shape[0]
    ends = np.zeros((c, bins, 2), np.float32)
    n, ns = int(n), int(ns)
    for ch in range(c):
        cnt = counts[ch].astype(np.int64)
        scnt = s_counts[ch].astype(np.int64)
        live = np.nonzero(cnt)[0]
        if live.size == 0:
            continue
        slo, shi = np.float64(s_lo_hi[ch, 0]), np.float64(s_lo_hi[ch, 1])
        if shi == slo or scnt.sum() == 0:
            ends[ch, live, :] = np.float32(slo)
            continue
        cum = np.concatenate([[0], np.cumsum(cnt)])
        scum = np.concatenate([[0], np.cumsum(scnt)])
        keys = scum[1:] * n
        width = (shi - slo) / np.float64(bins)
        for side, which, pick in (("right", 0, cum[live]), ("left", 1, cum[live + 1])):
            x = pick * ns
            j = np.searchsorted(keys, x, side=side)
            t = (x - scum[j] * n).astype(np.float64) / (scnt[j] * n).astype(np.float64)
            ends[ch, live, which] = (slo + (j.astype(np.float64) + t) * width).astype(np.float32)
    return ends


def remap(f, lo_hi, ends, bins):
    """(R (N,C) float64, flat (C,), parts) - parts = (start, fr, end) as float64 for the rounding bounds."""
    b, fr, flat = bins_of(f, lo_hi[:, 0], lo_hi[:, 1], bins)
    ch = np.arange(f.shape[1])[None, :]
    start = ends[ch, b, 0].astype(np.float64)
    end = ends[ch, b, 1].astype(np.float64)
    r = start + fr.astype(np.float64) * (end - start)
    r = np.where(flat[None, :], np.asarray(f, np.float64), r)
    return r, flat, (start, fr.astype(np.float64), end)


def term(f, lo_hi, ends, bins, coef=None):
    """(hist (float64), dF (N,C) float64) at fixed tables; coef None: 2 / (C N)."""
    f = np.asarray(f, np.float32)
    r, _, _ = remap(f, lo_hi, ends, bins)
    d = f.astype(np.float64) - r
    if coef is None:
        coef = 2.0 / d.size
    return float((d * d).sum() / d.size), np.float64(np.float32(coef)) * d


def full(f, fs, bins):
    """Everything from the two maps: (lo_hi, counts, s_lo_hi, s_counts, ends)."""
    lo_hi, counts = range_counts(f, bins)
    s_lo_hi, s_counts = range_counts(fs, bins)
    return lo_hi, counts, s_lo_hi, s_counts, tables(counts, f.shape[0], s_lo_hi, s_counts, fs.shape[0], bins)
