"""The long-term anchor (include/nst_hip.h, nst_anchor_fold) restated from the header: numpy, fp64 by default.  In fp32
every operation below is one IEEE rounding, so fold(..., dtype=np.float32) reproduces the `weight` and `parts` of the
kernel bit for bit; fold_torch is the same formula in torch, the evaluation the project's bound for a streaming kernel is
taken from (three times the distance of the torch-fp32 evaluation from fp64).  Shared by tests/test_long_term_host.py and
tests/test_hip_long_term.py; nothing here needs a GPU."""
import numpy as np
import torch

MAX_SOURCES = 8


def parts_of(weights, dtype=np.float64):
    """(parts (J,h,w), Wsum (h,w)) of J weight planes: c_j = w_j > 0 ? min(w_j, 1) : 0; s_0 = 0, l_j = max(c_j - s_j, 0),
    s_{j+1} = s_j + c_j; Wsum = ((l_0 + l_1) + ...)."""
    s = np.zeros(np.shape(weights[0]), dtype)
    parts = []
    for wj in weights:
        wj = np.asarray(wj).astype(dtype)
        c = np.where(wj > 0, np.minimum(np.nan_to_num(wj, nan=0.0), dtype(1)), dtype(0)).astype(dtype)
        parts.append(np.maximum(c - s, dtype(0)))
        s = s + c
    wsum = parts[0]
    for l in parts[1:]:
        wsum = wsum + l
    return np.stack(parts), wsum


def fold(sources, weights, dtype=np.float64):
    """(anchor (C,h,w), weight (h,w), parts (J,h,w), Wsum (h,w)): sources J x (C,h,w), weights J x (h,w), in the operation
    order of the header.  A source enters only where its l_j > 0 (a select: its non-finite values elsewhere do not leak)."""
    parts, wsum = parts_of(weights, dtype)
    src = [np.asarray(s).astype(dtype) for s in sources]
    have = np.zeros(wsum.shape, bool)
    base = np.zeros(src[0].shape, dtype)
    acc = src[0].copy()                                   # where no source is live: source 0
    safe = np.where(wsum > 0, wsum, dtype(1))
    for j, a in enumerate(src):
        on = parts[j] > 0
        first = on & ~have
        a = np.where(on[None], a, dtype(0))
        ratio = np.where(on, parts[j] / safe, dtype(0)).astype(dtype)
        nxt = acc + ratio[None] * (a - base)
        acc = np.where(first[None], a, np.where((on & have)[None], nxt, acc))
        base = np.where(first[None], a, base)
        have |= on
    return acc.astype(dtype), np.minimum(wsum, dtype(1)), parts, wsum


def fold_torch(sources, weights, dtype=torch.float32):
    """The anchor of fold() in torch at `dtype`, same order of operations."""
    src = [torch.as_tensor(np.asarray(s)).to(dtype) for s in sources]
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    s = torch.zeros(src[0].shape[1:], dtype=dtype)
    parts = []
    for wj in weights:
        wj = torch.nan_to_num(torch.as_tensor(np.asarray(wj)).to(dtype), nan=0.0)
        c = torch.where(wj > 0, torch.minimum(wj, one), zero)
        parts.append(torch.maximum(c - s, zero))
        s = s + c
    wsum = parts[0]
    for l in parts[1:]:
        wsum = wsum + l
    safe = torch.where(wsum > 0, wsum, one)
    have = torch.zeros(wsum.shape, dtype=torch.bool)
    base = torch.zeros_like(src[0])
    acc = src[0].clone()
    for j, a in enumerate(src):
        on = parts[j] > 0
        first = on & ~have
        a = torch.where(on[None], a, zero)
        ratio = torch.where(on, parts[j] / safe, zero)
        nxt = acc + ratio[None] * (a - base)
        acc = torch.where(first[None], a, torch.where((on & have)[None], nxt, acc))
        base = torch.where(first[None], a, base)
        have = have | on
    return acc.numpy()


def mean_anchor(sources, parts):
    """a~ = sum_j l_j a_j / W in fp64, the plain weighted mean (source 0 where W = 0): what the header's incremental form
    a_j* + sum (l_j / W)(a_j - a_j*) equals in exact arithmetic."""
    parts = np.asarray(parts, np.float64)
    w = parts.sum(0)
    num = sum(np.where(parts[j][None] > 0, np.asarray(a, np.float64), 0.0) * parts[j][None] for j, a in enumerate(sources))
    return np.where(w[None] > 0, num / np.where(w > 0, w, 1.0)[None], np.asarray(sources[0], np.float64)), w


def constant(sources, parts):
    """(1/n) sum_{ch,p} sum_j l_j (a_j - a~)^2, n = C h w: what the J-term loss exceeds tmp of the folded anchor by."""
    abar, _ = mean_anchor(sources, parts)
    parts = np.asarray(parts, np.float64)
    total = 0.0
    for j, a in enumerate(sources):
        d = np.where(parts[j][None] > 0, np.asarray(a, np.float64) - abar, 0.0)
        total += float((parts[j][None] * d * d).sum())
    return total / abar.size


def vec_paths(source_ptrs, weight_ptrs, anchor_ptr, weight_ptr, parts_ptr, C, hw):
    """The kernel's per-plane rule for 16-byte accesses, from the byte addresses: {'weights': bool, 'channels': [bool] * C,
    'parts': [bool] * J or None, 'quads': full groups of four pixels, 'tail': h w % 4 pixels that go one by one}."""
    al = lambda p: p % 16 == 0
    J = len(source_ptrs)
    return {
        "weights": al(weight_ptr) and all(al(p) for p in weight_ptrs),
        "channels": [al(anchor_ptr + 4 * ch * hw) and all(al(p + 4 * ch * hw) for p in source_ptrs) for ch in range(C)],
        "parts": None if parts_ptr is None else [al(parts_ptr + 4 * j * hw) for j in range(J)],
        "quads": hw // 4,
        "tail": hw % 4,
    }


def random_weights(J, h, w, seed):
    """J planes uniform in [0,1] (fp32) with a fifth exact 0 and a fifth exact 1."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(J):
        c = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
        kind = rng.uniform(0.0, 1.0, (h, w))
        c[kind < 0.2] = 0.0
        c[kind > 0.8] = 1.0
        out.append(c)
    return out


def random_sources(J, C, h, w, seed):
    """J planes sets on the scale of prepared images."""
    rng = np.random.RandomState(seed)
    return [rng.uniform(-120.0, 135.0, (C, h, w)).astype(np.float32) for _ in range(J)]
