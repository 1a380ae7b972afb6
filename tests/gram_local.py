"""The Gram pass held locally (CPU only: numpy / torch): the statistic, the split rule restated, the window plan and a model.

tests/local_accuracy.py holds every convolution launch to fp64 per class of entries a launch treats alike.  This module does
the same for a Gram-shaped result (C x C) and adds what a Gram needs beyond it: the pixel axis is the K axis of the product, so
nothing of the OUTPUT is owned by one K chunk, one split or one slab of the finish pass - a defect there is spread over every
entry it touches and diluted by every other chunk.  An INPUT that is zero outside a pixel window [p0, p1) makes the window's
chunks the whole sum: every chunk, split and slab becomes observable through the output the kernels already have.

  statistic   errors normalised by the rms of the WHOLE fp64 matrix; classes: every 32 x 32 block (the MFMA accumulator),
              every TS x TS tile pair, every row; the whole matrix is a fourth statistic.  The bound is local_accuracy's:
              max(FACTOR x the same statistic of a torch-fp32 evaluation, FLOOR).
  split rule  gram_nsplit, gram_nsplit_in_batch and the pixels-per-split rule of gram.hip, restated.
  plan        window_plan / slab_plan: named pixel windows of a geometry; window_features says what a window isolates (which
              staged chunk and LDS buffer, which k-step, which slab of the finish reads ...) - the coverage proof of
              tests/test_gram_local_host.py is a statement about these sets.
  model       the f16x2 Gram in the kernel's K order (one power-of-two scale from the absmax, hi = fp16(x s), lo = fp16((x s -
              hi) 2^11), main + cross / 2048 per split, the slabs rounded to fp32, the finish pass's lane-group order), with
              planted defects.  The products of a split accumulate in double: the model shows what the PIECES and a defect
              leave, not the fp32 accumulators - the device bound is tied to torch-fp32 for that reason."""
import functools

import numpy as np
import torch

from hip_helpers import report
from local_accuracy import FACTOR, FLOOR, MAX_FACTOR

FAMILIES = ("blocks", "tiles", "rows")
BLOCK = 32
SLAB_BYTES = 32 << 20
BATCH_MAX = 16


# ---- the split rule of gram.hip ------------------------------------------------------------------------------------------------
def gram_ts(C):
    return 128 if C % 128 == 0 else (64 if C == 64 else 0)


def gram_kp(C):
    """pixels per staged chunk"""
    return 32 if gram_ts(C) == 128 else 128


def gram_pairs(C):
    T = C // gram_ts(C)
    return T * (T + 1) // 2


def gram_max_splits(C):
    """the largest split count of a channel count: 256 workgroups over the tile pairs, or the 32 MiB cap of the slabs"""
    return max(1, min(256 // gram_pairs(C), SLAB_BYTES // (C * C * 4)))


def _whole_chunks(chunks, ns):
    cps = -(-chunks // ns)
    return -(-chunks // cps)


def gram_nsplit(C, N):
    chunks = -(-N // gram_kp(C))
    return _whole_chunks(chunks, max(1, min(gram_max_splits(C), chunks)))


def gram_pix_per_split(C, N, nsplit):
    kp = gram_kp(C)
    chunks = -(-N // kp)
    return -(-chunks // nsplit) * kp


def gram_nsplit_in_batch(items, i):
    """items: [(C, N)].  The largest map of a channel count takes gram_nsplit; a smaller one the same PIXELS per workgroup."""
    C, N = items[i]
    nmax = max(n for c, n in items if c == C)
    scaled = max(1, -(-gram_nsplit(C, nmax) * N // nmax))
    ns = min(scaled, gram_nsplit(C, N))
    return _whole_chunks(-(-N // gram_kp(C)), ns)


def geometry(C, N, items=None, i=None):
    """(nsplit, pix_per_split) of a lone map, or of item i of a batch"""
    ns = gram_nsplit(C, N) if items is None else gram_nsplit_in_batch(items, i)
    return ns, gram_pix_per_split(C, N, ns)


def read64(slab, nslabs):
    """the finish pass reads this slab in its 64-at-a-time loop (else in the 32-at-a-time tail)"""
    g, m = slab % 8, slab // 8
    return g + 64 * (m // 8) + 56 < nslabs


# ---- the window plan -----------------------------------------------------------------------------------------------------------
def _split_range(N, pps, s):
    return s * pps, min((s + 1) * pps, N)


def window_features(C, N, nsplit, pps, p0, p1):
    """What the window [p0, p1) isolates in a (C, N) map cut into nsplit splits of pps pixels."""
    assert 0 <= p0 < p1 <= N and (nsplit - 1) * pps < N <= nsplit * pps, (C, N, nsplit, pps, p0, p1)
    kp, out = gram_kp(C), set()
    s0, s1 = p0 // pps, (p1 - 1) // pps
    if (p0, p1) == (N - 1, N):
        out.add("last_pixel")
    if N % 8 and p0 >= N - N % 8:
        out.add("ragged_group")
    if s0 != s1:
        out.add("straddle")
        return out
    a, b = _split_range(N, pps, s0)
    nch = -(-(b - a) // kp)
    if (p0, p1) == (a, b):
        out.add("split:one" if nch == 1 else ("split:odd" if nch % 2 else "split:even"))
    c0, c1 = (p0 - a) // kp, (p1 - 1 - a) // kp
    if c0 == c1:
        out.add("chunk:load0" if c0 == 0 else ("chunk:load1" if c0 == 1 else f"chunk:loop_buf{c0 & 1}"))
        k0, k1 = ((p0 - a) % kp) // 16, ((p1 - 1 - a) % kp) // 16
        if k0 == k1:
            out.add(f"kstep:{k0 & 1}")
    if s0 == nsplit - 1 and c1 == nch - 1 and (b - a) % kp and p1 == N:
        out.add("ragged_chunk")
    out.add(f"slab:group{s0 % 8}")
    out.add("slab:read64" if read64(s0, nsplit) else "slab:read32")
    if s0 == 0:
        out.add("slab:0")
    if s0 == nsplit - 1 and nsplit > 1:
        if nsplit % 8:
            out.add("slab:last_not_mult8")
        if nsplit == gram_max_splits(C):
            out.add("slab:last_of_max")
    return out


def _dedupe(wins, N):
    seen, out = set(), []
    for name, p0, p1 in wins:
        p0, p1 = max(0, p0), min(N, p1)
        if p0 < p1 and (p0, p1) not in seen:
            seen.add((p0, p1))
            out.append((name, p0, p1))
    return out


def window_plan(C, N, nsplit, pps):
    """Named windows [p0, p1) of a geometry: in a middle split (a full one) its first four chunks - the two of the prologue and
    the two the loop stages, one per LDS buffer - and the k-steps of its first chunk (a 64-wide tile: of its first and last
    wave's pixel slice); the first and the last split whole; a window across a split boundary; the ragged last chunk, the
    ragged last 8-pixel group and the last pixel."""
    kp = gram_kp(C)
    s = nsplit // 2 if nsplit > 2 else 0
    a, b = _split_range(N, pps, s)
    wins = [(f"split{s}.chunk{c}", a + c * kp, min(a + (c + 1) * kp, b)) for c in range(min(4, -(-(b - a) // kp)))]
    for slice0 in ((0,) if kp == 32 else (0, 96)):
        for ks in (0, 1):
            wins.append((f"split{s}.pix{slice0}.kstep{ks}", a + slice0 + ks * 16, min(a + slice0 + ks * 16 + 16, b)))
    wins.append(("first split", *_split_range(N, pps, 0)))
    wins.append(("last split", *_split_range(N, pps, nsplit - 1)))
    if nsplit > 1:
        edge = max(s, 1) * pps
        wins.append((f"across the boundary at {edge}", edge - 8, edge + 8))
    if N % kp:
        wins.append(("ragged last chunk", N - N % kp, N))
    if N % 8:
        wins.append(("ragged last group", N - N % 8, N))
    wins.append(("last pixel", N - 1, N))
    return _dedupe(wins, N)


def slab_plan(C, N, nsplit, pps):
    """One whole-split window in each slab class of the finish pass: slabs 0 .. 7 (slab 0 and the 8 lane groups), the first
    slab past them that the 64-at-a-time loop reads, the first one left to the 32-at-a-time tail, the last slab."""
    picks = list(range(min(8, nsplit)))
    for want in (True, False):
        picks += [k for k in range(8, nsplit) if read64(k, nsplit) == want][:1]
    picks.append(nsplit - 1)
    return _dedupe([(f"slab {k}", *_split_range(N, pps, k)) for k in picks], N)


# ---- the statistic -------------------------------------------------------------------------------------------------------------
def _as_matrix(t):
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = a.astype(np.float64)
    if a.ndim == 3:
        assert a.shape[0] == 1, a.shape
        a = a[0]
    assert a.ndim == 2 and a.shape[0] == a.shape[1], a.shape
    return a


def gram_errors(got, ref, scale=None):
    """family -> the error of every class (rms of got - ref over the class / rms of ref over the whole matrix; `scale`
    replaces that rms), 'matrix' -> the whole-matrix value.  blocks: (C/32, C/32), tiles: (C/TS, C/TS), rows: (C,)."""
    got, ref = _as_matrix(got), _as_matrix(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    C = ref.shape[0]
    ts = gram_ts(C)
    assert ts, C
    if scale is None:
        scale = float(np.sqrt(np.mean(ref * ref)))
    assert scale > 0 and np.isfinite(scale)
    sq = (got - ref) ** 2
    cls = lambda n: np.sqrt(sq.reshape(C // n, n, C // n, n).mean(axis=(1, 3))) / scale
    return {"blocks": cls(BLOCK), "tiles": cls(ts), "rows": np.sqrt(sq.mean(axis=1)) / scale, "matrix": float(np.sqrt(sq.mean())) / scale}


def gram_stats(got, ref, scale=None):
    """family -> (largest class error, index of that class), 'matrix' -> (whole-matrix error, None)"""
    errs = gram_errors(got, ref, scale)
    out = {"matrix": (errs["matrix"], None)}
    for fam in FAMILIES:
        e = errs[fam]
        i = np.unravel_index(int(np.argmax(e)), e.shape)
        out[fam] = (float(e[i]), tuple(int(k) for k in i) if len(i) > 1 else int(i[0]))
    return out


def assert_gram_locally_as_accurate(got, ref64, ref32, what, factor=FACTOR, floor=FLOOR, scale=None):
    """Every statistic of `got` against the fp64 truth is at most max(factor x the same statistic of `ref32`, floor).  Reports
    every ratio (hip_helpers.report); returns family -> (device statistic, torch-fp32 statistic)."""
    assert factor <= MAX_FACTOR, factor
    dev_s, t32_s = gram_stats(got, ref64, scale), gram_stats(ref32, ref64, scale)
    bad, parts, out = [], [], {}
    for fam in ("matrix",) + FAMILIES:
        (d, where), (t, _) = dev_s[fam], t32_s[fam]
        out[fam] = (d, t)
        ratio = f"{d / t:.2f}x" if t > 0 else "-"
        parts.append(f"{fam} {d:.2e} / {t:.2e} = {ratio}" + ("" if where is None else f" @{where}"))
        if not d <= max(factor * t, floor):
            bad.append((fam, where, d, t, factor))
    report(f"gram local {what}: device / torch-fp32 vs fp64 - " + ", ".join(parts))
    assert not bad, (what, bad)
    return out


# ---- inputs and their truths ---------------------------------------------------------------------------------------------------
PEAK = 1.0
TAIL = 8


@functools.lru_cache(maxsize=4)
def feature_map(C, h, w):
    """The post-ReLU-like (1,C,h,w) map of test_hip_gram_pack.py, kept while the windows of a shape are walked - with the values
    of each of its last TAIL pixels (the ragged last group and the pixel N - 1) compressed towards PEAK x their rms.  That is the
    condition the bound puts on a window of one or two pixels: its Gram is f f^T, nothing is averaged over pixels, every entry
    carries the relative error of the two-piece cut (2^-22 at worst, 1.5e-7 rms), and row i stands at |f_i| / rms(f) times that.
    A pixel whose largest channel is 3 ... 4x its rms - any pixel of this map - puts the HEALTHY arithmetic at 4e-7 ... 6.6e-7
    in the rows family, on either side of the floor.  (A hard cap would make the peak channels equal and their errors coherent:
    the compression is smooth.)"""
    from test_hip_gram_pack import _map
    f = _map(C, h, w).clone()
    flat = f[0].reshape(C, -1)
    tail = flat[:, -TAIL:]
    cap = PEAK * tail.double().pow(2).mean(dim=0, keepdim=True).sqrt().float()
    flat[:, -TAIL:] = cap * torch.tanh(tail / cap)
    return f


def pixel_major(f):
    """(1,C,h,w) -> (N, C) float32, contiguous"""
    C = f.shape[1]
    return f[0].reshape(C, -1).t().contiguous()


def window_truths(F, p0, p1, divisor, t=None, o=None):
    """(fp64 truth, torch-fp32 yardstick) of the Gram of F (N, C) with every pixel outside [p0, p1) zeroed, / divisor.
    t (N,): the guided form sum_p t(p)^2 F F^T.  o (C,): the shifted form (F + o)(F + o)^T - the zeroed pixels inside [0, N) do
    contribute o o^T.  Without o only the window's rows are multiplied: the other rows add exact zeros in either precision."""
    N = F.shape[0]
    out = []
    for dt in (torch.float64, torch.float32):
        X = F[p0:p1].to(dt)
        if t is not None:
            X = X * t[p0:p1].to(dt)[:, None]
        if o is not None:
            od = o.to(dt)
            X = X + od[None, :]
            G = X.t() @ X + (N - (p1 - p0)) * torch.outer(od, od)
        else:
            G = X.t() @ X
        out.append((G / divisor).numpy())
    return out


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def operand_scale(absmax):
    """gram_h2_body's scale from the absmax record: 2^(141 - e) for the biased exponent e of the absmax, clamped to 32 .. 250"""
    e = int((np.float32(absmax).view(np.uint32) >> 23) & 0xFF)
    e = min(max(e, 32), 250)
    return float(2.0 ** (141 - e))


def _cut2(x, s):
    xs = (x.astype(np.float32) * np.float32(s)).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = ((xs - hi.astype(np.float32)).astype(np.float32) * np.float32(2048)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def _blk(rb, cb):
    return slice(rb * BLOCK, rb * BLOCK + BLOCK), slice(cb * BLOCK, cb * BLOCK + BLOCK)


def model_gram(F, nsplit, pps, divisor, window=None, t=None, o=None, absmax=None, defect=None):
    """The f16x2 Gram of F (N, C) float32 numpy, in the kernel's order.  window (p0, p1): the map is F inside it and zero outside
    (without o only the splits it touches are evaluated: the others are exact zeros; the absmax is the window's).  t: the guided form, o: the shifted form (absmax: the
    record of the shifted operand).  defect: None or (kind, args) -
      ("kstep_cross", split, first pixel of the k-step in the split, rb, cb)   both cross products of 16 pixels lost in a block
      ("one_cross", split, chunk, rb, cb)        lo x hi of one chunk lost in a block (the other cross product stays)
      ("wrong_fragment", split, rb, cb, cb2)     a wave slot multiplies fragment cb2 where it should take cb
      ("no_slab", split)                         the finish pass leaves a slab out
      ("tail_offsets",)                          shifted form: the staged pixels behind p1 of the last chunk hold o, not 0
      ("guide_off_by_one",)                      guided form: t is read one pixel late"""
    N, C = F.shape
    kp, ts = gram_kp(C), gram_ts(C)
    kind = defect[0] if defect else None
    if kind == "guide_off_by_one":
        t = np.concatenate([t[1:], np.zeros(1, t.dtype)])
    p0, p1 = window if window else (0, N)
    if absmax is None:
        absmax = float(np.abs(F[p0:p1]).max())
    s = operand_scale(absmax)
    q0, q1 = (p0, p1) if o is None else (0, N)
    slabs = {}
    for sp in range(q0 // pps, (q1 - 1) // pps + 1):
        a, b = _split_range(N, pps, sp)
        Xs = F[a:b].copy()
        Xs[:max(0, min(p0, b) - a)] = 0
        Xs[max(p1, a) - a:] = 0
        if t is not None:
            Xs = (Xs * t[a:b, None].astype(np.float32)).astype(np.float32)
        if o is not None:
            Xs = (Xs + o[None, :].astype(np.float32)).astype(np.float32)
            if kind == "tail_offsets" and sp == nsplit - 1 and (b - a) % kp:
                Xs = np.concatenate([Xs, np.repeat(o[None, :].astype(np.float32), kp - (b - a) % kp, axis=0)])
        hi, lo = _cut2(Xs, s)
        # a 64-wide tile: wave v owns pixels [32 v, 32 v + 32) of every chunk, the four partial sums meet in fp32 in wave order
        waves = [np.arange(len(Xs)) % kp // 32 == v for v in range(4)] if ts == 64 else [slice(None)]
        slab = None
        for v, rows in enumerate(waves):
            h, l = hi[rows], lo[rows]
            main, lo_hi, hi_lo = h.T @ h, l.T @ h, h.T @ l
            idx = np.arange(len(Xs))[rows]
            if sp == (defect[1] if kind in ("kstep_cross", "one_cross") else -1):
                if kind == "kstep_cross":
                    sel = (idx >= defect[2]) & (idx < defect[2] + 16)
                else:
                    sel = idx // kp == defect[2]
                B = _blk(defect[3], defect[4])
                lo_hi[B] -= (l[sel].T @ h[sel])[B]
                if kind == "kstep_cross":
                    hi_lo[B] -= (h[sel].T @ l[sel])[B]
            acc = _f32(main + (lo_hi + hi_lo) / 2048.0)
            if kind == "wrong_fragment" and sp == defect[1]:
                acc[_blk(defect[2], defect[3])] = acc[_blk(defect[2], defect[4])]
            slab = acc if slab is None else _f32(slab.astype(np.float64) + acc)
        slabs[sp] = _f32(slab.astype(np.float64) / (s * s))
    if kind == "no_slab":
        slabs.pop(defect[1], None)
    # the finish pass: lane group g adds every 8th slab in slab order, then the 8 group sums in group order, all in fp32
    groups = []
    for g in range(8):
        acc = np.zeros((C, C), np.float32)
        for k in sorted(k for k in slabs if k % 8 == g):
            acc = acc + slabs[k]
        groups.append(acc)
    tot = groups[0]
    for g in range(1, 8):
        tot = tot + groups[g]
    G = tot / np.float32(divisor)
    return np.triu(G) + np.triu(G, 1).T          # (elements with j >= i are read, each written to (i,j) and (j,i))
