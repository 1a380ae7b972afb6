"""An integer-valued VGG19 for the exact-tie tests (test_exact_net_host.py, test_hip_exact_ties.py).

With ternary weights, integer biases and an integer image every product and every partial sum of the network is a small
integer, so any correct evaluation - fp32 MFMA, bf16x3, f16x2, the Winograd form, in any summation order - must give the
fp64 result BITWISE, forward and backward.  At the same time a large share of the pre-activations is exactly 0 and a large
share of the pooling windows holds its (positive) maximum at two or more positions: the first-maximum rule, the numbering
of the four window positions (q = 2 dy + dx, the scan order of torch's max_pool2d) and the strict `pre > 0` of the ReLU
become observable.  Plain helper module; the premises it relies on are held by test_exact_net_host.py."""
import functools

import torch
import torch.nn.functional as F

from oracle import cpu_ref

# the settings of the issue: (nnz, bias_lo, bias_hi, weight seed), image (blk, amp, seed)
NARROW = dict(nnz=3, bias_lo=-1, bias_hi=1, seed=7)
WIDE = dict(nnz=6, bias_lo=-3, bias_hi=1, seed=7)
IMAGE = dict(blk=4, amp=4, seed=11)
GOUT_DENSITY, GOUT_SEED = 0.05, 5


def ternary_vgg19_weights(nnz, bias_lo, bias_hi, seed):
    """13 (weight, bias) fp32 pairs in the layout of cpu_ref.synthetic_vgg19_weights: every output channel has `nnz` taps of
    its Cin*9, drawn without replacement, each +1 or -1 with equal chance; the bias is an integer in [bias_lo, bias_hi]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _, cin, cout in cpu_ref.VGG19_CONVS:
        taps = torch.rand(cout, cin * 9, generator=g).argsort(dim=1)[:, :nnz]          # a random subset per channel
        sign = torch.randint(0, 2, (cout, nnz), generator=g).float() * 2.0 - 1.0
        w = torch.zeros(cout, cin * 9).scatter_(1, taps, sign).view(cout, cin, 3, 3)
        b = torch.randint(bias_lo, bias_hi + 1, (cout,), generator=g).float()
        out.append((w.contiguous(), b))
    return out


def block_image(h, w, blk, amp, seed):
    """(1,3,h,w) fp32, constant on blk x blk blocks, block values integers in [-amp, amp]: an already-prepared image."""
    g = torch.Generator().manual_seed(seed)
    bh, bw = -(-h // blk), -(-w // blk)
    v = torch.randint(-amp, amp + 1, (1, 3, bh, bw), generator=g).float()
    return v.repeat_interleave(blk, 2).repeat_interleave(blk, 3)[:, :, :h, :w].contiguous()


def ternary_gouts(shapes, keep=(0, 1, 2, 3, 4, 5), density=GOUT_DENSITY, seed=GOUT_SEED):
    """Six output gradients, one per map of cpu_ref.TAPS: entries -1, 0, +1, `density` of them non-zero; None outside `keep`.
    Every tap draws from a generator of its own, so a tap's gradient does not depend on `keep`."""
    out = []
    for i, s in enumerate(shapes):
        if i not in keep:
            out.append(None)
            continue
        g = torch.Generator().manual_seed(seed + i)
        on = (torch.rand(tuple(s), generator=g) < density).float()
        out.append(on * (torch.randint(0, 2, tuple(s), generator=g).float() * 2.0 - 1.0))
    return out


# ---- the 2x2/2 pooling window, position q = 2 dy + dx ------------------------------------------------------------------
def windows(a):
    """(..., H/2, W/2, 4): the four units of every pooling window at positions 0..3 (a row or column left over is in none)."""
    h2, w2 = a.shape[-2] // 2, a.shape[-1] // 2
    a = a[..., :2 * h2, :2 * w2]
    return torch.stack((a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]), dim=-1)


def _scan(win, order):
    """Position of the first maximum when the window is scanned in `order`."""
    top = win.max(dim=-1).values
    pos = torch.full(top.shape, order[-1], dtype=torch.int64)
    for q in reversed(order[:-1]):
        pos = torch.where(win[..., q] == top, torch.full_like(pos, q), pos)
    return pos


RULES = {
    "first": lambda win: _scan(win, (0, 1, 2, 3)),         # torch's max_pool2d, the kernels' `if (e > best)` chain
    "last": lambda win: _scan(win, (3, 2, 1, 0)),          # `>=` instead of `>`
    "swap12": lambda win: _scan(win, (0, 2, 1, 3)),        # positions 1 and 2 exchanged: a column-major scan
}


def unwindow(g, pos, shape):
    """Backward of the pick: (..., H/2, W/2) -> shape (..., H, W), every window's value at its position `pos`."""
    out = torch.zeros(shape, dtype=g.dtype)
    h2, w2 = g.shape[-2], g.shape[-1]
    for q in range(4):
        out[..., q // 2:2 * h2:2, q % 2:2 * w2:2] = torch.where(pos == q, g, torch.zeros_like(g))
    return out


def tie_classes(a):
    """Of the windows of the post-ReLU map a: how many hold a positive maximum at two or more positions, split by the
    position of the first maximum (0, 1, 2), and how many hold it at positions 1 and 2 with position 0 lower - the class
    that tells a row-major scan from a column-major one.  Returns (windows, tied, (first0, first1, first2), one_two)."""
    win = windows(a)
    top = win.max(dim=-1).values
    eq = win == top.unsqueeze(-1)
    tied = (top > 0) & (eq.sum(-1) >= 2)
    first = _scan(win, (0, 1, 2, 3))
    split = tuple(int((tied & (first == q)).sum()) for q in range(3))
    one_two = int(((top > 0) & eq[..., 1] & eq[..., 2] & ~eq[..., 0]).sum())
    return top.numel(), int(tied.sum()), split, one_two


def frac_bits(t, limit=40):
    """The smallest f for which t * 2**f is integral (fp64 tensor)."""
    for f in range(limit + 1):
        s = t * 2.0 ** f
        if bool((s == s.round()).all()):
            return f
    return None


# ---- the network in fp64 -----------------------------------------------------------------------------------------------
def forward64(x, weights, pooling="max", rule="first", alive=lambda pre: pre > 0):
    """fp64 forward: (13 pre-activations, 13 ReLU masks, positions of the four pools {name: (..., H/2, W/2) int64}).
    `rule` (RULES) picks the pooling position, `alive` the units the ReLU keeps."""
    x = x.double()
    pres, masks, picks = [], [], {}
    for (name, _, _), (w, b) in zip(cpu_ref.VGG19_CONVS, weights):
        pre = F.conv2d(x, w.double(), b.double(), padding=1)
        m = alive(pre)
        pres.append(pre)
        masks.append(m)
        x = torch.relu(pre)                          # (a unit kept on at pre == 0 still outputs 0: `alive` shows in the backward)
        if name in cpu_ref.POOL_AFTER:
            win = windows(x)
            if pooling == "avg":
                x = win.sum(-1) * 0.25
            else:
                picks[name] = RULES[rule](win)
                x = win.gather(-1, picks[name].unsqueeze(-1)).squeeze(-1)
    return pres, masks, picks


def backward64(weights, pres, masks, picks, gouts, pooling="max", stats=None):
    """fp64 image gradient of sum_i <map_i, gouts[i]> (gouts[i] None: the map has no gradient) for the forward above.
    `stats` (a list) receives per layer, conv5_1 first: (name, gradient w.r.t. the layer's input, max conv_transpose2d(|g|, |w|)
    - the bound of every partial sum of that gradient in any order)."""
    g = None
    for li in range(len(cpu_ref.VGG19_CONVS) - 1, -1, -1):
        name = cpu_ref.VGG19_CONVS[li][0]
        if name in cpu_ref.POOL_AFTER and g is not None:
            shape = pres[li].shape
            if pooling == "avg":
                up = (g * 0.25).repeat_interleave(2, -2).repeat_interleave(2, -1)
                g = torch.zeros(shape, dtype=torch.float64)
                g[..., :up.shape[-2], :up.shape[-1]] = up
            else:
                g = unwindow(g, picks[name], shape)
        if name in cpu_ref.TAPS and gouts[cpu_ref.TAPS.index(name)] is not None:
            add = gouts[cpu_ref.TAPS.index(name)].double()
            g = add if g is None else g + add
        if g is None:
            continue
        gpre = g * masks[li]
        w = weights[li][0].double()
        g = F.conv_transpose2d(gpre, w, padding=1)
        if stats is not None:
            stats.append((name, g, float(F.conv_transpose2d(gpre.abs(), w.abs(), padding=1).max())))
    return g


def autograd64(x, weights, gouts, pooling="max"):
    """The same gradient by torch's own autograd in fp64 (F.relu, F.max_pool2d / F.avg_pool2d): torch's own rule."""
    x = x.double().clone().requires_grad_(True)
    a, total = x, 0.0
    for (name, _, _), (w, b) in zip(cpu_ref.VGG19_CONVS, weights):
        a = F.relu(F.conv2d(a, w.double(), b.double(), padding=1))
        if name in cpu_ref.TAPS and gouts[cpu_ref.TAPS.index(name)] is not None:
            total = total + (a * gouts[cpu_ref.TAPS.index(name)].double()).sum()
        if name in cpu_ref.POOL_AFTER:
            a = F.avg_pool2d(a, 2, 2) if pooling == "avg" else F.max_pool2d(a, 2, 2)
    total.backward()
    return x.grad.detach()


def premise(x, weights, pooling="max", gouts=None):
    """What the bitwise tests rely on, from an fp64 evaluation: a dict with
    "pre": the 13 pre-activations; "layers": per layer a dict (name, frac_bits, max_abs, bound = max of conv2d(|a_in|, |w|)
    + |b|, alive = share with pre > 0, zero = share with pre == 0, zeros = their number); "pools": per pool a dict (name,
    windows, tied, first = (first0, first1, first2), one_two); with `gouts` also "grad" (the image gradient) and "backward":
    per layer (name, frac_bits, max_abs, bound = max of conv_transpose2d(|g|, |w|))."""
    pres, masks, picks = forward64(x, weights, pooling)
    out = {"pre": pres, "masks": masks, "picks": picks, "layers": [], "pools": []}
    a = x.double()
    for (name, _, _), (w, b), pre in zip(cpu_ref.VGG19_CONVS, weights, pres):
        bound = float((F.conv2d(a.abs(), w.double().abs(), padding=1) + b.double().abs().view(1, -1, 1, 1)).max())
        out["layers"].append(dict(name=name, frac_bits=frac_bits(pre), max_abs=float(pre.abs().max()), bound=bound,
                                  alive=float((pre > 0).double().mean()), zero=float((pre == 0).double().mean()),
                                  zeros=int((pre == 0).sum())))
        a = torch.relu(pre)
        if name in cpu_ref.POOL_AFTER:
            n, tied, first, one_two = tie_classes(a)
            out["pools"].append(dict(name=name, windows=n, tied=tied, first=first, one_two=one_two))
            a = windows(a).sum(-1) * 0.25 if pooling == "avg" else windows(a).max(-1).values
    if gouts is not None:
        stats = []
        out["grad"] = backward64(weights, pres, masks, picks, gouts, pooling, stats)
        out["backward"] = [dict(name=n, frac_bits=frac_bits(g), max_abs=float(g.abs().max()), bound=bd) for n, g, bd in stats]
    return out


def layer_input(p, li, x, pooling="max"):
    """The input of conv layer li in the evaluation p = premise(x, ...)."""
    if li == 0:
        return x.double()
    a = torch.relu(p["pre"][li - 1])
    if cpu_ref.VGG19_CONVS[li - 1][0] in cpu_ref.POOL_AFTER:
        a = windows(a).sum(-1) * 0.25 if pooling == "avg" else windows(a).max(-1).values
    return a


def tap_shapes(h, w):
    return [(1, c, h >> s, w >> s) for c, s in zip((64, 128, 256, 512, 512, 512), (0, 1, 2, 3, 3, 4))]


@functools.lru_cache(maxsize=None)
def weights_of(setting):
    return ternary_vgg19_weights(**{"narrow": NARROW, "wide": WIDE}[setting])


@functools.lru_cache(maxsize=None)
def image_of(h, w):
    return block_image(h, w, **IMAGE)


@functools.lru_cache(maxsize=None)
def case(setting, pooling, h, w, keep=None):
    """premise() of a setting ("narrow" | "wide") on the h x w block image, computed once and shared; `keep`: the taps that
    carry a ternary gradient (None: forward only).  Callers leave the result unchanged."""
    gouts = ternary_gouts(tap_shapes(h, w), keep) if keep is not None else None
    return premise(image_of(h, w), weights_of(setting), pooling, gouts)


@functools.lru_cache(maxsize=None)
def autograd_of(setting, pooling, h, w, keep):
    """torch's fp64 autograd gradient of the ternary output gradients on the taps `keep`, computed once and shared."""
    return autograd64(image_of(h, w), weights_of(setting), ternary_gouts(tap_shapes(h, w), keep), pooling)
