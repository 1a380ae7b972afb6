"""GPU: the guided Gram backward launch alone (guided_bwd_kernel through nst_guided_gram_backward) against fp64:

    out[p][c] = addend[p][c] + sum_r t_r(p)^2 sum_k F[p][k] S_r[k][c]

The kernel forms t_r^2 (one rounding), t_r^2 F (one rounding), and the K = R C products exactly on the fp32 matrix cores,
accumulated in fp32 in a fixed order (at most two roundings per term, whether or not a product and its add are fused), then
adds the addend (one rounding).  With u = 2^-24 the standard bound of such a sum is, per element,

    |out - ref| <= (2 K + 4) u (|addend| + sum_r t_r^2 sum_k |F||S_r|)     (gamma_n <= n u (1 + small) for n u << 1)

which is what every case asserts, on every element; the measured rel-L2 is printed beside it.  Nothing of the bound comes
from what the kernel gives.  Cases: 17 x 65 = 1 105 pixels (eight whole 128-pixel blocks and a ragged one of 81), a pixel
count below one block, an exact multiple; C = 64 (one channel block) and C = 128 (two); R = 1, 3, 4; with and without an
addend, an addend that is the output buffer itself, the ReLU bit-mask (masked outputs are exactly zero), planes that are
zero over whole blocks, and the absmax record (exactly max |out|)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def eng(vgg_weights):
    from artstyletransfer_amd.engine import StyleEngine
    e = StyleEngine(vgg_weights, 0)
    yield e
    e.close()


def make(n, c, r, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(n, c, generator=g)) * 3.0                      # a post-ReLU map: about half zeros
    t = torch.rand(r, n, generator=g)
    t[0, : n // 2] = 0.0                                                     # region 0 is zero over whole leading blocks
    if r > 1:
        t[1, n // 2:] = 1.0                                                  # region 1 is hard one to the end, the ragged tail included
    s = torch.randn(r, c, c, generator=g) * 1e-3
    s = s + s.transpose(1, 2)                                                # S_r is symmetric in the closure
    addend = torch.randn(n, c, generator=g)
    keep = torch.rand(n, c, generator=g) > 0.4
    return f, t, s, addend, keep


def pack_bits(keep):
    n, c = keep.shape
    k = keep.reshape(n, c // 32, 32).to(torch.int64)
    words = (k << torch.arange(32, dtype=torch.int64)).sum(-1)               # bit (c & 31) of word c >> 5
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
    return words.to(torch.int32).contiguous()


def reference(f, t, s, addend, keep):
    f64, t2, s64 = f.double(), t.double() ** 2, s.double()
    ref = torch.zeros(f.shape, dtype=torch.float64)
    mag = torch.zeros(f.shape, dtype=torch.float64)
    for r in range(t.shape[0]):
        ref += t2[r][:, None] * (f64 @ s64[r])
        mag += t2[r][:, None] * (f64.abs() @ s64[r].abs())
    if addend is not None:
        ref += addend.double()
        mag += addend.double().abs()
    if keep is not None:
        ref = torch.where(keep, ref, torch.zeros_like(ref))
    return ref, mag


CASES = [  # n, c, r, addend ("none" / "separate" / "aliased"), bits
    (1105, 64, 3, "aliased", True),
    (1105, 64, 2, "separate", False),
    (300, 128, 4, "none", True),
    (81, 128, 1, "aliased", False),
    (256, 64, 1, "none", False),
    (6, 512, 4, "separate", True),          # a 2 x 3-pixel relu5_1 map: K = 2 048
]


@pytest.mark.parametrize("n,c,r,addend_kind,bits", CASES, ids=lambda v: str(v))
def test_guided_backward_against_fp64(eng, n, c, r, addend_kind, bits):
    f, t, s, addend, keep = make(n, c, r, seed=n + c + r)
    if addend_kind == "none":
        addend = None
    if not bits:
        keep = None
    ref, mag = reference(f, t, s, addend, keep)
    d = lambda a: a.cuda().contiguous()
    out = None
    add_d = None
    if addend_kind == "separate":
        add_d = d(addend)
    elif addend_kind == "aliased":
        out = d(addend)
        add_d = out
    got, amax = eng.guided_gram_backward(d(f), d(t), d(s), addend=add_d, relu_bits=d(pack_bits(keep)) if bits else None, out=out,
                                         want_absmax=True)
    torch.cuda.synchronize()
    got = got.cpu()
    err = (got.double() - ref).abs()
    bound = (2 * r * c + 4) * U * mag
    rel = float((got.double() - ref).norm() / ref.norm())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"guided backward N={n} C={c} R={r} addend={addend_kind} bits={bits}: rel-L2 {rel:.2e} against fp64, largest error "
          f"{worst:.3f} of its bound (2K+4)u with K = {r * c}")
    assert torch.isfinite(got).all()
    assert bool((err <= bound).all()), f"largest error is {worst:.3f} of the bound"
    if bits:
        assert bool((got[~keep] == 0).all()), "a masked output is not exactly zero"
    assert float(amax.cpu()) == float(got.abs().max()), "the absmax record is not max |out|"


def test_guided_backward_is_reproducible_and_refuses_bad_shapes(eng):
    from artstyletransfer_amd.engine import NstError
    f, t, s, addend, _ = make(1105, 64, 3, seed=9)
    d = lambda a: a.cuda().contiguous()
    a = eng.guided_gram_backward(d(f), d(t), d(s), addend=d(addend))
    b = eng.guided_gram_backward(d(f), d(t), d(s), addend=d(addend))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(NstError):
        eng.guided_gram_backward(d(f[:, :48]), d(t), d(s[:, :48, :48]))          # C is no multiple of 64
    with pytest.raises(NstError):
        eng.guided_gram_backward(d(f), d(t.repeat(2, 1)[:5]), d(s.repeat(2, 1, 1)[:5]))   # R = 5
    c = eng.guided_gram_backward(d(f), d(t), d(s), addend=d(addend))             # the context still works
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))
