// flow.hip - the optical flow a sequence needs when the caller has none: multi-scale Horn-Schunck with warping (Horn &
// Schunck 1981 in the coarse-to-fine form of Meinhardt-Llopis, Sanchez & Kondermann, IPOL 2013; include/nst_hip.h,
// nst_flow_estimate, has the normative definitions and the order of operations of every stage).
//   flow_reduce_kernel      one pyramid step: the 5-tap binomial along x, then along y, every second pixel kept
//   flow_prolong_kernel     a coarse flow to the next finer grid: the two-tap mean per axis, times 2
//   flow_linearize_kernel   Ix, Iy, rho at the current flow: B and its central differences sampled by the warp's position rule
//   flow_sweep_kernel       one Jacobi step of both flow planes - the hot loop: `iterations` launches per warp
// Streaming kernels: nothing is reduced and nothing is added atomically, so every run gives the same bits.  The sweep
// covers a row in groups of four pixels that start where the output row reaches a 16-byte boundary; a group loads and
// stores 16 bytes per lane where all seven planes lie on a boundary there, and single floats elsewhere (the pixels of a row before
// its first boundary, its last w % 4, and rows of a plane that start off a boundary).  The two planes of a flow are h w
// floats apart, so when h w % 4 != 0 no group has all seven planes on a boundary and the whole sweep takes single floats.
// alpha^2 + Ix^2 + Iy^2 is formed in the sweep: a sweep moves seven planes (u, v, Ix, Iy, rho in; u', v' out).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "nst_flow.h"
#include "nst_kernels.h"
#include "nst_sample.h"

namespace nst {

// ------------------------------------------------------------------ reduce: (h,w) -> ((h+1)/2, (w+1)/2)
__global__ __launch_bounds__(FLOW_THREADS) void flow_reduce_kernel(const float* __restrict__ in, int h, int w, int hc, int wc,
                                                                   float* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr float K0 = 0.0625f, K1 = 0.25f, K2 = 0.375f;      // (1, 4, 6, 4, 1) / 16, exact
    const size_t n = (size_t)hc * wc;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / (size_t)wc), x = (int)(p - (size_t)y * wc);
        int xi[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) xi[i] = min(max(2 * x + i - 2, 0), w - 1);
        float col[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const float* r = in + (size_t)min(max(2 * y + j - 2, 0), h - 1) * w;
            float s = K0 * r[xi[0]];
            s = s + K1 * r[xi[1]];
            s = s + K2 * r[xi[2]];
            s = s + K1 * r[xi[3]];
            s = s + K0 * r[xi[4]];
            col[j] = s;
        }
        float s = K0 * col[0];
        s = s + K1 * col[1];
        s = s + K2 * col[2];
        s = s + K1 * col[3];
        s = s + K0 * col[4];
        out[p] = s;
    }
}
hipError_t launch_flow_reduce(const float* in, int h, int w, float* out, hipStream_t stream) {
    if (h < 1 || w < 1 || !in || !out) return hipErrorInvalidValue;
    const int hc = (h + 1) / 2, wc = (w + 1) / 2;
    hipLaunchKernelGGL(flow_reduce_kernel, dim3(flow_blocks((size_t)hc * wc)), dim3(FLOW_THREADS), 0, stream, in, h, w, hc, wc, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ prolong: (2,hc,wc) -> (2,h,w), hc = (h+1)/2, wc = (w+1)/2
__global__ __launch_bounds__(FLOW_THREADS) void flow_prolong_kernel(const float* __restrict__ coarse, int hc, int wc, int h, int w,
                                                                    float* __restrict__ fine) {
#pragma clang fp contract(off)
    const size_t hw = (size_t)h * w, hwc = (size_t)hc * wc;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
        const int xa = x >> 1, xb = min(xa + (x & 1), wc - 1);
        const int ya = y >> 1, yb = min(ya + (y & 1), hc - 1);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const float* ra = coarse + pl * hwc + (size_t)ya * wc;
            const float* rb = coarse + pl * hwc + (size_t)yb * wc;
            const float top = 0.5f * (ra[xa] + ra[xb]);
            const float bot = 0.5f * (rb[xa] + rb[xb]);
            fine[pl * hw + p] = 2.f * (0.5f * (top + bot));
        }
    }
}
hipError_t launch_flow_prolong(const float* coarse, int h, int w, float* fine, hipStream_t stream) {
    if (h < 1 || w < 1 || !coarse || !fine) return hipErrorInvalidValue;
    hipLaunchKernelGGL(flow_prolong_kernel, dim3(flow_blocks((size_t)h * w)), dim3(FLOW_THREADS), 0, stream, coarse, (h + 1) / 2,
                       (w + 1) / 2, h, w, fine);
    return hipGetLastError();
}

// ------------------------------------------------------------------ linearise at the flow (u, v)
// Bx, By are never stored: the central differences are formed at the four taps, which gives the bits of sampling stored planes.
__global__ __launch_bounds__(FLOW_THREADS) void flow_linearize_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                                      const float* __restrict__ u, const float* __restrict__ v,
                                                                      int h, int w, float* __restrict__ Ix, float* __restrict__ Iy,
                                                                      float* __restrict__ rho) {
#pragma clang fp contract(off)
    const size_t hw = (size_t)h * w;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
        const float du = u[p], dv = v[p];
        float ix = 0.f, iy = 0.f, r = 0.f;
        if (isfinite(du) && isfinite(dv)) {
            const AxisTap ax = axis_tap(x, du, w), ay = axis_tap(y, dv, h);
            if (ax.inside && ay.inside) {
                const int xs[2] = {ax.i0, ax.i1}, ys[2] = {ay.i0, ay.i1};
                float gx[2][2], gy[2][2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float* row = B + (size_t)ys[j] * w;
                    const float* up = B + (size_t)max(ys[j] - 1, 0) * w;
                    const float* dn = B + (size_t)min(ys[j] + 1, h - 1) * w;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        gx[j][i] = 0.5f * (row[min(xs[i] + 1, w - 1)] - row[max(xs[i] - 1, 0)]);
                        gy[j][i] = 0.5f * (dn[xs[i]] - up[xs[i]]);
                    }
                }
                const float bw = bilinear(B, w, ax, ay);
                ix = bilinear_mix(gx[0][0], gx[0][1], gx[1][0], gx[1][1], ax.t, ay.t);
                iy = bilinear_mix(gy[0][0], gy[0][1], gy[1][0], gy[1][1], ax.t, ay.t);
                r = ((bw - ix * du) - iy * dv) - A[p];
            }
        }
        Ix[p] = ix;
        Iy[p] = iy;
        rho[p] = r;
    }
}
hipError_t launch_flow_linearize(const float* from, const float* to, const float* u, const float* v, int h, int w, float* Ix,
                                 float* Iy, float* rho, hipStream_t stream) {
    if (h < 1 || w < 1 || !from || !to || !u || !v || !Ix || !Iy || !rho) return hipErrorInvalidValue;
    hipLaunchKernelGGL(flow_linearize_kernel, dim3(flow_blocks((size_t)h * w)), dim3(FLOW_THREADS), 0, stream, from, to, u, v, h, w,
                       Ix, Iy, rho);
    return hipGetLastError();
}

// ------------------------------------------------------------------ sweep
namespace {

// columns x0 - 1 ... x0 + 4 of one row, clamped to the row: what the pixels x0 ... x0 + 3 need of it.  wide: x0 + 3 < w and
// row + x0 lies on a 16-byte boundary
__device__ __forceinline__ void sweep_row(const float* __restrict__ row, int x0, int w, bool wide, float o[6]) {
    o[0] = row[max(x0 - 1, 0)];
    if (wide) {
        const float4 q = *reinterpret_cast<const float4*>(row + x0);
        o[1] = q.x; o[2] = q.y; o[3] = q.z; o[4] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[1 + k] = row[min(x0 + k, w - 1)];
    }
    o[5] = row[min(x0 + 4, w - 1)];
}
// the pixels x0 ... x0 + 3 of one row of a plane the sweep reads at the centre only
template <bool WIDE>
__device__ __forceinline__ void sweep_centre(const float* __restrict__ row, int x0, int w, float o[4]) {
    if (WIDE) {
        const float4 q = *reinterpret_cast<const float4*>(row + x0);
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = row[min(x0 + k, w - 1)];
    }
}
template <bool WIDE>
__device__ __forceinline__ void sweep_store(float* __restrict__ row, int x0, int n, const float o[4]) {
    if (WIDE) {
        *reinterpret_cast<float4*>(row + x0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) row[x0 + k] = o[k];
    }
}
// the weighted mean of the eight neighbours of pixel x0 + k; a, b, c: sweep_row of the rows y - 1, y, y + 1
__device__ __forceinline__ float sweep_mean(const float a[6], const float b[6], const float c[6], int k) {
#pragma clang fp contract(off)
    const float cross = ((a[k + 1] + c[k + 1]) + b[k]) + b[k + 2];        // N + S + W + E
    const float diag = ((a[k] + a[k + 2]) + c[k]) + c[k + 2];             // NW + NE + SW + SE
    return cross / 6.f + diag / 12.f;
}

// The pixels x0 ... x0 + n - 1 of row y, n <= 4.  WIDE: n = 4 and the seven planes lie on a 16-byte boundary at (y, x0) -
// 16 bytes per lane on each; the rows above and below come as 16 bytes too where they lie on a boundary (every row does when
// w is a multiple of 4).
template <bool WIDE>
__device__ __forceinline__ void sweep_group(const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ Ix,
                                            const float* __restrict__ Iy, const float* __restrict__ rho, int h, int w, float alpha2,
                                            float* __restrict__ un, float* __restrict__ vn, int y, int x0, int n) {
#pragma clang fp contract(off)
    const size_t off = (size_t)y * w, up = (size_t)max(y - 1, 0) * w, dn = (size_t)min(y + 1, h - 1) * w;
    const bool wide_u = WIDE && aligned16(u + up + x0) && aligned16(u + dn + x0);
    const bool wide_v = WIDE && aligned16(v + up + x0) && aligned16(v + dn + x0);
    float ua[6], ub[6], uc[6], va[6], vb[6], vc[6], ix[4], iy[4], r[4], ou[4], ov[4];
    sweep_row(u + up, x0, w, wide_u, ua);
    sweep_row(u + off, x0, w, WIDE, ub);
    sweep_row(u + dn, x0, w, wide_u, uc);
    sweep_row(v + up, x0, w, wide_v, va);
    sweep_row(v + off, x0, w, WIDE, vb);
    sweep_row(v + dn, x0, w, wide_v, vc);
    sweep_centre<WIDE>(Ix + off, x0, w, ix);
    sweep_centre<WIDE>(Iy + off, x0, w, iy);
    sweep_centre<WIDE>(rho + off, x0, w, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float um = sweep_mean(ua, ub, uc, k), vm = sweep_mean(va, vb, vc, k);
        const float num = (r[k] + ix[k] * um) + iy[k] * vm;
        const float den = (alpha2 + ix[k] * ix[k]) + iy[k] * iy[k];
        const float t = num / den;
        ou[k] = um - ix[k] * t;
        ov[k] = vm - iy[k] * t;
    }
    sweep_store<WIDE>(un + off, x0, n, ou);
    sweep_store<WIDE>(vn + off, x0, n, ov);
}

// The groups without 16-byte accesses, out of line: inlined beside the wide path the compiler merges the tails of the two and
// splits the wide path's last store into 12 + 4 bytes.
__device__ __noinline__ void sweep_group_narrow(const float* __restrict__ u, const float* __restrict__ v, const float* __restrict__ Ix,
                                                const float* __restrict__ Iy, const float* __restrict__ rho, int h, int w, float alpha2,
                                                float* __restrict__ un, float* __restrict__ vn, int y, int x0, int n) {
    sweep_group<false>(u, v, Ix, Iy, rho, h, w, alpha2, un, vn, y, x0, n);
}

}  // namespace

__global__ __launch_bounds__(FLOW_THREADS) void flow_sweep_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                                  const float* __restrict__ Ix, const float* __restrict__ Iy,
                                                                  const float* __restrict__ rho, int h, int w, float alpha2,
                                                                  float* __restrict__ un, float* __restrict__ vn) {
    const size_t groups = (size_t)(w + 3) / 4 + 1;      // of one row: the pixels before the first boundary, then fours
    const size_t items = (size_t)h * groups;
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(it / groups), g = (int)(it - (size_t)y * groups);
        const size_t off = (size_t)y * w;
        // pixels of the row before the output row's first 16-byte boundary
        const int head = min((int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(un + off) & 15u)) & 15u) >> 2), w);
        const int x0 = g == 0 ? 0 : head + 4 * (g - 1);
        const int x1 = g == 0 ? head : min(x0 + 4, w);
        const int n = x1 - x0;
        if (n <= 0) continue;
        const size_t c = off + x0;
        const bool wide = n == 4 && aligned16(un + c) && aligned16(vn + c) && aligned16(u + c) && aligned16(v + c) &&
                          aligned16(Ix + c) && aligned16(Iy + c) && aligned16(rho + c);
        if (wide) sweep_group<true>(u, v, Ix, Iy, rho, h, w, alpha2, un, vn, y, x0, n);
        else sweep_group_narrow(u, v, Ix, Iy, rho, h, w, alpha2, un, vn, y, x0, n);
    }
}

namespace {

hipError_t launch_flow_sweep(const float* u, const float* v, const float* Ix, const float* Iy, const float* rho, int h, int w,
                             float alpha2, float* un, float* vn, hipStream_t stream) {
    const size_t items = (size_t)h * ((size_t)(w + 3) / 4 + 1);
    hipLaunchKernelGGL(flow_sweep_kernel, dim3(flow_blocks(items)), dim3(FLOW_THREADS), 0, stream, u, v, Ix, Iy, rho, h, w, alpha2,
                       un, vn);
    return hipGetLastError();
}

}  // namespace

// n Jacobi steps from `in`; step k writes `out` when n - k is even and `tmp` otherwise, so the last one writes `out`.  The
// first step must not write what it reads; a later one may overwrite `in` (the driver's two buffers).
hipError_t launch_flow_sweeps(const float* Ix, const float* Iy, const float* rho, const float* in, int h, int w, float alpha2, int n,
                              float* out, float* tmp, hipStream_t stream) {
    if (h < 1 || w < 1 || n < 1 || !Ix || !Iy || !rho || !in || !out || (n > 1 && !tmp) || out == tmp ||
        in == (((n - 1) & 1) ? tmp : out))
        return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    const float* src = in;
    for (int k = 1; k <= n; ++k) {
        float* dst = ((n - k) & 1) ? tmp : out;
        const hipError_t e = launch_flow_sweep(src, src + hw, Ix, Iy, rho, h, w, alpha2, dst, dst + hw, stream);
        if (e != hipSuccess) return e;
        src = dst;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ the driver
int flow_layout(int h, int w, int scales, FlowLayout* out) {
    if (h < 1 || w < 1 || scales < 0 || scales > NST_FLOW_MAX_SCALES || !out) return -1;
    const int limit = scales == 0 ? NST_FLOW_MAX_SCALES : scales;
    FlowLayout l{};
    l.h[0] = h; l.w[0] = w;
    l.scales = 1;
    size_t floats = 0;
    while (l.scales < limit) {
        const int hc = (l.h[l.scales - 1] + 1) / 2, wc = (l.w[l.scales - 1] + 1) / 2;
        if ((hc < wc ? hc : wc) < 8) break;
        l.h[l.scales] = hc; l.w[l.scales] = wc;
        l.from[l.scales] = floats; floats += round4((size_t)hc * wc);
        l.to[l.scales] = floats; floats += round4((size_t)hc * wc);
        ++l.scales;
    }
    const size_t hw = (size_t)h * w;
    l.ix = floats; floats += round4(hw);
    l.iy = floats; floats += round4(hw);
    l.rho = floats; floats += round4(hw);
    l.other = floats; floats += round4(2 * hw);
    l.floats = floats;
    *out = l;
    return 0;
}

hipError_t launch_flow_estimate(const float* from, const float* to, const FlowLayout& l, float alpha2, int warps, int iterations,
                                float* flow, float* ws, hipStream_t stream) {
    if (!from || !to || !flow || !ws || warps < 1 || iterations < 1 || l.scales < 1) return hipErrorInvalidValue;
    const int S = l.scales;
    const float* A[NST_FLOW_MAX_SCALES];
    const float* B[NST_FLOW_MAX_SCALES];
    A[0] = from; B[0] = to;
    for (int s = 1; s < S; ++s) {
        hipError_t e = launch_flow_reduce(A[s - 1], l.h[s - 1], l.w[s - 1], ws + l.from[s], stream);
        if (e == hipSuccess) e = launch_flow_reduce(B[s - 1], l.h[s - 1], l.w[s - 1], ws + l.to[s], stream);
        if (e != hipSuccess) return e;
        A[s] = ws + l.from[s]; B[s] = ws + l.to[s];
    }
    // The flow of a scale lies in one of two buffers, the caller's `flow` (0) and the workspace's (1).  A warp of an odd
    // number of sweeps leaves it in the other one, and so does a prolongation; the coarsest scale starts where the finest ends in `flow`.
    float* buf[2] = {flow, ws + l.other};
    const int flip = (iterations & 1) & (warps & 1);      // buffers changed by the warps of one scale, mod 2
    int cur = flip ? 1 : ((S - 1) & 1);
    hipError_t e = hipMemsetAsync(buf[cur], 0, 2 * (size_t)l.h[S - 1] * l.w[S - 1] * sizeof(float), stream);
    if (e != hipSuccess) return e;
    for (int s = S - 1; s >= 0; --s) {
        const int h = l.h[s], w = l.w[s];
        const size_t hw = (size_t)h * w;
        for (int k = 0; k < warps; ++k) {
            e = launch_flow_linearize(A[s], B[s], buf[cur], buf[cur] + hw, h, w, ws + l.ix, ws + l.iy, ws + l.rho, stream);
            if (e != hipSuccess) return e;
            // an even count ends where it began (the first step then writes the other buffer), an odd one in the other buffer
            float* out = (iterations & 1) ? buf[cur ^ 1] : buf[cur];
            float* tmp = (iterations & 1) ? buf[cur] : buf[cur ^ 1];
            if (iterations == 1) tmp = nullptr;
            e = launch_flow_sweeps(ws + l.ix, ws + l.iy, ws + l.rho, buf[cur], h, w, alpha2, iterations, out, tmp, stream);
            if (e != hipSuccess) return e;
            cur ^= iterations & 1;
        }
        if (s > 0) {
            e = launch_flow_prolong(buf[cur], l.h[s - 1], l.w[s - 1], buf[cur ^ 1], stream);
            if (e != hipSuccess) return e;
            cur ^= 1;
        }
    }
    return cur == 0 ? hipSuccess : hipErrorUnknown;
}

}  // namespace nst
