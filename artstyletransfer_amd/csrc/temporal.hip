// temporal.hip - what a sequence needs on top of the still-image job (Ruder, Dosovitskiy & Brox, "Artistic Style Transfer for
// Videos", GCPR 2016; include/nst_hip.h has the normative definitions): a pixel-space term that holds the level image to an
// anchor under a per-pixel weight plane, the bilinear warp that makes the anchor from the previous frame's result, and the
// weight plane from a forward / backward flow pair (section 4 of the paper, after Sundaram, Brox & Keutzer 2010).
//   anchor_kernel<false>   the forward half: ANCHOR_BLOCKS double partials of c d^2, d = y - a
//   anchor_kernel<true>    the backward half: grad (+)= coef * (c * d); d is formed again, no residual goes through HBM
//   anchor_value_kernel    the block partials -> tmp (the standalone entry point; the loss rows read the partials)
//   warp_kernel            out = bilinear(src, p + flow(p)), valid = the four taps lie inside the image
//   flow_weights_kernel    c = 0 at disocclusions, motion boundaries and samples off the image, 1 elsewhere
//   anchor_fold_kernel     several warped results under their weight planes -> the one anchor and weight plane of a level
// Streaming kernels: 16 bytes per lane where a plane's offset keeps every operand on a 16-byte boundary, scalar loads on
// such a plane's last h w % 4 pixels and on the planes that are not.  The grid of the anchor kernels is fixed, every thread
// adds its share in index order, and the block tree is the one of pixel_ops.hip: no float atomics, the same bits every run.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "nst_kernels.h"
#include "nst_sample.h"   // axis_tap, bilinear: the position rule the warp, the flow weights and flow.hip share

namespace nst {

namespace {

constexpr int ANCHOR_THREADS = 256;
constexpr int ANCHOR_VEC = 4;               // pixels of one lane's 16-byte load

__device__ __forceinline__ double anchor_block_sum(double v, double* sh) {
    // 256 threads; fixed tree order (pixel_ops.hip's block_reduce_sum)
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < 4; ++i) r += sh[i];
    __syncthreads();
    return r;   // valid in thread 0
}

// one pixel of the backward half: coef * (c * d), product by product (the caller switches contraction off); a term of
// exactly zero (d = 0, c = 0) leaves the gradient's bits alone, the sign of a zero included
__device__ __forceinline__ float anchor_grad(float g, float y, float a, float c, bool has_c, float coef, int accumulate) {
#pragma clang fp contract(off)
    const float d = y - a;
    const float t = has_c ? c * d : d;
    const float term = coef * t;
    if (!accumulate) return term;
    return term != 0.f ? g + term : g;
}

}  // namespace

// y, a (C,hw), c (hw) or nullptr = ones.  vec_mask bit ch: plane ch of y, a (and grad) and c start on 16-byte boundaries.
// GRAD = false: partial[block] = sum of c d^2 over the block's share (channel by channel: quads, then the scalar pixels)
// GRAD = true: grad (+)= coef * (c * d)
template <bool GRAD>
__global__ __launch_bounds__(ANCHOR_THREADS) void anchor_kernel(const float* __restrict__ y, const float* __restrict__ a,
                                                                const float* __restrict__ c, int C, size_t hw, unsigned vec_mask,
                                                                double* __restrict__ partial, float coef, float* __restrict__ grad,
                                                                int accumulate) {
    __shared__ double sh[4];
    const size_t tid = (size_t)blockIdx.x * ANCHOR_THREADS + threadIdx.x;
    const size_t nthreads = (size_t)gridDim.x * ANCHOR_THREADS;
    const bool has_c = c != nullptr;
    double acc = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        const float* yc = y + (size_t)ch * hw;
        const float* ac = a + (size_t)ch * hw;
        float* gc = GRAD ? grad + (size_t)ch * hw : nullptr;
        const size_t nq = ((vec_mask >> ch) & 1u) ? hw / ANCHOR_VEC : 0;
        for (size_t q = tid; q < nq; q += nthreads) {
            const float4 yv = reinterpret_cast<const float4*>(yc)[q];
            const float4 av = reinterpret_cast<const float4*>(ac)[q];
            const float4 cv = has_c ? reinterpret_cast<const float4*>(c)[q] : make_float4(1.f, 1.f, 1.f, 1.f);
            if (GRAD) {
                float4 gv = accumulate ? reinterpret_cast<const float4*>(gc)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
                gv.x = anchor_grad(gv.x, yv.x, av.x, cv.x, has_c, coef, accumulate);
                gv.y = anchor_grad(gv.y, yv.y, av.y, cv.y, has_c, coef, accumulate);
                gv.z = anchor_grad(gv.z, yv.z, av.z, cv.z, has_c, coef, accumulate);
                gv.w = anchor_grad(gv.w, yv.w, av.w, cv.w, has_c, coef, accumulate);
                reinterpret_cast<float4*>(gc)[q] = gv;
            } else {
                const double d0 = (double)yv.x - (double)av.x, d1 = (double)yv.y - (double)av.y;
                const double d2 = (double)yv.z - (double)av.z, d3 = (double)yv.w - (double)av.w;
                acc += (double)cv.x * (d0 * d0);
                acc += (double)cv.y * (d1 * d1);
                acc += (double)cv.z * (d2 * d2);
                acc += (double)cv.w * (d3 * d3);
            }
        }
        for (size_t p = nq * ANCHOR_VEC + tid; p < hw; p += nthreads) {
            const float cp = has_c ? c[p] : 1.f;
            if (GRAD) {
                gc[p] = anchor_grad(accumulate ? gc[p] : 0.f, yc[p], ac[p], cp, has_c, coef, accumulate);
            } else {
                const double d = (double)yc[p] - (double)ac[p];
                acc += (double)cp * (d * d);
            }
        }
    }
    if (!GRAD) {
        const double b = anchor_block_sum(acc, sh);
        if (threadIdx.x == 0) partial[blockIdx.x] = b;
    }
}

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// bit ch: plane ch of every (C,hw) operand, and the weight plane, start on a 16-byte boundary
unsigned anchor_vec_mask(const float* y, const float* a, const float* c, const float* grad, int C, size_t hw) {
    unsigned m = 0;
    if (c && !aligned16(c)) return 0;
    for (int ch = 0; ch < C; ++ch) {
        const size_t o = (size_t)ch * hw;
        if (aligned16(y + o) && aligned16(a + o) && (!grad || aligned16(grad + o))) m |= 1u << ch;
    }
    return m;
}

}  // namespace

int anchor_block_elems() { return ANCHOR_THREADS * ANCHOR_VEC; }

hipError_t launch_anchor_forward(const float* y, const float* a, const float* c, int C, int h, int w, double* partial,
                                 hipStream_t stream) {
    if ((C != 1 && C != 3) || h < 1 || w < 1 || !y || !a || !partial) return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    hipLaunchKernelGGL(anchor_kernel<false>, dim3(ANCHOR_BLOCKS), dim3(ANCHOR_THREADS), 0, stream, y, a, c, C, hw,
                       anchor_vec_mask(y, a, c, nullptr, C, hw), partial, 0.f, nullptr, 0);
    return hipGetLastError();
}

hipError_t launch_anchor_backward(const float* y, const float* a, const float* c, int C, int h, int w, float coef, float* grad,
                                  int accumulate, hipStream_t stream) {
    if ((C != 1 && C != 3) || h < 1 || w < 1 || !y || !a || !grad) return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    // (no reduction here: enough blocks to cover the image once, capped where the forward half's grid is)
    const size_t want = (hw / ANCHOR_VEC + ANCHOR_THREADS) / ANCHOR_THREADS;
    const int blocks = (int)(want < (size_t)ANCHOR_BLOCKS ? want : (size_t)ANCHOR_BLOCKS);
    hipLaunchKernelGGL(anchor_kernel<true>, dim3(blocks), dim3(ANCHOR_THREADS), 0, stream, y, a, c, C, hw,
                       anchor_vec_mask(y, a, c, grad, C, hw), nullptr, coef, grad, accumulate);
    return hipGetLastError();
}

// ------------------------------------------------------------------ tmp = (float)(sum of the block partials / n)
// thread t adds the partials t, t + 256, ... in index order, then the fixed tree: the order of loss_rows_kernel
__global__ __launch_bounds__(256) void anchor_value_kernel(const double* __restrict__ partial, int blocks, double n, float* __restrict__ out) {
    __shared__ double sh[4];
    double v = 0.0;
    for (int b = threadIdx.x; b < blocks; b += 256) v += partial[b];
    const double r = anchor_block_sum(v, sh);
    if (threadIdx.x == 0) out[0] = (float)(r / n);
}
hipError_t launch_anchor_value(const double* partial, int blocks, double n, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(anchor_value_kernel, dim3(1), dim3(256), 0, stream, partial, blocks, n, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ warp
__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ src, const float* __restrict__ flow, int C, int h, int w,
                                                   float* __restrict__ out, float* __restrict__ valid) {
    const size_t hw = (size_t)h * w;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
        const float dx = flow[p], dy = flow[hw + p];
        if (!(isfinite(dx) && isfinite(dy))) {
            for (int ch = 0; ch < C; ++ch) out[(size_t)ch * hw + p] = src[(size_t)ch * hw + p];
            if (valid) valid[p] = 0.f;
            continue;
        }
        const AxisTap ax = axis_tap(x, dx, w), ay = axis_tap(y, dy, h);
        for (int ch = 0; ch < C; ++ch) out[(size_t)ch * hw + p] = bilinear(src + (size_t)ch * hw, w, ax, ay);
        if (valid) valid[p] = (ax.inside && ay.inside) ? 1.f : 0.f;
    }
}
hipError_t launch_warp_bilinear(const float* src, const float* flow, int C, int h, int w, float* out, float* valid,
                                hipStream_t stream) {
    if (C < 1 || h < 1 || w < 1 || !src || !flow || !out) return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    const size_t want = (hw + 255) / 256;
    hipLaunchKernelGGL(warp_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, stream, src, flow, C, h, w, out, valid);
    return hipGetLastError();
}

// ------------------------------------------------------------------ flow weights
// fwd, bwd (2,h,w): plane 0 = u (x), plane 1 = v (y).  Every comparison in fp32, one rounding per operation.
__global__ __launch_bounds__(256) void flow_weights_kernel(const float* __restrict__ fwd, const float* __restrict__ bwd, int h, int w,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t hw = (size_t)h * w;
    const float* bu_p = bwd;
    const float* bv_p = bwd + hw;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
        const float bu = bu_p[p], bv = bv_p[p];
        if (!(isfinite(bu) && isfinite(bv))) { out[p] = 0.f; continue; }
        const AxisTap ax = axis_tap(x, bu, w), ay = axis_tap(y, bv, h);
        bool ok = ax.inside && ay.inside;
        // w~ = fwd at p + bwd(p)
        const float wu = bilinear(fwd, w, ax, ay), wv = bilinear(fwd + hw, w, ax, ay);
        const float bb = bu * bu + bv * bv;
        // disocclusion: |w~ + bwd|^2 > 0.01 (|w~|^2 + |bwd|^2) + 0.5
        {
            const float su = wu + bu, sv = wv + bv;
            const float lhs = su * su + sv * sv;
            const float rhs = 0.01f * ((wu * wu + wv * wv) + bb) + 0.5f;
            ok = ok && lhs <= rhs;        // (a NaN on either side: not reliable)
        }
        // motion boundary: |grad u|^2 + |grad v|^2 > 0.01 |bwd|^2 + 0.002, central differences with replicated borders
        {
            const int xm = max(x - 1, 0), xp = min(x + 1, w - 1), ym = max(y - 1, 0), yp = min(y + 1, h - 1);
            const size_t row = (size_t)y * w;
            const float ux = 0.5f * (bu_p[row + xp] - bu_p[row + xm]);
            const float uy = 0.5f * (bu_p[(size_t)yp * w + x] - bu_p[(size_t)ym * w + x]);
            const float vx = 0.5f * (bv_p[row + xp] - bv_p[row + xm]);
            const float vy = 0.5f * (bv_p[(size_t)yp * w + x] - bv_p[(size_t)ym * w + x]);
            const float lhs = (ux * ux + uy * uy) + (vx * vx + vy * vy);
            const float rhs = 0.01f * bb + 0.002f;
            ok = ok && lhs <= rhs;
        }
        out[p] = ok ? 1.f : 0.f;
    }
}
hipError_t launch_flow_weights(const float* fwd, const float* bwd, int h, int w, float* out, hipStream_t stream) {
    if (h < 1 || w < 1 || !fwd || !bwd || !out) return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    const size_t want = (hw + 255) / 256;
    hipLaunchKernelGGL(flow_weights_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, stream, fwd, bwd, h, w, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ anchor fold (the long-term anchor)
// J warped results under J reliability planes -> the ONE anchor and weight plane a level holds (include/nst_hip.h,
// nst_anchor_fold).  A lane owns four consecutive pixels: the weights give l_j, Wsum and the live set once, then channel by
// channel the sources are mixed.  Every plane is read or written 16 bytes at a time where its bit of the mask is set and the
// lane's four pixels exist, pixel by pixel otherwise.  A source none of the lane's pixels takes is not loaded; one that a
// neighbour takes is loaded and dropped by a select, never by a product - its non-finite values do not leak.
namespace {

constexpr int FOLD_THREADS = 256;
constexpr unsigned FOLD_VEC_WEIGHTS = 1u << 3;     // bits 0..2: plane ch of every source and of the anchor
constexpr unsigned FOLD_VEC_PARTS = 1u << 8;       // bit 8 + j: plane j of parts

__device__ __forceinline__ void fold_load4(const float* __restrict__ p, size_t at, bool vec, int n, float v[4]) {
    if (vec) {
        const float4 t = *reinterpret_cast<const float4*>(p + at);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < n ? p[at + k] : 0.f;
    }
}
__device__ __forceinline__ void fold_store4(float* __restrict__ p, size_t at, bool vec, int n, const float v[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(p + at) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[at + k] = v[k];
    }
}

}  // namespace

__global__ __launch_bounds__(FOLD_THREADS) void anchor_fold_kernel(const AnchorFoldArgs a, int J, int C, size_t hw, unsigned vec_mask,
                                                                   float* __restrict__ anchor, float* __restrict__ weight,
                                                                   float* __restrict__ parts) {
#pragma clang fp contract(off)
    const size_t nq = (hw + 3) / 4;
    for (size_t q = (size_t)blockIdx.x * FOLD_THREADS + threadIdx.x; q < nq; q += (size_t)gridDim.x * FOLD_THREADS) {
        const size_t at = q * 4;
        const int n = hw - at >= 4 ? 4 : (int)(hw - at);
        const bool full = n == 4;
        // r[j][k]: l_j of pixel k, then l_j / Wsum; live bit 4 j + k: l_j > 0
        float r[NST_FOLD_MAX_SOURCES][4], s[4] = {0.f, 0.f, 0.f, 0.f}, wsum[4] = {0.f, 0.f, 0.f, 0.f};
        unsigned live = 0;
#pragma unroll
        for (int j = 0; j < NST_FOLD_MAX_SOURCES; ++j) {
            if (j < J) {
                float wv[4];
                fold_load4(a.weights[j], at, full && (vec_mask & FOLD_VEC_WEIGHTS), n, wv);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float c = wv[k] > 0.f ? fminf(wv[k], 1.f) : 0.f;      // NaN, negative: 0
                    const float l = fmaxf(c - s[k], 0.f);
                    s[k] = s[k] + c;
                    wsum[k] = j == 0 ? l : wsum[k] + l;
                    r[j][k] = l;
                    if (l > 0.f) live |= 1u << (4 * j + k);
                }
                if (parts) fold_store4(parts + (size_t)j * hw, at, full && ((vec_mask >> j) & FOLD_VEC_PARTS), n, r[j]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) r[j][k] = 0.f;
            }
        }
        unsigned none = 0;                  // bit k: no source is live at pixel k
        {
            float wo[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(wsum[k] > 0.f)) none |= 1u << k;
                wo[k] = fminf(wsum[k], 1.f);
            }
            fold_store4(weight, at, full && (vec_mask & FOLD_VEC_WEIGHTS), n, wo);
        }
#pragma unroll
        for (int j = 1; j < NST_FOLD_MAX_SOURCES; ++j)      // (source 0, where live, is the base: its ratio is never read)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((live >> (4 * j + k)) & 1u) r[j][k] = r[j][k] / wsum[k];
        for (int ch = 0; ch < C; ++ch) {
            const bool vec = full && ((vec_mask >> ch) & 1u);
            const size_t o = (size_t)ch * hw + at;
            float base[4] = {0.f, 0.f, 0.f, 0.f}, acc[4] = {0.f, 0.f, 0.f, 0.f};
            unsigned have = 0;          // bit k: pixel k has its base, the first live source (source 0 where none is)
#pragma unroll
            for (int j = 0; j < NST_FOLD_MAX_SOURCES; ++j) {
                const unsigned lj = ((live >> (4 * j)) & 15u) | (j == 0 ? none : 0u);
                if (j < J && lj) {
                    float v[4];
                    fold_load4(a.sources[j], o, vec, n, v);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool on = (lj >> k) & 1u, first = !((have >> k) & 1u);
                        const float next = acc[k] + r[j][k] * (v[k] - base[k]);
                        if (on && first) base[k] = v[k];
                        acc[k] = on ? (first ? v[k] : next) : acc[k];
                    }
                    have |= lj;
                }
            }
            fold_store4(anchor, o, vec, n, acc);
        }
    }
}

unsigned anchor_fold_vec_mask(const AnchorFoldArgs& a, int J, int C, size_t hw, const float* anchor, const float* weight,
                              const float* parts) {
    unsigned m = 0;
    bool wv = aligned16(weight);
    for (int j = 0; j < J; ++j) wv = wv && aligned16(a.weights[j]);
    if (wv) m |= FOLD_VEC_WEIGHTS;
    for (int ch = 0; ch < C; ++ch) {
        const size_t o = (size_t)ch * hw;
        bool v = aligned16(anchor + o);
        for (int j = 0; j < J; ++j) v = v && aligned16(a.sources[j] + o);
        if (v) m |= 1u << ch;
    }
    if (parts)
        for (int j = 0; j < J; ++j)
            if (aligned16(parts + (size_t)j * hw)) m |= FOLD_VEC_PARTS << j;
    return m;
}

hipError_t launch_anchor_fold(const AnchorFoldArgs& a, int J, int C, int h, int w, float* anchor, float* weight, float* parts,
                              hipStream_t stream) {
    if (J < 1 || J > NST_FOLD_MAX_SOURCES || (C != 1 && C != 3) || h < 1 || w < 1 || !anchor || !weight) return hipErrorInvalidValue;
    for (int j = 0; j < J; ++j)
        if (!a.sources[j] || !a.weights[j]) return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    const size_t want = ((hw + 3) / 4 + FOLD_THREADS - 1) / FOLD_THREADS;
    hipLaunchKernelGGL(anchor_fold_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(FOLD_THREADS), 0, stream, a, J, C, hw,
                       anchor_fold_vec_mask(a, J, C, hw, anchor, weight, parts), anchor, weight, parts);
    return hipGetLastError();
}

}  // namespace nst
