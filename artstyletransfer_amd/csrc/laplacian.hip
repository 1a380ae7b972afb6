// laplacian.hip - the Laplacian loss (Li, Xu, Nikolova & He, "Laplacian-Steered Neural Style Transfer", ACM MM 2017;
// include/nst_hip.h has the definition): a pixel-space term of the closure that reads the level image and adds into the
// level gradient, as total variation does.  Three HBM streams and one scalar kernel:
//   lap_pool_kernel     (C,h,w) -> s (hk,wk): the sum over the channels of the p x p mean pool, cell sums in double and
//                       kept in double (near +-120 an fp32 s loses the digits the stencil then needs)
//   lap_stencil_kernel  s -> D s (- target): the valid 3x3 stencil, the residual and its double SSE partials; without a
//                       target it makes the target itself
//   lap_bwd_kernel      one pass over the level gradient: every pixel adds coef_k (D^T r_k)(its cell) of every entry
//   lap_value_kernel    the partials -> lap_k (the standalone entry point; the closure's loss rows read the partials)
// No float atomics; every sum has a fixed order (the cell sums are exact in double whatever their order: at most 3 x 32 x 32
// fp32 values), so a closure with the term stays bitwise reproducible.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "nst_kernels.h"

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int LAP_TX = 64;     // threads along x of the pool kernel (VEC columns each)
constexpr int LAP_TY = 4;      // row groups of the pool kernel: group ty takes the rows r = ty, ty + 4, ... of every cell row

__device__ __forceinline__ double lap_block_sum(double v, double* sh) {
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

}  // namespace

// ------------------------------------------------------------------ pool-sum: s(a,b) = mult * sum_c sum_cell y_c / p^2
// grid = (column tiles, hk); a workgroup owns pooled row blockIdx.y and tile_w image columns (a multiple of p and of VEC):
// thread (tx, ty) adds the rows r = ty (mod 4) of its VEC columns over the channels (coalesced, 16-byte loads when VEC = 4),
// the column sums meet in LDS, and one thread per cell adds its p columns.  No division in the streaming loop.
template <int VEC>
__global__ __launch_bounds__(256) void lap_pool_kernel(const float* __restrict__ y, int C, int h, int w, int p, int wk,
                                                       int tile_w, double mult, double* __restrict__ s) {
    __shared__ double col[LAP_TY][LAP_TX * VEC];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int a = blockIdx.y;
    const int x0 = blockIdx.x * tile_w;
    const int xe = min(x0 + tile_w, wk * p);       // (a multiple of p; columns beyond it belong to no cell)
    const int x = x0 + tx * VEC;
    double acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
    if (x < xe) {                                  // (VEC = 4: w % 4 == 0 and x % 4 == 0, so x + 3 < w)
        for (int c = 0; c < C; ++c) {
            const float* line = y + ((size_t)c * h + (size_t)a * p + ty) * w + x;
#pragma unroll 4
            for (int r = ty; r < p; r += LAP_TY, line += (size_t)LAP_TY * w) {
                if (VEC == 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(line);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] += (double)q[v];
                } else {
                    acc[0] += (double)line[0];
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) col[ty][tx * VEC + v] = acc[v];
    __syncthreads();
    const int t = ty * LAP_TX + tx;
    const int ncell = (xe - x0) / p;
    if (t < ncell) {
        double sum = 0.0;
        for (int q = 0; q < p; ++q)
            for (int g = 0; g < LAP_TY; ++g) sum += col[g][t * p + q];
        s[(size_t)a * wk + x0 / p + t] = mult * sum / (double)(p * p);      // (the sum is exact: one rounding, in double)
    }
}

hipError_t launch_lap_pool(const float* y, int C, int h, int w, int p, double* s, hipStream_t stream) {
    const int hk = h / p, wk = w / p;
    if (p < 1 || p > 32 || hk < 1 || wk < 1 || (C != 1 && C != 3)) return hipErrorInvalidValue;
    const double mult = C == 1 ? 3.0 : 1.0;        // luminance: the three channels of E(u) pool to the same value
    const bool vec = (w % 4 == 0) && ((uintptr_t)y % 16 == 0);
    if (vec) {
        const int tile_w = (LAP_TX * 4 / (4 * p)) * (4 * p);
        const dim3 grid((wk * p + tile_w - 1) / tile_w, hk);
        hipLaunchKernelGGL(lap_pool_kernel<4>, grid, dim3(LAP_TX, LAP_TY), 0, stream, y, C, h, w, p, wk, tile_w, mult, s);
    } else {
        const int tile_w = (LAP_TX / p) * p;
        const dim3 grid((wk * p + tile_w - 1) / tile_w, hk);
        hipLaunchKernelGGL(lap_pool_kernel<1>, grid, dim3(LAP_TX, LAP_TY), 0, stream, y, C, h, w, p, wk, tile_w, mult, s);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ stencil, residual, SSE partials
// target == nullptr: target_out (hk-2, wk-2) = D s, in double (the content side).  Else r (hk-2, wk-2) = (float)(D s - target),
// rounded once, and partial: LAP_BLOCKS doubles, partial[b] = sum of r^2 over the rows b, b + LAP_BLOCKS, ... in a fixed
// order.
__global__ __launch_bounds__(256) void lap_stencil_kernel(const double* __restrict__ s, int hk, int wk,
                                                          const double* __restrict__ target, double* __restrict__ target_out,
                                                          float* __restrict__ r, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int oh = hk - 2, ow = wk - 2;
    double acc = 0.0;
    for (int i = blockIdx.x; i < oh; i += gridDim.x) {
        const double* r0 = s + (size_t)i * wk;
        const double* r1 = r0 + wk;
        const double* r2 = r1 + wk;
        for (int j = threadIdx.x; j < ow; j += blockDim.x) {
            const double d = 4.0 * r1[j + 1] - r0[j + 1] - r2[j + 1] - r1[j] - r1[j + 2];
            const size_t o = (size_t)i * ow + j;
            if (target) {
                const float v = (float)(d - target[o]);
                acc += (double)v * (double)v;
                r[o] = v;
            } else {
                target_out[o] = d;
            }
        }
    }
    if (!partial) return;
    const double b = lap_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = b;
}

hipError_t launch_lap_stencil(const double* s, int hk, int wk, const double* target, double* target_out, float* r, double* partial,
                              hipStream_t stream) {
    if (hk < 3 || wk < 3) return hipErrorInvalidValue;
    if (target ? (!r || !partial) : !target_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lap_stencil_kernel, dim3(LAP_BLOCKS), dim3(256), 0, stream, s, hk, wk, target, target_out, r, partial);
    return hipGetLastError();
}

// ------------------------------------------------------------------ lap_k = (float)(sum of the partials / n)
__global__ __launch_bounds__(256) void lap_value_kernel(const double* __restrict__ partial, double n, float* __restrict__ out) {
    __shared__ double sh[4];
    const double r = lap_block_sum(threadIdx.x < LAP_BLOCKS ? partial[threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) out[0] = (float)(r / n);
}
hipError_t launch_lap_value(const double* partial, double n, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(lap_value_kernel, dim3(1), dim3(256), 0, stream, partial, n, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ backward: grad (+)= sum_k coef_k (D^T r_k)(i / p, j / p)
// D^T r at cell (a,b) = 4 r(a-1,b-1) - r(a-2,b-1) - r(a,b-1) - r(a-1,b-2) - r(a-1,b), r zero outside its (hk-2, wk-2).
__device__ __forceinline__ float lap_dt(const float* __restrict__ r, int oh, int ow, int a, int b) {
    auto at = [&](int aa, int bb) -> double {
        return ((unsigned)aa < (unsigned)oh && (unsigned)bb < (unsigned)ow) ? (double)r[(size_t)aa * ow + bb] : 0.0;
    };
    return (float)(4.0 * at(a - 1, b - 1) - at(a - 2, b - 1) - at(a, b - 1) - at(a - 1, b - 2) - at(a - 1, b));
}

// grid = (column blocks, row groups): a thread keeps its VEC columns (their cell columns b_k are computed once, by a
// multiply-high with ceil(2^32 / p): no division per element) and walks the image rows of its row group; the entries are
// added in ascending k, product and sum each rounded.  Ragged last rows / columns belong to no cell: they get nothing
// (accumulate = 0: zero).
template <int VEC>
__global__ __launch_bounds__(256) void lap_bwd_kernel(LapBackward lb, int C, int h, int w, float* __restrict__ grad,
                                                      int accumulate) {
#pragma clang fp contract(off)
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * VEC;
    if (x >= w) return;
    int b[NST_LAP_MAX][VEC];
#pragma unroll
    for (int k = 0; k < NST_LAP_MAX; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const unsigned xv = (unsigned)(x + v);
            const int cell = (k < lb.K) ? (lb.p[k] == 1 ? (int)xv : (int)__umulhi(xv, lb.magic[k])) : 0;
            b[k][v] = (k < lb.K && cell < lb.wk[k]) ? cell : -1;
        }
    for (int row = blockIdx.y; row < C * h; row += gridDim.y) {
        const int i = row % h;
        float* g = grad + (size_t)row * w + x;
        float val[VEC];
        if (accumulate) {
            if (VEC == 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(g);
#pragma unroll
                for (int v = 0; v < VEC; ++v) val[v] = q[v];
            } else {
                val[0] = g[0];
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) val[v] = 0.f;
        }
#pragma unroll
        for (int k = 0; k < NST_LAP_MAX; ++k) {
            if (k >= lb.K) break;
            const int a = i / lb.p[k];                        // (once per row and entry)
            if (a >= lb.hk[k]) continue;
            const int oh = lb.hk[k] - 2, ow = lb.wk[k] - 2;
            float dt = 0.f;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (b[k][v] < 0) continue;
                if (v == 0 || b[k][v] != b[k][v - 1]) dt = lap_dt(lb.r[k], oh, ow, a, b[k][v]);
                val[v] = val[v] + lb.coef[k] * dt;
            }
        }
        if (VEC == 4) {
            f32x4 q;
#pragma unroll
            for (int v = 0; v < VEC; ++v) q[v] = val[v];
            *reinterpret_cast<f32x4*>(g) = q;
        } else {
            g[0] = val[0];
        }
    }
}

hipError_t launch_lap_backward(const LapBackward& in, int C, int h, int w, float* grad, int accumulate, hipStream_t stream) {
    if (in.K < 1 || in.K > NST_LAP_MAX) return hipErrorInvalidValue;
    LapBackward lb = in;
    for (int k = 0; k < lb.K; ++k) {
        if (lb.p[k] < 1 || lb.p[k] > 32) return hipErrorInvalidValue;
        lb.hk[k] = h / lb.p[k]; lb.wk[k] = w / lb.p[k];
        if (lb.hk[k] < 3 || lb.wk[k] < 3) return hipErrorInvalidValue;
        lb.magic[k] = lb.p[k] == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)lb.p[k] - 1) / (unsigned)lb.p[k]);
    }
    const int all_rows = C * h;
    const int gy = all_rows < 768 ? all_rows : 768;
    const bool vec = (w % 4 == 0) && ((uintptr_t)grad % 16 == 0);
    if (vec)
        hipLaunchKernelGGL(lap_bwd_kernel<4>, dim3((w / 4 + 255) / 256, gy), dim3(256), 0, stream, lb, C, h, w, grad, accumulate);
    else
        hipLaunchKernelGGL(lap_bwd_kernel<1>, dim3((w + 255) / 256, gy), dim3(256), 0, stream, lb, C, h, w, grad, accumulate);
    return hipGetLastError();
}

}  // namespace nst
