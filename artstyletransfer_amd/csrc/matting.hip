// matting.hip - the photorealism regulariser of Luan, Paris, Shechtman & Bala ("Deep Photo Style Transfer", CVPR 2017): the
// quadratic form of Levin's matting Laplacian over the 3x3 windows of the level image, guided by the level's content
// (include/nst_hip.h has the definition).  A pixel-space term of the closure, beside total variation and the Laplacian loss.
//   mat_window_kernel<C, false>  the forward half: E_k of every window -> one double partial per tile (fixed order)
//   mat_window_kernel<C, true>   the backward half: the windows of a tile and of its two-pixel halo once more, their
//                                coefficients (mu_k, a_kc, mean V) in LDS in double, and every pixel of the tile gathers
//                                the residuals of its (up to nine) windows and adds coef * sum into the level gradient
//   mat_value_kernel             the tile partials -> mat (the standalone entry point; the loss rows read the partials)
// Nothing of a window goes through HBM: the per-window coefficients would have to be stored in double (a_kc reaches the
// hundreds where the guide is flat, and a^T I cancels against mean V), 120 bytes per window written and read again; the
// recomputation is a few hundred fp64 operations.  Per window the moments, the 3x3 solve (LDL^T of the SPD M_k, no stored
// inverse) and E are formed in double; the gradient is rounded once.  No float atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "nst_kernels.h"

namespace nst {

namespace {

constexpr int MAT_TW = 32;                  // tile: MAT_TW x MAT_TH windows (value) or pixels (gradient), one per thread
constexpr int MAT_TH = 8;
constexpr int MAT_SW = MAT_TW + 4;          // staged pixels of the gradient tile (two-pixel halo); the value tile uses + 2
constexpr int MAT_SH = MAT_TH + 4;
constexpr int MAT_NWIN = (MAT_TW + 2) * (MAT_TH + 2);      // windows of the gradient tile

__device__ __forceinline__ double mat_block_sum(double v, double* sh) {
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

// LDL^T of the symmetric positive definite M = (m00 m01 m02; . m11 m12; . . m22).  Every pivot of M_k is a Schur complement
// of a matrix whose smallest eigenvalue is floor = epsilon / 9: the clamp changes nothing in exact arithmetic and keeps a
// pivot that rounding pushed below the floor from flipping the solve.
struct MatLdl {
    double l1, l2, l3, i0, i1, i2;
    __device__ __forceinline__ void factor(double m00, double m01, double m02, double m11, double m12, double m22, double floor) {
        const double d0 = fmax(m00, floor);
        i0 = 1.0 / d0;
        l1 = m01 * i0; l2 = m02 * i0;
        const double d1 = fmax(m11 - l1 * m01, floor);
        i1 = 1.0 / d1;
        const double t12 = m12 - l1 * m02;
        l3 = t12 * i1;
        const double d2 = fmax(m22 - l2 * m02 - l3 * t12, floor);
        i2 = 1.0 / d2;
    }
    __device__ __forceinline__ void solve(double v0, double v1, double v2, double& x0, double& x1, double& x2) const {
        const double z1 = v1 - l1 * v0;
        const double z2 = v2 - l2 * v0 - l3 * z1;
        x2 = z2 * i2;
        x1 = z1 * i1 - l3 * x2;
        x0 = v0 * i0 - l1 * x1 - l2 * x2;
    }
};

}  // namespace

// y (C,h,w): the level image; guide (C,h,w): I * 255 up to a constant per channel when gscale = 1 / 255 (the level's prepared
// content), I itself when gscale = 1 (only differences inside a window enter).  C = 1: the scalar reduction of the
// three-equal-channel guide, epsilon / 3 in place of epsilon.
// GRAD = false: grid = tiles of windows; partial[tile] = sum over the tile's windows (and channels) of E.
// GRAD = true: grid = tiles of pixels; grad (+)= coef * sum over the windows of a pixel of (Vc_i - a^T Ic_i).
template <int C, bool GRAD>
__global__ __launch_bounds__(256) void mat_window_kernel(const float* __restrict__ y, const float* __restrict__ guide, int h, int w,
                                                         double gscale, double eps, double* __restrict__ partial, float coef,
                                                         float* __restrict__ grad, int accumulate) {
    constexpr int HALO = GRAD ? 2 : 0;
    constexpr int SW = MAT_TW + 2 + HALO, SH = MAT_TH + 2 + HALO;       // staged pixels
    constexpr int WW = SW - 2, WH = SH - 2;                              // windows (top-left corners) of the tile
    constexpr int NREC = C == 3 ? 15 : 3;                                // doubles of a window's record
    __shared__ float sy[C][MAT_SH][MAT_SW];
    __shared__ float sg[C][MAT_SH][MAT_SW];
    __shared__ double rec[GRAD ? NREC * MAT_NWIN : 1];
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const int ox = blockIdx.x * MAT_TW - HALO, oy = blockIdx.y * MAT_TH - HALO;   // image position of the staged origin
    for (int i = tid; i < C * SH * SW; i += 256) {
        const int c = i / (SH * SW), r = (i / SW) % SH, q = i % SW;
        const int gy = oy + r, gx = ox + q;
        const bool in = (unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w;
        const size_t o = ((size_t)c * h + (in ? gy : 0)) * w + (in ? gx : 0);
        sy[c][r][q] = in ? y[o] : 0.f;
        sg[c][r][q] = in ? guide[o] : 0.f;
    }
    __syncthreads();
    // (1/9 and 1/255 as factors: an fp64 division costs tens of instructions, a window has twenty of them, and one more
    // rounding at 1e-16 is far below what the fp32 results keep)
    const double inv255 = 1.0 / 255.0, inv9 = 1.0 / 9.0;
    double acc = 0.0;
    for (int wi = tid; wi < WH * WW; wi += 256) {
        const int wr = wi / WW, wc = wi % WW;
        const int gy = oy + wr, gx = ox + wc;
        if (gy < 0 || gx < 0 || gy > h - 3 || gx > w - 3) continue;      // (no window here: nothing reads its record)
        if (C == 3) {
            double ic[3][9], mu[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double sum = 0.0;
#pragma unroll
                for (int p = 0; p < 9; ++p) { ic[c][p] = (double)sg[c][wr + p / 3][wc + p % 3]; sum += ic[c][p]; }
                mu[c] = sum * inv9;
#pragma unroll
                for (int p = 0; p < 9; ++p) ic[c][p] = (ic[c][p] - mu[c]) * gscale;
            }
            double m[6] = {0, 0, 0, 0, 0, 0};      // 00 01 02 11 12 22
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                m[0] += ic[0][p] * ic[0][p]; m[1] += ic[0][p] * ic[1][p]; m[2] += ic[0][p] * ic[2][p];
                m[3] += ic[1][p] * ic[1][p]; m[4] += ic[1][p] * ic[2][p]; m[5] += ic[2][p] * ic[2][p];
            }
            const double e9 = eps * inv9;
            MatLdl f;
            f.factor(m[0] * inv9 + e9, m[1] * inv9, m[2] * inv9, m[3] * inv9 + e9, m[4] * inv9, m[5] * inv9 + e9, e9);
            if (GRAD) {
#pragma unroll
                for (int c = 0; c < 3; ++c) rec[c * MAT_NWIN + wi] = mu[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double vc[9], sum = 0.0;
#pragma unroll
                for (int p = 0; p < 9; ++p) { vc[p] = (double)sy[c][wr + p / 3][wc + p % 3] * inv255; sum += vc[p]; }
                const double mv = sum * inv9;
                double v0 = 0.0, v1 = 0.0, v2 = 0.0, ss = 0.0;
#pragma unroll
                for (int p = 0; p < 9; ++p) {
                    vc[p] -= mv;
                    ss += vc[p] * vc[p];
                    v0 += vc[p] * ic[0][p]; v1 += vc[p] * ic[1][p]; v2 += vc[p] * ic[2][p];
                }
                double a0, a1, a2;
                f.solve(v0, v1, v2, a0, a1, a2);
                a0 *= inv9; a1 *= inv9; a2 *= inv9;
                if (GRAD) {
                    // residual of pixel i: (V_i - mv) - (a gscale)^T (g_i - mu)
                    double* q = rec + (3 + 4 * c) * MAT_NWIN + wi;
                    q[0] = mv; q[MAT_NWIN] = a0 * gscale; q[2 * MAT_NWIN] = a1 * gscale; q[3 * MAT_NWIN] = a2 * gscale;
                } else {
                    acc += ss - (v0 * a0 + v1 * a1 + v2 * a2);
                }
            }
        } else {
            double gc[9], vc[9], sg1 = 0.0, sv = 0.0;
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                gc[p] = (double)sg[0][wr + p / 3][wc + p % 3]; sg1 += gc[p];
                vc[p] = (double)sy[0][wr + p / 3][wc + p % 3] * inv255; sv += vc[p];
            }
            const double mu = sg1 * inv9, mv = sv * inv9;
            double S = 0.0, t = 0.0, ss = 0.0;
#pragma unroll
            for (int p = 0; p < 9; ++p) {
                gc[p] = (gc[p] - mu) * gscale; vc[p] -= mv;
                S += gc[p] * gc[p]; t += vc[p] * gc[p]; ss += vc[p] * vc[p];
            }
            const double b = t / (S + eps / 3.0);
            if (GRAD) { rec[wi] = mu; rec[MAT_NWIN + wi] = mv; rec[2 * MAT_NWIN + wi] = b * gscale; }
            else acc += ss - t * b;
        }
    }
    if (!GRAD) {
        const double b = mat_block_sum(acc, sh);
        if (tid == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = b;
        return;
    }
    __syncthreads();
    const int ly = tid / MAT_TW, lx = tid % MAT_TW;
    const int py = oy + HALO + ly, px = ox + HALO + lx;
    if (py >= h || px >= w) return;
    double r[C];
#pragma unroll
    for (int c = 0; c < C; ++c) r[c] = 0.0;
    // the windows that hold the pixel: top-left (py - dy, px - dx), in ascending (dy, dx)
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int gy = py - dy;
        if (gy < 0 || gy > h - 3) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int gx = px - dx;
            if (gx < 0 || gx > w - 3) continue;
            const int wi = (ly + HALO - dy) * WW + (lx + HALO - dx);
            if (C == 3) {
                const double d0 = (double)sg[0][ly + HALO][lx + HALO] - rec[wi];
                const double d1 = (double)sg[C > 1 ? 1 : 0][ly + HALO][lx + HALO] - rec[MAT_NWIN + wi];
                const double d2 = (double)sg[C > 2 ? 2 : 0][ly + HALO][lx + HALO] - rec[2 * MAT_NWIN + wi];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const double* q = rec + (3 + 4 * c) * MAT_NWIN + wi;
                    const double v = (double)sy[c][ly + HALO][lx + HALO] * inv255 - q[0];
                    r[c] += v - (q[MAT_NWIN] * d0 + q[2 * MAT_NWIN] * d1 + q[3 * MAT_NWIN] * d2);
                }
            } else {
                const double d = (double)sg[0][ly + HALO][lx + HALO] - rec[wi];
                const double v = (double)sy[0][ly + HALO][lx + HALO] * inv255 - rec[MAT_NWIN + wi];
                r[0] += v - rec[2 * MAT_NWIN + wi] * d;
            }
        }
    }
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float* g = grad + ((size_t)c * h + py) * w + px;
            const float term = coef * (float)r[c];      // product and sum each rounded (contraction is off in this block)
            g[0] = accumulate ? g[0] + term : term;
        }
    }
}

int mat_tiles(int h, int w) {
    if (h < 3 || w < 3) return 0;
    return ((w - 2 + MAT_TW - 1) / MAT_TW) * ((h - 2 + MAT_TH - 1) / MAT_TH);
}

hipError_t launch_mat_forward(const float* y, const float* guide, int C, int h, int w, double gscale, double eps, double* partial,
                              hipStream_t stream) {
    if ((C != 1 && C != 3) || h < 3 || w < 3 || !(eps > 0.0) || !y || !guide || !partial) return hipErrorInvalidValue;
    const dim3 grid((w - 2 + MAT_TW - 1) / MAT_TW, (h - 2 + MAT_TH - 1) / MAT_TH);
    if (C == 3)
        hipLaunchKernelGGL((mat_window_kernel<3, false>), grid, dim3(256), 0, stream, y, guide, h, w, gscale, eps, partial, 0.f, nullptr, 0);
    else
        hipLaunchKernelGGL((mat_window_kernel<1, false>), grid, dim3(256), 0, stream, y, guide, h, w, gscale, eps, partial, 0.f, nullptr, 0);
    return hipGetLastError();
}

hipError_t launch_mat_backward(const float* y, const float* guide, int C, int h, int w, double gscale, double eps, float coef,
                               float* grad, int accumulate, hipStream_t stream) {
    if ((C != 1 && C != 3) || h < 3 || w < 3 || !(eps > 0.0) || !y || !guide || !grad) return hipErrorInvalidValue;
    const dim3 grid((w + MAT_TW - 1) / MAT_TW, (h + MAT_TH - 1) / MAT_TH);
    if (C == 3)
        hipLaunchKernelGGL((mat_window_kernel<3, true>), grid, dim3(256), 0, stream, y, guide, h, w, gscale, eps, nullptr, coef, grad, accumulate);
    else
        hipLaunchKernelGGL((mat_window_kernel<1, true>), grid, dim3(256), 0, stream, y, guide, h, w, gscale, eps, nullptr, coef, grad, accumulate);
    return hipGetLastError();
}

// ------------------------------------------------------------------ mat = (float)(sum of the tile partials / n)
// thread t adds the partials t, t + 256, ... in index order, then the fixed tree: the order of loss_rows_kernel
__global__ __launch_bounds__(256) void mat_value_kernel(const double* __restrict__ partial, int tiles, double n, float* __restrict__ out) {
    __shared__ double sh[4];
    double v = 0.0;
    for (int b = threadIdx.x; b < tiles; b += 256) v += partial[b];
    const double r = mat_block_sum(v, sh);
    if (threadIdx.x == 0) out[0] = (float)(r / n);
}
hipError_t launch_mat_value(const double* partial, int tiles, double n, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(mat_value_kernel, dim3(1), dim3(256), 0, stream, partial, tiles, n, out);
    return hipGetLastError();
}

}  // namespace nst
