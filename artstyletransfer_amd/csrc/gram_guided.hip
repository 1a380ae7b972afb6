// gram_guided.hip - spatial control (Gatys et al. 2017, guided Gram matrices; include/nst_hip.h has the definitions): the
// kernels around the guided Gram partials of gram.hip.
//   guide_pool_kernel          the guidance pyramid: one 2x2/2 mean-pool step of the (R,h,w) planes, the order of every
//                              pooling kernel here
//   guide_mass_*               n_r = sum_p t_r(p)^2 in double, two ordered stages, and the count of values outside [0,1]
//   guided_fold_kernel         the loss partials of a map: sum_r lambda_r * partial_r, in double
//   guided_bwd_kernel          dF = addend + sum_r t_r^2 . F . S_r on the exact fp32 matrix cores
#include <hip/hip_runtime.h>

#include "nst_kernels.h"

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- guidance pyramid ------------------------------------------------------------------------------------------------
// out (R, H/2, W/2) = mean of the 2x2 windows of in (R, H, W): ((e00 + e01) + e10) + e11, times 1/4 (floor sizes)
__global__ __launch_bounds__(256) void guide_pool_kernel(const float* __restrict__ in, int R, int H, int W, float* __restrict__ out) {
    const int oh = H / 2, ow = W / 2;
    const size_t n = (size_t)R * oh * ow;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % ow);
        const size_t ry = i / ow;
        const int y = (int)(ry % oh), r = (int)(ry / oh);
        const float* src = in + ((size_t)r * H + 2 * y) * W + 2 * x;
        const float s = __fadd_rn(__fadd_rn(__fadd_rn(src[0], src[1]), src[W]), src[W + 1]);
        out[i] = __fmul_rn(s, 0.25f);
    }
}

// ---- masses ----------------------------------------------------------------------------------------------------------
// stage 1: block b of region r sums t^2 (double) over its strided share of the plane's n values and counts the values that
// are not in [0,1] (a NaN fails both comparisons' complement); partial[(r * GUIDE_MASS_BLOCKS + b) * 2 + {0, 1}]
__global__ __launch_bounds__(256) void guide_mass_partial_kernel(const float* __restrict__ t, size_t n, double* __restrict__ partial) {
    __shared__ double sh[256], shb[256];
    const int r = blockIdx.y;
    const float* p = t + (size_t)r * n;
    double s = 0.0, bad = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)GUIDE_MASS_BLOCKS * 256) {
        const float v = p[i];
        s += (double)v * (double)v;
        if (!(v >= 0.f && v <= 1.f)) bad += 1.0;
    }
    sh[threadIdx.x] = s; shb[threadIdx.x] = bad;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) { sh[threadIdx.x] += sh[threadIdx.x + off]; shb[threadIdx.x] += shb[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[((size_t)r * GUIDE_MASS_BLOCKS + blockIdx.x) * 2] = sh[0];
        partial[((size_t)r * GUIDE_MASS_BLOCKS + blockIdx.x) * 2 + 1] = shb[0];
    }
}
// stage 2: the block partials in block order; out[r * 2 + {0, 1}] = mass, count of bad values
__global__ void guide_mass_finish_kernel(const double* __restrict__ partial, int R, double* __restrict__ out) {
    const int r = threadIdx.x;
    if (r >= R) return;
    double s = 0.0, bad = 0.0;
    for (int b = 0; b < GUIDE_MASS_BLOCKS; ++b) {
        s += partial[((size_t)r * GUIDE_MASS_BLOCKS + b) * 2];
        bad += partial[((size_t)r * GUIDE_MASS_BLOCKS + b) * 2 + 1];
    }
    out[r * 2] = s; out[r * 2 + 1] = bad;
}

// ---- loss partials of a guided map -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void guided_fold_kernel(const double* __restrict__ part, int R, int blocks, float l0, float l1, float l2,
                                                          float l3, double* __restrict__ out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= blocks) return;
    const float lam[4] = {l0, l1, l2, l3};
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += (double)lam[r] * part[(size_t)r * blocks + b];
    out[b] = s;
}

// ---- guided Gram backward --------------------------------------------------------------------------------------------
// out[p][c] = addend[p][c] + sum_r t_r(p)^2 sum_k F[p][k] S_r[k][c]: one GEMM with M = pixels, N = C, K = R C, whose A rows
// are scaled per K block.  v_mfma_f32_32x32x2_f32: exact fp32 products, an ordered fmaf chain over k.  A workgroup owns 128
// pixels x 64 output channels, a wave 32 pixels x 64 channels (two accumulators); K is staged 32 deep: A rows (scaled by
// t_r^2 on the way) at a 33-float pitch, S_r rows as they are.  The next chunk's global loads are issued before the MFMAs
// of the current one.  Pixels beyond N are staged as zeros and never stored.
constexpr int GB_M = 128, GB_N = 64, GB_K = 32, GB_APITCH = GB_K + 1;

__global__ __launch_bounds__(256) void guided_bwd_kernel(GuidedBwd g) {
    __shared__ float As[GB_M * GB_APITCH];
    __shared__ __attribute__((aligned(16))) float Bs[GB_K * GB_N];
    __shared__ float T2[4][GB_M];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const size_t p0 = (size_t)blockIdx.x * GB_M;
    const int c0 = blockIdx.y * GB_N;
    const int C = g.C;

    for (int i = tid; i < g.R * GB_M; i += 256) {
        const int r = i / GB_M, m = i - r * GB_M;
        const size_t p = p0 + m;
        const float t = p < g.N ? g.t[r][p] : 0.f;
        T2[r][m] = t * t;
    }

    f32x4 ra[4], rb[2];
    const int chunks_per_r = C / GB_K;
    const int nchunks = g.R * chunks_per_r;
    auto load = [&](int chunk) {
        const int r = chunk / chunks_per_r, k0 = (chunk - r * chunks_per_r) * GB_K;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + i * 256;
            const int m = u >> 3, kq = u & 7;
            const size_t p = p0 + m;
            ra[i] = p < g.N ? *reinterpret_cast<const f32x4*>(g.F + p * C + k0 + kq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* S = g.S[r];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + i * 256;
            const int k = u >> 4, cq = u & 15;
            rb[i] = *reinterpret_cast<const f32x4*>(S + (size_t)(k0 + k) * C + c0 + cq * 4);
        }
    };
    auto store = [&](int chunk) {
        const int r = chunk / chunks_per_r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + i * 256;
            const int m = u >> 3, kq = u & 7;
            const float t2 = T2[r][m];
            float* dst = As + m * GB_APITCH + kq * 4;
            dst[0] = ra[i][0] * t2; dst[1] = ra[i][1] * t2; dst[2] = ra[i][2] * t2; dst[3] = ra[i][3] * t2;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + i * 256;
            *reinterpret_cast<f32x4*>(Bs + u * 4) = rb[i];
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;

    load(0);
    __syncthreads();                 // T2 is complete
    for (int c = 0; c < nchunks; ++c) {
        store(c);
        __syncthreads();
        if (c + 1 < nchunks) load(c + 1);
        const float* arow = As + (wave * 32 + l31) * GB_APITCH + half;
        const float* brow = Bs + half * GB_N + l31;
#pragma unroll
        for (int k2 = 0; k2 < GB_K / 2; ++k2) {
            const float a = arow[2 * k2];
            const float b0 = brow[2 * k2 * GB_N];
            const float b1 = brow[2 * k2 * GB_N + 32];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
        }
        __syncthreads();
    }

    float vmax = 0.f;
    const int words = C / 32;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
            const size_t p = p0 + wave * 32 + m;
            if (p >= g.N) continue;
            const int c = c0 + nt * 32 + l31;
            const size_t e = p * C + c;
            float v = acc[nt][r];
            if (g.addend) v = g.addend[e] + v;
            if (g.bits) { if (!((g.bits[p * words + (c >> 5)] >> (c & 31)) & 1u)) v = 0.f; }
            else if (g.mask) { if (!(g.mask[e] > 0.f)) v = 0.f; }
            g.out[e] = v;
            vmax = fmaxf(vmax, fabsf(v));
        }
    if (g.amax_out) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off));
        if (lane == 0) atomicMax(g.amax_out + ((blockIdx.x * 4 + wave) & (NST_AMAX_SLOTS - 1)), __float_as_uint(vmax));
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------
hipError_t launch_guide_pool(const float* in, int R, int H, int W, float* out, hipStream_t stream) {
    const size_t n = (size_t)R * (H / 2) * (W / 2);
    if (n == 0) return hipErrorInvalidValue;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(guide_pool_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, in, R, H, W, out);
    return hipGetLastError();
}

hipError_t launch_guide_mass(const float* t, int R, size_t n, double* scratch, double* out, hipStream_t stream) {
    if (R < 1 || R > NST_MAX_REGIONS_K) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guide_mass_partial_kernel, dim3(GUIDE_MASS_BLOCKS, R), dim3(256), 0, stream, t, n, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(guide_mass_finish_kernel, dim3(1), dim3(64), 0, stream, scratch, R, out);
    return hipGetLastError();
}

hipError_t launch_guided_fold(const double* part, int R, int blocks, const float* lambda, double* out, hipStream_t stream) {
    float l[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < R && r < 4; ++r) l[r] = lambda[r];
    hipLaunchKernelGGL(guided_fold_kernel, dim3((blocks + 255) / 256), dim3(256), 0, stream, part, R, blocks, l[0], l[1], l[2], l[3], out);
    return hipGetLastError();
}

hipError_t launch_guided_bwd(const GuidedBwd& g, hipStream_t stream) {
    if (g.R < 1 || g.R > NST_MAX_REGIONS_K || g.C % GB_N != 0 || g.N == 0 || !g.F || !g.out) return hipErrorInvalidValue;
    const size_t mb = (g.N + GB_M - 1) / GB_M;
    if (mb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(guided_bwd_kernel, dim3((unsigned)mb, g.C / GB_N), dim3(256), 0, stream, g);
    return hipGetLastError();
}

}  // namespace nst
