// selfsim.hip - the self-similarity content term (Kolkin, Salavon & Shakhnarovich 2019; include/nst_hip.h has the definition):
// the pattern of pairwise cosine distances between the sampled feature vectors of a map must be that of the same map of the
// content image.  The sample grid, the norms (launch_remd_norms) and the packed f16x2 operand (launch_remd_pack) are the
// relaxed EMD term's; nst_pieces.h has the operand pieces.
//
//   selfsim_matrix_kernel        D = the n x n cosine distances: remd_search_kernel's tile with both operands the same sample
//                                set, K = C, on v_mfma_f32_32x32x16_f16 with three MFMAs per product block; the epilogue
//                                stores the tile where the search's took an arg-max
//   selfsim_colsum_kernel        s_j = sum_i D_ij in double, per row block; selfsim_colsum_finish_kernel: the row blocks in
//                                ascending order, and q_j = 1 / (s_j + epsilon)
//   selfsim_value_kernel         streams D and the content's D: the signs sg, and per row block the partials of |N - M| and of
//                                t_j = sum_i sg_ij N_ij; selfsim_value_finish_kernel: t_j and the value
//   selfsim_w_kernel             W = E + E^T, E_ij = (sg_ij - t_j) q_j off the diagonal and the clamp
//   selfsim_u_kernel             U = the normalised samples rp_j X_j, n x C
//   selfsim_grad_kernel          g = -W U on v_mfma_f32_32x32x2_f32, k ascending, then the norm's Jacobian, the coefficient and
//                                the scatter to the sampled pixels
//
// Reproducibility: no atomic at all.  Every sum has one owner and a fixed order.
#include <hip/hip_runtime.h>

#include "nst_kernels.h"
#include "nst_pieces.h"

namespace nst {

namespace {

__device__ __forceinline__ size_t sample_off(const RemdSide& s, int k) {
    const int a = k / s.nb, b = k - a * s.nb;
    return ((size_t)(a * s.stride) * s.w + (size_t)(b * s.stride)) * s.C;
}

// ---- the distance matrix --------------------------------------------------------------------------------------------------
// remd_search_kernel's staging and walk (remd.hip has the description): a workgroup (8 waves) owns 32 NCT consecutive column
// samples j, cut into the two pieces once in LDS; wave g of the grid's 8 nsplit takes the row tiles g, g + 8 nsplit, ... of the
// packed operand from global memory.  A 32x32 accumulator has its column on the lane, so register e of a lane half is one row
// of 32 consecutive columns: a 128-byte store into row-major D.
template <int NCT>
struct SelfSimCfg {
    static constexpr int COLS = 32 * NCT;
    static constexpr int PF = NCT == 1 ? 4 : 2;      // k-steps per prefetch group (C / 16 is a multiple of 4)
    static __host__ __device__ constexpr int rowb(int C) { return 4 * C + 16; }
    static __host__ __device__ constexpr int lds_bytes(int C) { return COLS * rowb(C); }
};

template <int NCT>
__global__ __launch_bounds__(512) void selfsim_matrix_kernel(RemdSide p, float* __restrict__ D) {
    using Cf = SelfSimCfg<NCT>;
    constexpr int PF = Cf::PF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, ROWB = Cf::rowb(C), n = p.count;
    const int j0 = (int)blockIdx.x * Cf::COLS;       // the tile's first column sample
    float sc, invs;
    tensor_scale(p.amax, lane, sc, invs);
    const float inv = invs * invs;
    {
        const int c4n = C >> 2;
        const int units = Cf::COLS * c4n;
        for (int u = tid; u < units; u += 512) {
            const int col = u / c4n, c4 = u - col * c4n;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j0 + col < n) v = *reinterpret_cast<const f32x4*>(p.f + sample_off(p, j0 + col) + c4 * 4);
            u32x2 hi, lo;
            cut2x4(v, sc, hi, lo);
            unsigned char* dst = smem + col * ROWB + (c4 >> 1) * 32 + (c4 & 1) * 8;
            *reinterpret_cast<u32x2*>(dst) = hi;
            *reinterpret_cast<u32x2*>(dst + 16) = lo;
        }
    }
    __syncthreads();

    const int r = lane & 31, hh = lane >> 5;
    const int KS = C / 16, G = KS / PF;
    const int lane_off = r * ROWB + hh * 32;
    const int ntiles = remd_tiles(n);
    const int g0 = (int)blockIdx.y * 8 + wave, gstride = (int)gridDim.y * 8;
    const int mine = g0 < ntiles ? (ntiles - g0 + gstride - 1) / gstride : 0;
    float rcol[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int j = j0 + 32 * ct + r;
        rcol[ct] = p.r[j < n ? j : n - 1];      // (a column behind the last sample is never stored)
    }

    const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.packed) + (size_t)lane * 16;
    auto group_ptr = [&](int it) -> const unsigned char* {      // prefetch group `it` of this wave's walk
        const int tl = it / G, g = it - tl * G;
        return abase + (((size_t)(g0 + tl * gstride) * KS + (size_t)g * PF) * 2) * 1024;
    };
    const int total = mine * G;
    u32x4 ah[PF], al[PF];
    if (total > 0) {
        const unsigned char* a = group_ptr(0);
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            ah[u] = *reinterpret_cast<const u32x4*>(a + u * 2048);
            al[u] = *reinterpret_cast<const u32x4*>(a + u * 2048 + 1024);
        }
    }
    f32x16 accm[NCT], accx[NCT];
    int g = 0, tl = 0;
    for (int it = 0; it < total; ++it) {
        if (g == 0) {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int e = 0; e < 16; ++e) { accm[ct][e] = 0.f; accx[ct][e] = 0.f; }
        }
        // the next group's row fragments (the last iteration loads its own again: no branch around the loads)
        u32x4 nh[PF], nl[PF];
        {
            const unsigned char* a = group_ptr(it + 1 < total ? it + 1 : it);
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                nh[u] = *reinterpret_cast<const u32x4*>(a + u * 2048);
                nl[u] = *reinterpret_cast<const u32x4*>(a + u * 2048 + 1024);
            }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const unsigned char* b = smem + lane_off + (g * PF + u) * 64;
            const f16x8 a_hi = __builtin_bit_cast(f16x8, ah[u]), a_lo = __builtin_bit_cast(f16x8, al[u]);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const f16x8 b_hi = *reinterpret_cast<const f16x8*>(b + ct * 32 * ROWB);
                const f16x8 b_lo = *reinterpret_cast<const f16x8*>(b + ct * 32 * ROWB + 16);
                accx[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, accx[ct], 0, 0, 0);
                accm[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, accm[ct], 0, 0, 0);
                accx[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, accx[ct], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) { ah[u] = nh[u]; al[u] = nl[u]; }
        if (++g == G) {
            // the tile is complete: register e of a lane is row (e & 3) + 8 (e >> 2) + 4 hh, row sample i = 32 tile + row.
            // c = (((hi + lo 2^-11) inv) r_row) r_col + 0, every operation rounded; D = 0 on the diagonal, else max(0, 1 - c)
#pragma clang fp contract(off)
            const int i0 = (g0 + tl * gstride) * 32;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 rrow = *reinterpret_cast<const f32x4*>(p.r + i0 + 8 * q + 4 * hh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = i0 + 8 * q + 4 * hh + e;
                    if (i >= n) continue;
                    float* drow = D + (size_t)i * n;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const int j = j0 + 32 * ct + r;
                        const float c = (((accm[ct][4 * q + e] + accx[ct][4 * q + e] * LO_DOWN) * inv) * rrow[e]) * rcol[ct] + 0.f;
                        const float d = i == j ? 0.f : fmaxf(0.f, 1.f - c);
                        if (j < n) drow[j] = d;
                    }
                }
            }
            g = 0;
            ++tl;
        }
    }
}

// ---- the passes over the n x n arrays ---------------------------------------------------------------------------------------
// One shape for the column sums and the value: grid (ceil(n / 64), SELFSIM_ROW_BLOCKS), the lane is the column, row block b owns
// the rows [b per, (b + 1) per), per = ceil(n / SELFSIM_ROW_BLOCKS); wave v of the four adds the rows b per + v, + 4, ... in
// ascending order, then the four waves in wave order.
__global__ __launch_bounds__(256) void selfsim_colsum_kernel(const float* __restrict__ D, int n, double* __restrict__ part) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = (int)blockIdx.x * 64 + lane;
    const int per = (n + SELFSIM_ROW_BLOCKS - 1) / SELFSIM_ROW_BLOCKS;
    const int i0 = (int)blockIdx.y * per;
    const int i1 = i0 + per < n ? i0 + per : n;
    double acc = 0.0;
    if (j < n) {
#pragma unroll 4
        for (int i = i0 + wave; i < i1; i += 4) acc += (double)D[(size_t)i * n + j];
    }
    sh[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && j < n) part[(size_t)blockIdx.y * n + j] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

__global__ __launch_bounds__(256) void selfsim_colsum_finish_kernel(const double* __restrict__ part, int n, double epsilon, double* __restrict__ s,
                                                                    double* __restrict__ q) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= n) return;
    double acc = 0.0;
    for (int b = 0; b < SELFSIM_ROW_BLOCKS; ++b) acc += part[(size_t)b * n + j];
    s[j] = acc;
    q[j] = 1.0 / (acc + epsilon);
}

// N_ij = D_ij q_j and M_ij = Dc_ij qc_j in double, each product rounded (contraction off: a fused N - M would not be 0 for
// equal operands); sg = sign(N - M); partials of |N - M| and of sg N
__global__ __launch_bounds__(256) void selfsim_value_kernel(SelfSimTerm t) {
#pragma clang fp contract(off)
    __shared__ double sa[4][64], st[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = t.n;
    const int j = (int)blockIdx.x * 64 + lane;
    const int per = (n + SELFSIM_ROW_BLOCKS - 1) / SELFSIM_ROW_BLOCKS;
    const int i0 = (int)blockIdx.y * per;
    const int i1 = i0 + per < n ? i0 + per : n;
    double aa = 0.0, at = 0.0;
    if (j < n) {
        const double qj = t.q[j], qcj = t.qc[j];
#pragma unroll 4
        for (int i = i0 + wave; i < i1; i += 4) {
            const size_t o = (size_t)i * n + j;
            const double a = (double)t.D[o] * qj, b = (double)t.Dc[o] * qcj;
            const double d = a - b;
            const int g = (d > 0.0) - (d < 0.0);
            t.sg[o] = (signed char)g;
            aa += fabs(d);
            at += g > 0 ? a : (g < 0 ? -a : 0.0);
        }
    }
    sa[wave][lane] = aa;
    st[wave][lane] = at;
    __syncthreads();
    if (wave == 0 && j < n) {
        t.part[(size_t)blockIdx.y * n + j] = ((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane];
        t.part[(size_t)(SELFSIM_ROW_BLOCKS + blockIdx.y) * n + j] = ((st[0][lane] + st[1][lane]) + st[2][lane]) + st[3][lane];
    }
}

// one workgroup: per column the row blocks in ascending order (t_j, and the column's |N - M|); thread u adds the columns u,
// u + 256, ... in ascending order, the 256 threads by a tree; value = (float)(sum / n)
__global__ __launch_bounds__(256) void selfsim_value_finish_kernel(SelfSimTerm t) {
    __shared__ double sh[256];
    const int tid = threadIdx.x, n = t.n;
    double acc = 0.0;
    for (int j = tid; j < n; j += 256) {
        double a = 0.0, tt = 0.0;
        for (int b = 0; b < SELFSIM_ROW_BLOCKS; ++b) {
            a += t.part[(size_t)b * n + j];
            tt += t.part[(size_t)(SELFSIM_ROW_BLOCKS + b) * n + j];
        }
        t.t[j] = tt;
        acc += a;
    }
    sh[tid] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    if (tid == 0) *t.val = (float)(sh[0] / (double)n);
}

// ---- the gradient -------------------------------------------------------------------------------------------------------------
// E_ij = (sg_ij - t_j) q_j in double, zero on the diagonal and where D_ij = 0 (the clamp); W_ij = (float)(E_ij + E_ji).  A
// workgroup owns one 32x32 tile and reads the mirrored tile through LDS.  The double sum commutes, so W_ij and W_ji share bits.
__device__ __forceinline__ double selfsim_e(const SelfSimTerm& t, int i, int j) {
#pragma clang fp contract(off)
    if (i >= t.n || j >= t.n || i == j) return 0.0;
    const size_t o = (size_t)i * t.n + j;
    if (t.D[o] == 0.f) return 0.0;
    return ((double)t.sg[o] - t.t[j]) * t.q[j];
}

__global__ __launch_bounds__(256) void selfsim_w_kernel(SelfSimTerm t, float* __restrict__ W) {
#pragma clang fp contract(off)
    __shared__ double sh[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = (int)blockIdx.y * 32, j0 = (int)blockIdx.x * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = ty + 8 * k;
        sh[a][tx] = selfsim_e(t, j0 + a, i0 + tx);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int a = ty + 8 * k;
        const int i = i0 + a, j = j0 + tx;
        if (i < t.n && j < t.n) W[(size_t)i * t.n + j] = (float)(selfsim_e(t, i, j) + sh[tx][a]);
    }
}

// U_j = rp_j X_j, fp32, one rounding: a thread per (sample, 4 channels)
__global__ __launch_bounds__(256) void selfsim_u_kernel(RemdSide x, float* __restrict__ U) {
    const int c4n = x.C >> 2;
    const size_t total = (size_t)x.count * c4n;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (size_t)gridDim.x * 256) {
        const int k = (int)(u / c4n), c4 = (int)(u - (size_t)k * c4n);
        const f32x4 v = *reinterpret_cast<const f32x4*>(x.f + sample_off(x, k) + c4 * 4);
        *reinterpret_cast<f32x4*>(U + (size_t)k * x.C + c4 * 4) = v * x.r[k];
    }
}

// A workgroup (8 waves) owns the 32 samples i0 .. i0 + 31 and all C channels; wave v the 32-channel blocks v and v + 8.  The row
// operand of v_mfma_f32_32x32x2_f32 is W[i][k]: a lane reads W[k][i], the same bits, so that 32 lanes read 128 consecutive
// bytes; the column operand is U[k][c].  k ascends, two a step.  Then per sample <g, u> in double - the 32 lanes of a channel
// block by the xor tree (offsets 16 .. 1), the blocks in ascending order through LDS - and
// dX = ((g - (float)<g, u> u) rp) coef, contraction off, written or added at the sample's pixel.
__global__ __launch_bounds__(512) void selfsim_grad_kernel(RemdSide x, const float* __restrict__ W, const float* __restrict__ U, float coef,
                                                           float* __restrict__ out, int accumulate) {
    __shared__ double dotp[16][32];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int n = x.count, C = x.C, nblk = C >> 5;
    const int i0 = (int)blockIdx.x * 32;
    const bool has0 = wave < nblk, has1 = wave + 8 < nblk;
    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
    if (has0) {
        const int ia = i0 + r;
        const bool aok = ia < n;
        const float* wp = W + (aok ? ia : n - 1);
        const float* up = U + wave * 32 + r;
        // eight k-steps a round: their loads first, then the MFMAs (operands behind row n - 1 are zeros and add nothing)
        for (int k = 0; k < n; k += 16) {
            float a[8], b0[8], b1[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int kk = k + 2 * u + hh;
                const bool ok = kk < n;
                const size_t kc = (size_t)(ok ? kk : n - 1);
                const float av = wp[kc * n], bv0 = up[kc * C], bv1 = has1 ? up[kc * C + 256] : 0.f;
                a[u] = ok && aok ? av : 0.f;
                b0[u] = ok ? bv0 : 0.f;
                b1[u] = ok ? bv1 : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b0[u], acc[0], 0, 0, 0);
                if (has1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b1[u], acc[1], 0, 0, 0);
            }
        }
    }
    // g = -acc; the partial <g, u> of every channel block
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        if (!(b ? has1 : has0)) continue;
        const int cb = wave + 8 * b;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * hh;
            const int i = i0 + row;
            const float u = i < n ? U[(size_t)i * C + cb * 32 + r] : 0.f;
            double pr = (double)(-acc[b][e]) * (double)u;
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) pr += __shfl_xor(pr, off);
            if (r == 0) dotp[cb][row] = pr;
        }
    }
    __syncthreads();
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            if (!(b ? has1 : has0)) continue;
            const int cb = wave + 8 * b;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * hh;
                const int i = i0 + row;
                if (i >= n) continue;
                double d = 0.0;
                for (int c2 = 0; c2 < nblk; ++c2) d += dotp[c2][row];
                const float df = (float)d;
                const float u = U[(size_t)i * C + cb * 32 + r];
                float v = (((-acc[b][e]) - df * u) * x.r[i]) * coef;
                float* dst = out + sample_off(x, i) + cb * 32 + r;
                if (accumulate) v = *dst + v;
                *dst = v;
            }
        }
    }
}

bool selfsim_side_ok(const RemdSide& s) {
    return s.f && s.count >= 1 && s.count <= SELFSIM_MAX_SAMPLES && (s.C == 64 || s.C == 128 || s.C == 256 || s.C == 512) && s.stride >= 1 &&
           s.nb >= 1 && s.na >= 1 && (long long)s.na * s.nb == s.count && (long long)(s.na - 1) * s.stride < s.h &&
           (long long)(s.nb - 1) * s.stride < s.w && s.r;
}

bool selfsim_term_ok(const SelfSimTerm& t) {
    return t.D && t.q && t.Dc && t.qc && t.n >= 1 && t.n <= SELFSIM_MAX_SAMPLES && t.sg && t.part && t.t && t.val;
}

template <int NCT>
hipError_t selfsim_matrix_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&selfsim_matrix_kernel<NCT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               SelfSimCfg<NCT>::lds_bytes(512 / NCT));
}

template <int NCT>
hipError_t selfsim_matrix_launch(const RemdSide& x, float* D, hipStream_t stream) {
    using Cf = SelfSimCfg<NCT>;
    const int tiles = (x.count + Cf::COLS - 1) / Cf::COLS, dt = remd_tiles(x.count);
    // remd_search_launch's split of the row walk: about two workgroups per CU's worth of waves, every wave at least one tile
    int nsplit = (512 + tiles - 1) / tiles;
    const int cap = (dt + 7) / 8;
    if (nsplit > cap) nsplit = cap;
    if (nsplit < 1) nsplit = 1;
    hipLaunchKernelGGL((selfsim_matrix_kernel<NCT>), dim3((unsigned)tiles, (unsigned)nsplit), dim3(512), (size_t)Cf::lds_bytes(x.C), stream, x, D);
    return hipGetLastError();
}

}  // namespace

// once per device, before the first launch there (the matrix kernels take more than 64 KB of dynamic LDS)
hipError_t selfsim_init_device() {
    hipError_t e = selfsim_matrix_attr<1>();
    if (e == hipSuccess) e = selfsim_matrix_attr<2>();
    if (e == hipSuccess) e = selfsim_matrix_attr<4>();
    return e;
}

hipError_t launch_selfsim_matrix(const RemdSide& x, float* D, hipStream_t stream) {
    if (!selfsim_side_ok(x) || !x.amax || !x.packed || !D) return hipErrorInvalidValue;
    return x.C == 512 ? selfsim_matrix_launch<1>(x, D, stream) : (x.C == 256 ? selfsim_matrix_launch<2>(x, D, stream) : selfsim_matrix_launch<4>(x, D, stream));
}

hipError_t launch_selfsim_colsums(const float* D, int n, double epsilon, double* part, double* s, double* q, hipStream_t stream) {
    if (!D || n < 1 || n > SELFSIM_MAX_SAMPLES || !(epsilon > 0.0) || !part || !s || !q) return hipErrorInvalidValue;
    hipLaunchKernelGGL(selfsim_colsum_kernel, dim3((unsigned)((n + 63) / 64), SELFSIM_ROW_BLOCKS), dim3(256), 0, stream, D, n, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(selfsim_colsum_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, part, n, epsilon, s, q);
    return hipGetLastError();
}

hipError_t launch_selfsim_value(const SelfSimTerm& t, hipStream_t stream) {
    if (!selfsim_term_ok(t)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(selfsim_value_kernel, dim3((unsigned)((t.n + 63) / 64), SELFSIM_ROW_BLOCKS), dim3(256), 0, stream, t);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(selfsim_value_finish_kernel, dim3(1), dim3(256), 0, stream, t);
    return hipGetLastError();
}

hipError_t launch_selfsim_grad(const RemdSide& x, const SelfSimTerm& t, float coef, float* W, float* U, float* out, int accumulate,
                               hipStream_t stream) {
    if (!selfsim_side_ok(x) || !selfsim_term_ok(t) || t.n != x.count || !W || !U || !out) return hipErrorInvalidValue;
    if (!accumulate) {
        const hipError_t e = launch_zero(out, (size_t)x.h * x.w * x.C, stream);
        if (e != hipSuccess) return e;
    }
    const unsigned nt = (unsigned)remd_tiles(t.n);
    hipLaunchKernelGGL(selfsim_w_kernel, dim3(nt, nt), dim3(256), 0, stream, t, W);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t units = (size_t)x.count * (x.C / 4), want = (units + 255) / 256;
    hipLaunchKernelGGL(selfsim_u_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(256), 0, stream, x, U);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(selfsim_grad_kernel, dim3(nt), dim3(512), 0, stream, x, W, U, coef, out, accumulate);
    return hipGetLastError();
}

}  // namespace nst
