// remd.hip - the relaxed EMD style term (Kolkin, Salavon & Shakhnarovich 2019; include/nst_hip.h has the definition): the
// feature vectors of a map, sampled on a stride grid, are matched by cosine to the sampled vectors of the style's map, and the
// style's vectors back to the map's; the term is the larger of the two mean cosine distances.
//
//   remd_norm_kernel     r_k = 1 / sqrt(|V_k|^2 + epsilon) of one side's samples, the norm summed in double
//   remd_pack_kernel     one side's samples cut into two scaled fp16 pieces and laid out in the lane order of the MFMA's row
//                        operand (patch_match.hip's layout with K = C)
//   remd_search_kernel   one direction of the search: an implicit GEMM, rows = the dictionary side's samples, columns = the
//                        other side's, K = C, on v_mfma_f32_32x32x16_f16 with three MFMAs per product block and the arg-max
//                        epilogue of pm_search_kernel.  Direction A has the style as the dictionary, direction B the image:
//                        the same kernel with the roles swapped, so both arg-maxes share one epilogue and one tie rule
//   remd_decode_kernel   keys -> nn (int32)
//   remd_value_kernel    the cosines at the matches in double, both sides, and their sums in two ordered stages
//                        (remd_value_finish_kernel: the second, which also decides the side)
//   remd_grad_kernel     the gradient of the active side at fixed matches, gather form: a wave per image sample
//
// Reproducibility: the only combine across waves and workgroups is the integer atomicMax on the 64-bit key, as in
// patch_match.hip; side B's sum over the style samples that chose one image sample runs in ascending j.  No float atomic.
#include <hip/hip_runtime.h>

#include "nst_kernels.h"
#include "nst_pieces.h"

namespace nst {

namespace {

__device__ __forceinline__ const float* sample_ptr(const RemdSide& s, int k) {
    const int a = k / s.nb, b = k - a * s.nb;
    return s.f + ((size_t)(a * s.stride) * s.w + (size_t)(b * s.stride)) * s.C;
}

// ---- norms and the packed operand -----------------------------------------------------------------------------------------
// one wave per sample: lane l adds the squares of its 16-byte runs l, l + 64, ... in ascending order, the lanes by a fixed tree;
// the padding entries of the last tile get 0
__global__ __launch_bounds__(256) void remd_norm_kernel(RemdSide s, double epsilon, float* __restrict__ r) {
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (k >= remd_tiles(s.count) * 32) return;
    if (k >= s.count) {
        if (lane == 0) r[k] = 0.f;
        return;
    }
    const float* src = sample_ptr(s, k);
    double acc = 0.0;
    for (int u = lane; u < (s.C >> 2); u += 64) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + u * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) r[k] = (float)(1.0 / sqrt(acc + epsilon));
}

// one thread per (sample, 8 consecutive channels).  packed: [tile of 32 samples][k-step of 16][piece][lane][8 fp16],
// lane = 32 (c % 16 / 8) + sample % 32; zeros behind the last sample
__global__ __launch_bounds__(256) void remd_pack_kernel(RemdSide s, unsigned char* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    float sc, inv;
    tensor_scale(s.amax, lane, sc, inv);
    const int k8n = s.C / 8, KS = s.C / 16;
    const size_t total = (size_t)remd_tiles(s.count) * 32 * k8n;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (size_t)gridDim.x * 256) {
        const int j = (int)(u / k8n), c = (int)(u - (size_t)j * k8n) * 8;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (j < s.count) {
            const float* src = sample_ptr(s, j) + c;
            v0 = *reinterpret_cast<const f32x4*>(src);
            v1 = *reinterpret_cast<const f32x4*>(src + 4);
        }
        u32x2 h0, l0, h1, l1;
        cut2x4(v0, sc, h0, l0);
        cut2x4(v1, sc, h1, l1);
        const int t = j >> 5, ks = c >> 4, ln = ((c >> 3) & 1) * 32 + (j & 31);
        unsigned char* dst = packed + (((size_t)t * KS + ks) * 2) * 1024 + (size_t)ln * 16;
        *reinterpret_cast<u32x4*>(dst) = u32x4{h0[0], h0[1], h1[0], h1[1]};
        *reinterpret_cast<u32x4*>(dst + 1024) = u32x4{l0[0], l0[1], l1[0], l1[1]};
    }
}

// ---- the search -----------------------------------------------------------------------------------------------------------
// A workgroup (8 waves) owns 32 NCT consecutive column samples.  It gathers them from the stride grid, all C channels, cut into
// the two pieces, once in LDS: a sample's row holds per 8 channels 16 B of hi and 16 B of lo, C / 8 such groups, + 16 B pad (an
// odd multiple of 16 B, so consecutive samples start on distinct 16-byte slots).  NCT = 512 / C capped at 4 keeps the tile at
// 66 KB for every C.  The waves then share the dictionary walk as in pm_search_kernel: wave g of the grid's 8 nsplit takes the
// tiles g, g + 8 nsplit, ...; a tile's row fragments come straight from global memory (two 1-KiB loads per k-step, prefetched PF
// k-steps ahead), the column fragments from LDS.  K = C is 4 to 32 k-steps, so a tile's epilogue (16 NCT scores per lane) is
// paid every 4 to 32 product blocks.
template <int NCT>
struct RemdCfg {
    static constexpr int COLS = 32 * NCT;
    static constexpr int PF = NCT == 1 ? 4 : 2;      // k-steps per prefetch group (C / 16 is a multiple of 4)
    static __host__ __device__ constexpr int rowb(int C) { return 4 * C + 16; }
    static __host__ __device__ constexpr int lds_bytes(int C) { return COLS * rowb(C); }
};

struct RemdSearch {
    RemdSide d, c;
    unsigned long long* keys;
};

template <int NCT>
__global__ __launch_bounds__(512) void remd_search_kernel(RemdSearch p) {
    using Cf = RemdCfg<NCT>;
    constexpr int PF = Cf::PF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.d.C, ROWB = Cf::rowb(C);
    const int i0 = (int)blockIdx.x * Cf::COLS;       // the tile's first column sample
    float sC, invC, sD, invD;
    tensor_scale(p.c.amax, lane, sC, invC);
    tensor_scale(p.d.amax, lane, sD, invD);
    const float inv = invC * invD;
    {
        const int c4n = C >> 2;
        const int units = Cf::COLS * c4n;
        for (int u = tid; u < units; u += 512) {
            const int col = u / c4n, c4 = u - col * c4n;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (i0 + col < p.c.count) v = *reinterpret_cast<const f32x4*>(sample_ptr(p.c, i0 + col) + c4 * 4);
            u32x2 hi, lo;
            cut2x4(v, sC, hi, lo);
            unsigned char* dst = smem + col * ROWB + (c4 >> 1) * 32 + (c4 & 1) * 8;
            *reinterpret_cast<u32x2*>(dst) = hi;
            *reinterpret_cast<u32x2*>(dst + 16) = lo;
        }
    }
    __syncthreads();

    const int r = lane & 31, hh = lane >> 5;
    const int KS = C / 16, G = KS / PF;
    // column r of column tile ct is sample i0 + 32 ct + r; its fragment of k-step ks: 8 channels from 16 ks + 8 hh
    const int lane_off = r * ROWB + hh * 32;
    const int ntiles = remd_tiles(p.d.count);
    const int g0 = (int)blockIdx.y * 8 + wave, gstride = (int)gridDim.y * 8;
    const int mine = g0 < ntiles ? (ntiles - g0 + gstride - 1) / gstride : 0;
    unsigned long long best[NCT];
    float rcol[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        best[ct] = 0ull;
        const int i = i0 + 32 * ct + r;
        rcol[ct] = p.c.r[i < p.c.count ? i : p.c.count - 1];      // (a column behind the last sample: its key is never written)
    }

    const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.d.packed) + (size_t)lane * 16;
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
            // the tile is complete: register e of a lane is row (e & 3) + 8 (e >> 2) + 4 hh, dictionary sample j = 32 tile + row.
            // c = (((hi + lo 2^-11) inv) r_row) r_col, every operation rounded, then + 0 (-0 -> +0)
#pragma clang fp contract(off)
            const int j0 = (g0 + tl * gstride) * 32;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 rrow = *reinterpret_cast<const f32x4*>(p.d.r + j0 + 8 * q + 4 * hh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = j0 + 8 * q + 4 * hh + e;
                    const unsigned low = ~(unsigned)j;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        const float sc = (((accm[ct][4 * q + e] + accx[ct][4 * q + e] * LO_DOWN) * inv) * rrow[e]) * rcol[ct] + 0.f;
                        const unsigned long long key = ((unsigned long long)score_order(sc) << 32) | low;
                        if (j < p.d.count && key > best[ct]) best[ct] = key;
                    }
                }
            }
            g = 0;
            ++tl;
        }
    }
    // the two lane halves hold different rows of the same columns; then one atomicMax per column and wave
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const unsigned long long o = __shfl_xor(best[ct], 32);
        const unsigned long long b = o > best[ct] ? o : best[ct];
        const int i = i0 + 32 * ct + r;
        if (hh == 0 && b != 0ull && i < p.c.count) atomicMax(p.keys + i, b);
    }
}

__global__ __launch_bounds__(256) void remd_decode_kernel(const unsigned long long* __restrict__ keys, int n, int m, int* __restrict__ nn) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    int j = (int)(~(unsigned)k);
    if (k == 0ull || j < 0 || j >= m) j = 0;
    nn[i] = j;
}

// ---- the value ------------------------------------------------------------------------------------------------------------
// stage one, blockIdx.y = the side (0: A, the image samples i with j = nnA(i); 1: B, the style samples j with i = nnB(j)): block b
// owns the samples [b per, (b + 1) per) of its side, wave v of it every fourth of them; per sample the wave forms <X, Y>, |X|^2
// and |Y|^2 in double (a lane its 16-byte runs in ascending order, the lanes by a fixed tree), the cosine
// <X, Y> / sqrt((|X|^2 + eps)(|Y|^2 + eps)), stores it as a float and adds it to its sum; the four waves in wave order
__global__ __launch_bounds__(256) void remd_value_kernel(RemdTerm t, double epsilon, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int side = (int)blockIdx.y;
    const int cnt = side ? t.y.count : t.x.count, other = side ? t.x.count : t.y.count;
    const int* nn = side ? t.nnB : t.nnA;
    float* cs = side ? t.cosB : t.cosA;
    const int per = (cnt + REMD_VALUE_BLOCKS - 1) / REMD_VALUE_BLOCKS;
    const long long k0 = (long long)blockIdx.x * per;
    long long k1 = k0 + per;
    if (k1 > cnt) k1 = cnt;
    const int c4n = t.x.C >> 2;
    double acc = 0.0;
    for (long long kk = k0 + wave; kk < k1; kk += 4) {
        const int k = (int)kk;
        int o = nn[k];
        o = o < 0 ? 0 : (o >= other ? other - 1 : o);
        const float* px = sample_ptr(t.x, side ? o : k);
        const float* py = sample_ptr(t.y, side ? k : o);
        double xy = 0.0, xx = 0.0, yy = 0.0;
        for (int u = lane; u < c4n; u += 64) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(px + u * 4);
            const f32x4 b = *reinterpret_cast<const f32x4*>(py + u * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xy += (double)a[e] * (double)b[e];
                xx += (double)a[e] * (double)a[e];
                yy += (double)b[e] * (double)b[e];
            }
        }
        xy = wave_sum(xy); xx = wave_sum(xx); yy = wave_sum(yy);
        const double c = xy / sqrt((xx + epsilon) * (yy + epsilon));
        if (lane == 0) cs[k] = (float)c;
        acc += c;
    }
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[side * REMD_VALUE_BLOCKS + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// stage two: each side's REMD_VALUE_BLOCKS partials by a fixed tree; rA = 1 - sum / n, rB = 1 - sum / m; the side and the value
__global__ __launch_bounds__(REMD_VALUE_BLOCKS) void remd_value_finish_kernel(const double* __restrict__ partial, double n, double m, int force,
                                                                              float* __restrict__ rec, int* __restrict__ side, float* __restrict__ val) {
    __shared__ double sh[2][REMD_VALUE_BLOCKS];
    const int tid = threadIdx.x;
    sh[0][tid] = partial[tid];
    sh[1][tid] = partial[REMD_VALUE_BLOCKS + tid];
    __syncthreads();
    for (int off = REMD_VALUE_BLOCKS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            sh[0][tid] += sh[0][tid + off];
            sh[1][tid] += sh[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double rA = 1.0 - sh[0][0] / n, rB = 1.0 - sh[1][0] / m;
        const int sd = force == 0 || force == 1 ? force : (rA >= rB ? 0 : 1);
        const float v = (float)(sd ? rB : rA);
        rec[0] = v; rec[1] = (float)rA; rec[2] = (float)rB;
        *side = sd;
        if (val) *val = v;
    }
}

// ---- the gradient at fixed matches, gather form -----------------------------------------------------------------------------
// one wave per image sample i, lane l the 16-byte channel runs l and l + 64.  d(i, j) = rp_i ((cos rp_i) X_i - rq_j Y_j), fp32,
// one rounding per operation.  Side A: coefA d(i, nnA(i)).  Side B: the wave scans nnB 64 entries at a time with a ballot and
// takes the j with nnB(j) = i in ascending order: coefB sum_j d(i, j) (no such j: zero).
__global__ __launch_bounds__(256) void remd_grad_kernel(RemdTerm t, float coefA, float coefB, float* __restrict__ out, int accumulate) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= t.x.count) return;
    const int c4n = t.x.C >> 2, m = t.y.count;
    const size_t off = (size_t)(sample_ptr(t.x, i) - t.x.f);
    const float rp = t.x.r[i];
    const bool has0 = lane < c4n, has1 = lane + 64 < c4n;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 x0 = has0 ? *reinterpret_cast<const f32x4*>(t.x.f + off + lane * 4) : zero;
    const f32x4 x1 = has1 ? *reinterpret_cast<const f32x4*>(t.x.f + off + (lane + 64) * 4) : zero;
    f32x4 g0 = zero, g1 = zero;
    if (*t.side == 0) {
        int j = t.nnA[i];
        j = j < 0 ? 0 : (j >= m ? m - 1 : j);
        const float* y = sample_ptr(t.y, j);
        const float rq = t.y.r[j], cr = t.cosA[i] * rp;
        if (has0) g0 = ((x0 * cr - *reinterpret_cast<const f32x4*>(y + lane * 4) * rq) * rp) * coefA;
        if (has1) g1 = ((x1 * cr - *reinterpret_cast<const f32x4*>(y + (lane + 64) * 4) * rq) * rp) * coefA;
    } else {
        f32x4 a0 = zero, a1 = zero;
        for (int base = 0; base < m; base += 64) {
            const int j1 = base + lane;
            unsigned long long mask = __ballot(j1 < m && t.nnB[j1] == i);
            while (mask) {
                const int j = base + __builtin_ctzll(mask);
                mask &= mask - 1;
                const float* y = sample_ptr(t.y, j);
                const float rq = t.y.r[j], cr = t.cosB[j] * rp;
                if (has0) a0 = a0 + (x0 * cr - *reinterpret_cast<const f32x4*>(y + lane * 4) * rq) * rp;
                if (has1) a1 = a1 + (x1 * cr - *reinterpret_cast<const f32x4*>(y + (lane + 64) * 4) * rq) * rp;
            }
        }
        g0 = a0 * coefB;
        g1 = a1 * coefB;
    }
    float* dst = out + off;
    if (has0) {
        if (accumulate) g0 = *reinterpret_cast<const f32x4*>(dst + lane * 4) + g0;
        *reinterpret_cast<f32x4*>(dst + lane * 4) = g0;
    }
    if (has1) {
        if (accumulate) g1 = *reinterpret_cast<const f32x4*>(dst + (lane + 64) * 4) + g1;
        *reinterpret_cast<f32x4*>(dst + (lane + 64) * 4) = g1;
    }
}

bool remd_channels_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

bool side_ok(const RemdSide& s) {
    return s.f && s.count >= 1 && remd_channels_ok(s.C) && s.stride >= 1 && s.nb >= 1 && s.na >= 1 && (long long)s.na * s.nb == s.count &&
           (long long)(s.na - 1) * s.stride < s.h && (long long)(s.nb - 1) * s.stride < s.w;
}

// the dynamic-LDS limit of one shape, for its widest map (C = 512 / NCT)
template <int NCT>
hipError_t remd_search_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&remd_search_kernel<NCT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               RemdCfg<NCT>::lds_bytes(512 / NCT));
}

template <int NCT>
hipError_t remd_search_launch(const RemdSearch& p, hipStream_t stream) {
    using Cf = RemdCfg<NCT>;
    const int tiles = (p.c.count + Cf::COLS - 1) / Cf::COLS, dt = remd_tiles(p.d.count);
    // the dictionary walk split over workgroups until the grid has about two workgroups per CU's worth of waves, every wave
    // keeping at least one tile
    int nsplit = (512 + tiles - 1) / tiles;
    const int cap = (dt + 7) / 8;
    if (nsplit > cap) nsplit = cap;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 65535) nsplit = 65535;
    hipLaunchKernelGGL((remd_search_kernel<NCT>), dim3((unsigned)tiles, (unsigned)nsplit), dim3(512), (size_t)Cf::lds_bytes(p.d.C), stream, p);
    return hipGetLastError();
}

}  // namespace

// once per device, before the first launch there (the search kernels take more than 64 KB of dynamic LDS)
hipError_t remd_init_device() {
    hipError_t e = remd_search_attr<1>();
    if (e == hipSuccess) e = remd_search_attr<2>();
    if (e == hipSuccess) e = remd_search_attr<4>();
    return e;
}

size_t remd_packed_bytes(int count, int C) { return (size_t)remd_tiles(count) * (size_t)(C / 16) * 2048; }

bool remd_side_geometry(int h, int w, int C, int stride, RemdSide* s) {
    if (h < 1 || w < 1 || stride < 1 || stride > 256 || !remd_channels_ok(C)) return false;
    if ((double)h * (double)w * (double)C >= 2147483648.0) return false;
    s->h = h; s->w = w; s->C = C; s->stride = stride;
    s->na = (h - 1) / stride + 1;
    s->nb = (w - 1) / stride + 1;
    s->count = s->na * s->nb;
    return true;
}

hipError_t launch_remd_norms(const RemdSide& s, double epsilon, float* r, hipStream_t stream) {
    if (!side_ok(s) || !r || !(epsilon > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(remd_norm_kernel, dim3((unsigned)(remd_tiles(s.count) * 8)), dim3(256), 0, stream, s, epsilon, r);
    return hipGetLastError();
}

hipError_t launch_remd_pack(const RemdSide& s, void* packed, hipStream_t stream) {
    if (!side_ok(s) || !s.amax || !packed) return hipErrorInvalidValue;
    const size_t total = (size_t)remd_tiles(s.count) * 32 * (s.C / 8);
    const size_t want = (total + 255) / 256;
    hipLaunchKernelGGL(remd_pack_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, stream, s, static_cast<unsigned char*>(packed));
    return hipGetLastError();
}

hipError_t launch_remd_search(const RemdSide& dict, const RemdSide& cols, unsigned long long* keys, int* nn, hipStream_t stream) {
    if (!side_ok(dict) || !side_ok(cols) || dict.C != cols.C || !dict.amax || !dict.r || !dict.packed || !cols.amax || !cols.r || !keys || !nn)
        return hipErrorInvalidValue;
    hipError_t e = launch_zero(keys, 2 * (size_t)cols.count, stream);
    if (e != hipSuccess) return e;
    const RemdSearch p{dict, cols, keys};
    e = dict.C == 512 ? remd_search_launch<1>(p, stream) : (dict.C == 256 ? remd_search_launch<2>(p, stream) : remd_search_launch<4>(p, stream));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(remd_decode_kernel, dim3((unsigned)((cols.count + 255) / 256)), dim3(256), 0, stream, keys, cols.count, dict.count, nn);
    return hipGetLastError();
}

static bool remd_term_ok(const RemdTerm& t) {
    return side_ok(t.x) && side_ok(t.y) && t.x.C == t.y.C && t.nnA && t.nnB && t.cosA && t.cosB && t.rec && t.side;
}

hipError_t launch_remd_value(const RemdTerm& t, double epsilon, int force, double* partial, float* val, hipStream_t stream) {
    if (!remd_term_ok(t) || !partial || !(epsilon > 0.0) || force < -1 || force > 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(remd_value_kernel, dim3(REMD_VALUE_BLOCKS, 2), dim3(256), 0, stream, t, epsilon, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(remd_value_finish_kernel, dim3(1), dim3(REMD_VALUE_BLOCKS), 0, stream, partial, (double)t.x.count, (double)t.y.count, force,
                       t.rec, t.side, val);
    return hipGetLastError();
}

hipError_t launch_remd_grad(const RemdTerm& t, float coefA, float coefB, float* out, int accumulate, hipStream_t stream) {
    if (!remd_term_ok(t) || !t.x.r || !t.y.r || !out) return hipErrorInvalidValue;
    if (!accumulate) {
        const hipError_t e = launch_zero(out, (size_t)t.x.h * t.x.w * t.x.C, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(remd_grad_kernel, dim3((unsigned)((t.x.count + 3) / 4)), dim3(256), 0, stream, t, coefA, coefB, out, accumulate);
    return hipGetLastError();
}

}  // namespace nst
