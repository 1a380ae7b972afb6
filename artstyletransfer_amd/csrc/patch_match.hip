// patch_match.hip - the MRF style term (Li & Wand 2016; include/nst_hip.h has the definition): every 3x3xC patch of a map
// is matched to its nearest neighbour, by normalised cross-correlation, among the 3x3xC patches of the style's map.
//
//   pm_rq_kernel       dictionary preparation: rq_j = 1 / sqrt(|Q_j|^2 + epsilon), the norm summed in double
//   pm_pack_kernel     dictionary preparation: the style patches cut into two scaled fp16 pieces (the cut and the power-of-two
//                      scale of conv_h2.hip) and laid out in the lane order of the MFMA's row operand
//   pm_search_kernel   the search: an implicit GEMM, rows = dictionary entries, columns = image patches, K = 9 C as
//                      (tap, 16 channels), on v_mfma_f32_32x32x16_f16 with three MFMAs per product block; the epilogue
//                      scales a row by rq_j and folds it into a running (score, index) key per column; the guided
//                      instantiation (SEM) also scales by the column's rp_i and adds gamma <d_i, e_j>
//   pm_desc_kernel     the semantic descriptors of the guided search (nst_level_set_patch_guidance): per patch the nine-tap sums
//                      of R pooled planes, normalised, as four floats
//   pm_decode_kernel   keys -> nn (int32) and score
//   pm_value_kernel    sum_i |P_i - Q_nn(i)|^2 in double, two ordered stages (pm_value_finish_kernel: the second)
//   pm_grad_kernel     the gradient at fixed nn, in gather form: nine taps per pixel, 16-byte channel runs
//
// Why rows are the dictionary: a 32x32 accumulator has its column on the lane and its rows in the 16 registers, so the
// arg-max over dictionary entries of one image patch is a loop over a lane's own registers, and the two lane halves meet
// once at the end.  The score matrix exists in accumulators only.
//
// Reproducibility: the only combine across waves and workgroups is an integer atomicMax on a 64-bit key (the order-preserving
// bit pattern of the score above ~j), which is independent of arrival order and resolves equal scores to the lowest j.
// There is no float atomic here.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "nst_kernels.h"
#include "nst_pieces.h"

namespace nst {

namespace {

// centre of dictionary entry j
__device__ __forceinline__ void dict_centre(const PatchDict& d, int j, int& cy, int& cx) {
    const int a = j / d.nb, b = j - a * d.nb;
    cy = 1 + a * d.stride;
    cx = 1 + b * d.stride;
}

// ---- dictionary preparation ---------------------------------------------------------------------------------------------
// one wave per entry; the padding entries of the last tile get rq = 0.  The guided search runs it on the image map too: a
// stride-1 geometry of the map has exactly the n image patches as its entries, and rp_i is rq_j's formula
__global__ __launch_bounds__(256) void pm_rq_kernel(PatchDict d, double epsilon, float* __restrict__ rq) {
    const int lane = threadIdx.x & 63;
    const int j = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= pm_dict_tiles(d.m) * 32) return;
    if (j >= d.m) {
        if (lane == 0) rq[j] = 0.f;
        return;
    }
    int cy, cx;
    dict_centre(d, j, cy, cx);
    const int c4n = d.C >> 2;
    double acc = 0.0;
    for (int u = lane; u < 9 * c4n; u += 64) {
        const int tap = u / c4n, c4 = u - tap * c4n;
        const int ty = tap / 3, tx = tap - ty * 3;
        const f32x4 v = *reinterpret_cast<const f32x4*>(d.fs + ((size_t)(cy - 1 + ty) * d.ws + (cx - 1 + tx)) * d.C + c4 * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)v[k] * (double)v[k];
    }
    acc = wave_sum(acc);
    if (lane == 0) rq[j] = (float)(1.0 / sqrt(acc + epsilon));
}

// one thread per (entry, 8 consecutive k): k = tap C + c.  packed: [tile of 32 entries][k-step of 16][piece][lane][8 fp16],
// lane = 32 (k % 16 / 8) + entry % 32 - the row operand of the 32x32x16 MFMA as a wave loads it, 1 KiB per piece and k-step
__global__ __launch_bounds__(256) void pm_pack_kernel(PatchDict d, unsigned char* __restrict__ packed) {
    const int lane = threadIdx.x & 63;
    float s, inv;
    tensor_scale(d.amax, lane, s, inv);
    const int k8n = 9 * d.C / 8, KS = 9 * d.C / 16;
    const size_t total = (size_t)pm_dict_tiles(d.m) * 32 * k8n;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (size_t)gridDim.x * 256) {
        const int j = (int)(u / k8n), k8 = (int)(u - (size_t)j * k8n);
        const int k = k8 * 8, tap = k / d.C, c = k - tap * d.C;
        const int ty = tap / 3, tx = tap - ty * 3;
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if (j < d.m) {
            int cy, cx;
            dict_centre(d, j, cy, cx);
            const float* src = d.fs + ((size_t)(cy - 1 + ty) * d.ws + (cx - 1 + tx)) * d.C + c;
            v0 = *reinterpret_cast<const f32x4*>(src);
            v1 = *reinterpret_cast<const f32x4*>(src + 4);
        }
        u32x2 h0, l0, h1, l1;
        cut2x4(v0, s, h0, l0);
        cut2x4(v1, s, h1, l1);
        const int t = j >> 5, ks = k >> 4, ln = ((k >> 3) & 1) * 32 + (j & 31);
        unsigned char* dst = packed + (((size_t)t * KS + ks) * 2) * 1024 + (size_t)ln * 16;
        *reinterpret_cast<u32x4*>(dst) = u32x4{h0[0], h0[1], h1[0], h1[1]};
        *reinterpret_cast<u32x4*>(dst + 1024) = u32x4{l0[0], l0[1], l1[0], l1[1]};
    }
}

// one thread per entry of a stride-`stride` geometry of the (R, hm, wm) planes, nb entries a row: a[r] = the nine taps of
// plane r in row-major order, d = (float)(a / sqrt(sum_r a[r]^2 + epsilon)), all in double; entries r >= R and the entries
// [count, padded) are zero
__global__ __launch_bounds__(256) void pm_desc_kernel(const float* __restrict__ planes, int R, int hm, int wm, int stride, int nb, int count,
                                                      int padded, double epsilon, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= padded) return;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if (j < count) {
        const int a = j / nb, b = j - a * nb;
        const int y0 = a * stride, x0 = b * stride;      // the patch's first pixel: its centre is (1 + a stride, 1 + b stride)
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        double ss = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r < R) {
                const float* pl = planes + ((size_t)r * hm + y0) * wm + x0;
                double t = 0.0;
#pragma unroll
                for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                    for (int tx = 0; tx < 3; ++tx) t += (double)pl[(size_t)ty * wm + tx];
                acc[r] = t;
                ss += t * t;
            }
        }
        const double nrm = sqrt(ss + epsilon);
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = r < R ? (float)(acc[r] / nrm) : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + (size_t)j * 4) = d;
}

// ---- the search ---------------------------------------------------------------------------------------------------------
// A workgroup (8 waves) owns 4 x 8 NCT image patches.  It stages their 6 x (8 NCT + 2) halo, all C channels, cut into the two
// pieces, once in LDS: a pixel's row holds per 8 channels 16 B of hi and 16 B of lo, C / 8 such groups, + 16 B pad (an odd
// multiple of 16 B, so consecutive pixels start on distinct 16-byte slots).  NCT = 512 / C capped at 4 keeps the image under
// 124 KB for every C.  The waves then share the dictionary walk: wave g of the grid's 8 nsplit takes the tiles g, g + 8 nsplit,
// ...; a tile's row fragments come straight from global memory (two 1-KiB loads per k-step, prefetched PF k-steps ahead), the
// column fragments from LDS.  Registers per lane: 32 NCT accumulators, 16 PF row fragments in flight, 8 NCT column
// fragments, 2 NCT key words.
// SEM (the guided search, include/nst_hip.h): T(i, j) = cos(i, j) + gamma <d_i, e_j>.  The row's e_j is one 16-byte load beside
// the rq load; the column's d_i and rp_i are fetched in the epilogue, once per tile, and not held over the K loop (NCT = 4 has
// 206 of 256 VGPRs in use without them).  SEM = false is the unguided kernel as it was.
template <int NCT>
struct PmCfg {
    static constexpr int TY = 4, TX = 8 * NCT;
    static constexpr int HP = TY + 2, WP = TX + 2;
    static constexpr int PF = NCT == 1 ? 4 : 2;      // k-steps per prefetch group (9 C / 16 is a multiple of 4)
    static __host__ __device__ constexpr int rowb(int C) { return 4 * C + 16; }
    static __host__ __device__ constexpr int lds_bytes(int C) { return HP * WP * rowb(C); }
};

template <int NCT, bool SEM>
__global__ __launch_bounds__(512) void pm_search_kernel(std::conditional_t<SEM, PatchSearch, PatchSearchCore> p) {
    using Cf = PmCfg<NCT>;
    constexpr int PF = Cf::PF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int C = p.C, ROWB = Cf::rowb(C);
    const int tile_y = (int)blockIdx.x / p.tiles_x, tile_x = (int)blockIdx.x - tile_y * p.tiles_x;
    const int y0 = tile_y * Cf::TY, x0 = tile_x * Cf::TX;      // the halo's first pixel; patch (py, px) is centred at (y0 + py + 1, x0 + px + 1)
    float sF, invF, sQ, invQ;
    tensor_scale(p.amax_f, lane, sF, invF);
    tensor_scale(p.d.amax, lane, sQ, invQ);
    const float inv = invF * invQ;
    // the image patch tile with its halo, zeros outside the map
    {
        const int c4n = C >> 2;
        const int units = Cf::HP * Cf::WP * c4n;
        for (int u = tid; u < units; u += 512) {
            const int px = u / c4n, c4 = u - px * c4n;
            const int hy = px / Cf::WP, hx = px - hy * Cf::WP;
            const int gy = y0 + hy, gx = x0 + hx;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gy < p.h && gx < p.w) v = *reinterpret_cast<const f32x4*>(p.f + ((size_t)gy * p.w + gx) * C + c4 * 4);
            u32x2 hi, lo;
            cut2x4(v, sF, hi, lo);
            unsigned char* dst = smem + px * ROWB + (c4 >> 1) * 32 + (c4 & 1) * 8;
            *reinterpret_cast<u32x2*>(dst) = hi;
            *reinterpret_cast<u32x2*>(dst + 16) = lo;
        }
    }
    __syncthreads();

    const int r = lane & 31, hh = lane >> 5;
    const int KS = 9 * C / 16, G = KS / PF;
    const int cshift = p.cshift;                 // log2(C / 16)
    const int cmask = (1 << cshift) - 1;
    // column r of column tile ct is patch (r / 8, 8 ct + r % 8); its fragment of k-step (tap (ty, tx), channels c0 ..):
    // pixel (r / 8 + ty, 8 ct + r % 8 + tx), 8 channels from c0 + 8 hh
    const int lane_off = ((r >> 3) * Cf::WP + (r & 7)) * ROWB + hh * 32;
    const int ntiles = pm_dict_tiles(p.d.m);
    const int g0 = (int)blockIdx.y * 8 + wave, gstride = (int)gridDim.y * 8;
    const int mine = g0 < ntiles ? (ntiles - g0 + gstride - 1) / gstride : 0;
    unsigned long long best[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) best[ct] = 0ull;

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
            const int ks = g * PF + u;
            const int tap = ks >> cshift, cg = ks & cmask;          // 16-channel group cg of tap `tap`
            const int ty = tap / 3, tx = tap - ty * 3;
            const unsigned char* b = smem + lane_off + (ty * Cf::WP + tx) * ROWB + cg * 64;
            const f16x8 a_hi = __builtin_bit_cast(f16x8, ah[u]), a_lo = __builtin_bit_cast(f16x8, al[u]);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const f16x8 b_hi = *reinterpret_cast<const f16x8*>(b + ct * 8 * ROWB);
                const f16x8 b_lo = *reinterpret_cast<const f16x8*>(b + ct * 8 * ROWB + 16);
                accx[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, accx[ct], 0, 0, 0);
                accm[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, accm[ct], 0, 0, 0);
                accx[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, accx[ct], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < PF; ++u) { ah[u] = nh[u]; al[u] = nl[u]; }
        if (++g == G) {
            // the tile is complete: register e of a lane is row (e & 3) + 8 (e >> 2) + 4 hh, entry j = 32 tile + row
#pragma clang fp contract(off)
            const int j0 = (g0 + tl * gstride) * 32;
            // the guided search: d_i and rp_i of this lane's NCT columns (a column outside the map reads the nearest patch's:
            // its key is never written)
            f32x4 dcol[SEM ? NCT : 1];
            float rpcol[SEM ? NCT : 1];
            if constexpr (SEM) {
                const int wn = p.w - 2, hn = p.h - 2;
                const int py = y0 + (r >> 3) < hn ? y0 + (r >> 3) : hn - 1;
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const int px = x0 + ct * 8 + (r & 7) < wn ? x0 + ct * 8 + (r & 7) : wn - 1;
                    const size_t i = (size_t)py * wn + px;
                    dcol[ct] = *reinterpret_cast<const f32x4*>(p.gd + i * 4);
                    rpcol[ct] = p.rp[i];
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 rq = *reinterpret_cast<const f32x4*>(p.d.rq + j0 + 8 * q + 4 * hh);
                f32x4 erow[SEM ? 4 : 1];
                if constexpr (SEM) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) erow[e] = *reinterpret_cast<const f32x4*>(p.ge + (size_t)(j0 + 8 * q + 4 * hh + e) * 4);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = j0 + 8 * q + 4 * hh + e;
                    const unsigned low = ~(unsigned)j;
#pragma unroll
                    for (int ct = 0; ct < NCT; ++ct) {
                        float sc;
                        if constexpr (SEM) {
                            const float feat = (((accm[ct][4 * q + e] + accx[ct][4 * q + e] * LO_DOWN) * inv) * rq[e]) * rpcol[ct];
                            const float sem = ((dcol[ct][0] * erow[e][0] + dcol[ct][1] * erow[e][1]) + dcol[ct][2] * erow[e][2]) +
                                              dcol[ct][3] * erow[e][3];
                            sc = feat + p.gamma * sem + 0.f;
                        } else {
                            sc = ((accm[ct][4 * q + e] + accx[ct][4 * q + e] * LO_DOWN) * inv) * rq[e] + 0.f;      // (+ 0: -0 -> +0)
                        }
                        const unsigned long long key = ((unsigned long long)score_order(sc) << 32) | low;
                        if (j < p.d.m && key > best[ct]) best[ct] = key;
                    }
                }
            }
            g = 0;
            ++tl;
        }
    }
    // the two lane halves hold different rows of the same columns; then one atomicMax per patch and wave
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const unsigned long long o = __shfl_xor(best[ct], 32);
        const unsigned long long b = o > best[ct] ? o : best[ct];
        const int y = y0 + (r >> 3) + 1, x = x0 + ct * 8 + (r & 7) + 1;
        if (hh == 0 && b != 0ull && y <= p.h - 2 && x <= p.w - 2) atomicMax(p.keys + (size_t)(y - 1) * (p.w - 2) + (x - 1), b);
    }
}

__global__ __launch_bounds__(256) void pm_decode_kernel(const unsigned long long* __restrict__ keys, size_t n, int m, int* __restrict__ idx,
                                                        float* __restrict__ score) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = keys[i];
    const unsigned hi = (unsigned)(k >> 32);
    int j = (int)(~(unsigned)k);
    if (k == 0ull || j < 0 || j >= m) j = 0;
    if (idx) idx[i] = j;
    if (score) score[i] = k == 0ull ? 0.f : __uint_as_float((hi & 0x80000000u) ? (hi & 0x7FFFFFFFu) : ~hi);
}

// ---- the value: sum_i |P_i - Q_nn(i)|^2 ----------------------------------------------------------------------------------
// stage one: block b owns the patches [b per, (b + 1) per), wave v of it every fourth of them; a lane adds its 16-byte runs of
// a patch's 9 C differences, squared in double, patch after patch; the lanes by a fixed tree, the four waves in wave order
__global__ __launch_bounds__(256) void pm_value_kernel(PatchTerm t, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n = (size_t)(t.h - 2) * (t.w - 2);
    const size_t per = (n + PM_VALUE_BLOCKS - 1) / PM_VALUE_BLOCKS;
    const size_t i0 = (size_t)blockIdx.x * per;
    size_t i1 = i0 + per;
    if (i1 > n) i1 = n;
    const int c4n = t.d.C >> 2, C = t.d.C, wn = t.w - 2;
    double acc = 0.0;
    for (size_t i = i0 + wave; i < i1; i += 4) {
        const int py = (int)(i / wn), px = (int)(i - (size_t)py * wn);      // centre (py + 1, px + 1): the patch starts at (py, px)
        int j = t.idx[i];
        j = j < 0 ? 0 : (j >= t.d.m ? t.d.m - 1 : j);
        int cy, cx;
        dict_centre(t.d, j, cy, cx);
        for (int u = lane; u < 9 * c4n; u += 64) {
            const int tap = u / c4n, c4 = u - tap * c4n;
            const int ty = tap / 3, tx = tap - ty * 3;
            const f32x4 a = *reinterpret_cast<const f32x4*>(t.f + ((size_t)(py + ty) * t.w + (px + tx)) * C + c4 * 4);
            const f32x4 q = *reinterpret_cast<const f32x4*>(t.d.fs + ((size_t)(cy - 1 + ty) * t.d.ws + (cx - 1 + tx)) * C + c4 * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double dlt = (double)a[k] - (double)q[k];
                acc += dlt * dlt;
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// stage two: the PM_VALUE_BLOCKS partials by a fixed tree -> (float)(sum / (9 C n))
__global__ __launch_bounds__(PM_VALUE_BLOCKS) void pm_value_finish_kernel(const double* __restrict__ partial, double denom, float* __restrict__ out) {
    __shared__ double sh[PM_VALUE_BLOCKS];
    const int tid = threadIdx.x;
    sh[tid] = partial[tid];
    __syncthreads();
    for (int off = PM_VALUE_BLOCKS / 2; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    if (tid == 0) *out = (float)(sh[0] / denom);
}

// ---- the gradient at fixed nn, gather form --------------------------------------------------------------------------------
// one thread per (pixel, four channels): dF = coef sum over the taps (dy, dx), in the order dy = -1, 0, 1 outer and dx = -1, 0, 1
// inner, whose patch centre (y - dy, x - dx) exists, of F(y, x) - Fs(cy + dy, cx + dx); fp32, one rounding per operation
__global__ __launch_bounds__(256) void pm_grad_kernel(PatchTerm t, float coef, float* __restrict__ out, int accumulate) {
#pragma clang fp contract(off)
    const int C = t.d.C, c4n = C >> 2, wn = t.w - 2;
    const size_t total = (size_t)t.h * t.w * c4n;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (size_t)gridDim.x * 256) {
        const size_t pix = u / c4n;
        const int c4 = (int)(u - pix * c4n);
        const int y = (int)(pix / t.w), x = (int)(pix - (size_t)y * t.w);
        const f32x4 v = *reinterpret_cast<const f32x4*>(t.f + pix * C + c4 * 4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int dy = -1; dy <= 1; ++dy) {
            const int py = y - dy;
            if (py < 1 || py > t.h - 2) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int px = x - dx;
                if (px < 1 || px > t.w - 2) continue;
                int j = t.idx[(size_t)(py - 1) * wn + (px - 1)];
                j = j < 0 ? 0 : (j >= t.d.m ? t.d.m - 1 : j);
                int cy, cx;
                dict_centre(t.d, j, cy, cx);
                const f32x4 q = *reinterpret_cast<const f32x4*>(t.d.fs + ((size_t)(cy + dy) * t.d.ws + (cx + dx)) * C + c4 * 4);
                acc = acc + (v - q);
            }
        }
        f32x4 gr = acc * coef;
        float* dst = out + pix * C + c4 * 4;
        if (accumulate) gr = *reinterpret_cast<const f32x4*>(dst) + gr;
        *reinterpret_cast<f32x4*>(dst) = gr;
    }
}

bool pm_channels_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

// the dynamic-LDS limit of one shape, for its widest map (C = 512 / NCT)
template <int NCT, bool SEM>
hipError_t pm_search_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&pm_search_kernel<NCT, SEM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               PmCfg<NCT>::lds_bytes(512 / NCT));
}

template <int NCT, bool SEM>
hipError_t pm_search_launch(PatchSearch p, hipStream_t stream) {
    using Cf = PmCfg<NCT>;
    p.tiles_y = (p.h - 2 + Cf::TY - 1) / Cf::TY;
    p.tiles_x = (p.w - 2 + Cf::TX - 1) / Cf::TX;
    const int tiles = p.tiles_x * p.tiles_y, dt = pm_dict_tiles(p.d.m);
    // the dictionary walk split over workgroups until the grid has about two workgroups per CU's worth of waves, every wave
    // keeping at least one tile
    int nsplit = (512 + tiles - 1) / tiles;
    const int cap = (dt + 7) / 8;
    if (nsplit > cap) nsplit = cap;
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 65535) nsplit = 65535;
    hipLaunchKernelGGL((pm_search_kernel<NCT, SEM>), dim3((unsigned)tiles, (unsigned)nsplit), dim3(512), (size_t)Cf::lds_bytes(p.C), stream, p);
    return hipGetLastError();
}

template <bool SEM>
hipError_t pm_search_by_channels(const PatchSearch& p, hipStream_t stream) {
    return p.C == 512 ? pm_search_launch<1, SEM>(p, stream) : (p.C == 256 ? pm_search_launch<2, SEM>(p, stream) : pm_search_launch<4, SEM>(p, stream));
}

}  // namespace

// once per device, before the first launch there (the search kernels take more than 64 KB of dynamic LDS)
hipError_t pm_init_device() {
    hipError_t e = pm_search_attr<1, false>();
    if (e == hipSuccess) e = pm_search_attr<2, false>();
    if (e == hipSuccess) e = pm_search_attr<4, false>();
    if (e == hipSuccess) e = pm_search_attr<1, true>();
    if (e == hipSuccess) e = pm_search_attr<2, true>();
    if (e == hipSuccess) e = pm_search_attr<4, true>();
    return e;
}

size_t pm_packed_bytes(int m, int C) { return (size_t)pm_dict_tiles(m) * (size_t)(9 * C / 16) * 2048; }

bool pm_dict_geometry(int hs, int ws, int C, int stride, PatchDict* d) {
    if (hs < 3 || ws < 3 || stride < 1 || stride > 8 || !pm_channels_ok(C)) return false;
    d->hs = hs; d->ws = ws; d->C = C; d->stride = stride;
    d->na = (hs - 3) / stride + 1;
    d->nb = (ws - 3) / stride + 1;
    const long long m = (long long)d->na * d->nb;
    if (m > (1ll << 30)) return false;
    d->m = (int)m;
    return true;
}

hipError_t launch_pm_norms(const PatchDict& d, double epsilon, float* out, hipStream_t stream) {
    if (!d.fs || !out || d.m < 1 || !pm_channels_ok(d.C) || !(epsilon > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pm_rq_kernel, dim3((unsigned)(pm_dict_tiles(d.m) * 8)), dim3(256), 0, stream, d, epsilon, out);
    return hipGetLastError();
}

hipError_t launch_pm_descriptors(const float* planes, int R, int hm, int wm, int stride, double epsilon, int padded, float* out,
                                 hipStream_t stream) {
    if (!planes || !out || R < 1 || R > 4 || hm < 3 || wm < 3 || stride < 1 || stride > 8 || !(epsilon > 0.0)) return hipErrorInvalidValue;
    const int na = (hm - 3) / stride + 1, nb = (wm - 3) / stride + 1;
    const long long count = (long long)na * nb;
    if (count > (1ll << 30) || padded < count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pm_desc_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, stream, planes, R, hm, wm, stride, nb, (int)count,
                       padded, epsilon, out);
    return hipGetLastError();
}

hipError_t launch_pm_prepare(const PatchDict& d, double epsilon, unsigned* amax, float* rq, void* packed, hipStream_t stream) {
    if (!d.fs || !amax || !rq || !packed || d.m < 1 || !pm_channels_ok(d.C) || !(epsilon > 0.0)) return hipErrorInvalidValue;
    hipError_t e = launch_zero(amax, NST_AMAX_SLOTS, stream);
    if (e != hipSuccess) return e;
    e = launch_absmax_slots(d.fs, (size_t)d.hs * d.ws * d.C, amax, stream);
    if (e != hipSuccess) return e;
    PatchDict dd = d;
    dd.amax = amax; dd.rq = rq; dd.packed = packed;
    const int padded = pm_dict_tiles(d.m) * 32;
    e = launch_pm_norms(dd, epsilon, rq, stream);
    if (e != hipSuccess) return e;
    const size_t total = (size_t)padded * (9 * d.C / 8);
    const size_t want = (total + 255) / 256;
    hipLaunchKernelGGL(pm_pack_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, stream, dd, static_cast<unsigned char*>(packed));
    return hipGetLastError();
}

hipError_t launch_pm_search(const PatchSearch& p0, int* idx, float* score, hipStream_t stream) {
    PatchSearch p = p0;
    if (!p.f || !p.amax_f || !p.keys || !p.d.fs || !p.d.amax || !p.d.rq || !p.d.packed || p.h < 3 || p.w < 3 || p.d.m < 1 ||
        p.C != p.d.C || !pm_channels_ok(p.C))
        return hipErrorInvalidValue;
    // the guidance: all of gd, ge, rp (and a finite gamma >= 0), or none of them
    const bool guided = p.gd || p.ge || p.rp;
    if (guided && (!p.gd || !p.ge || !p.rp || !(p.gamma >= 0.f) || p.gamma > 3.0e38f)) return hipErrorInvalidValue;
    const size_t n = (size_t)(p.h - 2) * (p.w - 2);
    p.cshift = p.C == 64 ? 2 : (p.C == 128 ? 3 : (p.C == 256 ? 4 : 5));
    hipError_t e = launch_zero(p.keys, 2 * n, stream);
    if (e != hipSuccess) return e;
    e = guided ? pm_search_by_channels<true>(p, stream) : pm_search_by_channels<false>(p, stream);
    if (e != hipSuccess) return e;
    if (!idx && !score) return hipSuccess;
    hipLaunchKernelGGL(pm_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p.keys, n, p.d.m, idx, score);
    return hipGetLastError();
}

static bool pm_term_ok(const PatchTerm& t) {
    return t.f && t.idx && t.d.fs && t.h >= 3 && t.w >= 3 && t.d.m >= 1 && pm_channels_ok(t.d.C);
}

hipError_t launch_pm_value_partials(const PatchTerm& t, double* partial, hipStream_t stream) {
    if (!pm_term_ok(t) || !partial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pm_value_kernel, dim3(PM_VALUE_BLOCKS), dim3(256), 0, stream, t, partial);
    return hipGetLastError();
}

hipError_t launch_pm_value(const double* partial, double denom, float* out, hipStream_t stream) {
    if (!partial || !out || !(denom > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pm_value_finish_kernel, dim3(1), dim3(PM_VALUE_BLOCKS), 0, stream, partial, denom, out);
    return hipGetLastError();
}

hipError_t launch_pm_grad(const PatchTerm& t, float coef, float* out, int accumulate, hipStream_t stream) {
    if (!pm_term_ok(t) || !out) return hipErrorInvalidValue;
    const size_t total = (size_t)t.h * t.w * (t.d.C / 4);
    const size_t want = (total + 255) / 256;
    hipLaunchKernelGGL(pm_grad_kernel, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(256), 0, stream, t, coef, out, accumulate);
    return hipGetLastError();
}

}  // namespace nst
