// xcorr.hip - the long-range style term (Berger & Memisevic 2017; include/nst_hip.h has the definition): Gram matrices of a map
// against a spatially shifted copy of itself, G_d = (1/Z_d) sum_p F(p + d) F(p)^T over the pixels p whose partner p + d lies in
// the map.
//
// Value pass: gram.hip's f16x2 arithmetic (two fp16 pieces under the map's one recorded absmax, three v_mfma_f32_32x32x16_f16 per
// 32x32x16 block, main and cross accumulators apart) on TWO staged pixel windows of the same map: side 0 holds the window at
// p + dy w + dx (the rows of G_d), side 1 the window at p (its columns).  G_d is not symmetric, so all T x T tile pairs are
// computed; a pixel p whose x >= w - dx has no partner in its row and is staged as zeros on side 1, so its pairs contribute
// exactly 0; the pixels behind the last pair, (h - dy) w - dx, are never staged.  Each side has its own buffer descriptor, both
// of the split's length, so the shifted window of a split's last pixels reaches into the next split's.  Ordered two-stage
// reduction over the splits: no float atomics, bitwise reproducible.
// Gradient: dF(q) = sum_d ([x >= dx, y >= dy] F(q - d) S_d^T + [x < w - dx, y < h - dy] F(q + d) S_d), one pixel-major GEMM with
// K = 2 C |D| on v_mfma_f32_32x32x2_f32 (fp32 operands), the masks applied while the pixel rows are staged.
#include <hip/hip_runtime.h>

#include "nst_kernels.h"

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- value pass --------------------------------------------------------------------------------------------------------
// LDS image of a chunk of XCORR_KP = 32 pairs: row = [side][channel of the tile], 144 bytes = [piece: hi, lo][32 pixels] fp16 +
// 16 bytes of pad (gram.hip's row: conflict-free ds_read_b128 fragments), two buffers.
constexpr int XC_ROWB = 144;
template <int TS>
struct XcorrCfg {
    static constexpr int NB = TS / 64;                        // 32x32 blocks per wave and side: 2x2 (TS = 128) or 1x1 (TS = 64)
    static constexpr int PER_T = TS * (XCORR_KP / 8) / 256;   // (channel, 8-pixel group) units per thread and side
    static constexpr int BUF_BYTES = 2 * TS * XC_ROWB;
};
constexpr int XC_LDS_BYTES = 2 * XcorrCfg<128>::BUF_BYTES;   // 72 KiB: two workgroups per CU

template <int TS>
__device__ __forceinline__ void xcorr_body(const XcorrItem& it, const int bid) {
    using G = XcorrCfg<TS>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_xc[];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int C = it.C, w = it.w, dx = it.dx;
    const int T = C / TS;

    const int split = bid % it.nsplit;
    const int tp = bid / it.nsplit;
    const int ti = tp / T, tj = tp - ti * T;      // rows of G_d: the shifted window's channels; columns: the window's at p

    const int np = (it.h - it.dy) * w - dx;       // pairs are the pixels p < np with x < w - dx
    const int off = it.dy * w + dx;
    const int p0 = split * it.pix_per_split;
    int p1 = p0 + it.pix_per_split;
    if (p1 > np) p1 = np;
    const int npix = p0 < p1 ? p1 - p0 : 0;
    const int nchunks = (npix + XCORR_KP - 1) / XCORR_KP;

    // scale from the recorded absmax (gram.hip's rule)
    float sc, inv;
    {
        unsigned m = it.amax[lane];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned v = (unsigned)__shfl_xor((int)m, o);
            m = v > m ? v : m;
        }
        int e = (int)((m >> 23) & 0xFFu);
        e = e < 32 ? 32 : (e > 250 ? 250 : e);
        sc = __uint_as_float((unsigned)(268 - e) << 23);
        inv = __uint_as_float((unsigned)(e - 14) << 23);
    }

    // side 0 reads pixels p0 + off .. p1 + off (inside the map: p1 + off <= h w), side 1 pixels p0 .. p1; behind either end the
    // range check returns zeros.  32-bit offsets inside one split (xcorr_geometry refuses larger ones).
    const unsigned bytes = (unsigned)((size_t)npix * (size_t)C * 4);
    const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(it.f) + ((size_t)p0 + off) * (size_t)C, 0, bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_u = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(it.f) + (size_t)p0 * (size_t)C, 0, bytes, 0x00020000);

    float st[2][G::PER_T][8];
    // x of the first pixel of each of the thread's units in the chunk that load() stages next, and the step from chunk to chunk
    int xb[G::PER_T];
#pragma unroll
    for (int i = 0; i < G::PER_T; ++i) xb[i] = (p0 + ((tid + i * 256) / TS) * 8) % w;
    const int kstep = XCORR_KP % w;
    const int xlim = w - dx;
    int next = 0;
    auto load = [&]() {
        const unsigned base = (unsigned)((size_t)next * XCORR_KP * (size_t)C * 4);
#pragma unroll
        for (int i = 0; i < G::PER_T; ++i) {
            const int u = tid + i * 256;
            const int ch = u % TS, gg = u / TS;
            const unsigned vs = (unsigned)(((gg * 8) * C + ti * TS + ch) * 4);
            const unsigned vu = (unsigned)(((gg * 8) * C + tj * TS + ch) * 4);
            int x = xb[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // (the whole offset in the lane's own word: it is what the range check compares)
                const unsigned pj = base + (unsigned)(j * C * 4);
                st[0][i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_s, vs + pj, 0, 0));
                const float v = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_u, vu + pj, 0, 0));
                st[1][i][j] = x < xlim ? v : 0.f;      // (a pixel whose partner would lie in the next row)
                x = (x + 1 == w) ? 0 : x + 1;
            }
            int xn = xb[i] + kstep;
            xb[i] = xn >= w ? xn - w : xn;
        }
        ++next;
    };
    auto store = [&](int buf) {
        unsigned char* base = smem_xc + buf * G::BUF_BYTES;
#pragma unroll
        for (int sd = 0; sd < 2; ++sd)
#pragma unroll
            for (int i = 0; i < G::PER_T; ++i) {
                const int u = tid + i * 256;
                const int ch = u % TS, gg = u / TS;
                unsigned hi[4], lo[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const f32x2 x = {st[sd][i][2 * k] * sc, st[sd][i][2 * k + 1] * sc};
                    const f16x2 h = __builtin_convertvector(x, f16x2);
                    const f32x2 r = (x - __builtin_convertvector(h, f32x2)) * 2048.f;
                    const f16x2 l = __builtin_convertvector(r, f16x2);
                    hi[k] = __builtin_bit_cast(unsigned, h);
                    lo[k] = __builtin_bit_cast(unsigned, l);
                }
                unsigned char* dst = base + (sd * TS + ch) * XC_ROWB + gg * 16;
                *reinterpret_cast<u32x4*>(dst) = u32x4{hi[0], hi[1], hi[2], hi[3]};
                *reinterpret_cast<u32x4*>(dst + 64) = u32x4{lo[0], lo[1], lo[2], lo[3]};
            }
    };

    // the wave's NB x NB blocks of the tile pair: row blocks rb0 .., column blocks cb0 ..
    const int rb0 = G::NB * (wave & 1), cb0 = G::NB * (wave >> 1);
    int fa[G::NB], fb[G::NB];
#pragma unroll
    for (int a = 0; a < G::NB; ++a) {
        fa[a] = ((rb0 + a) * 32 + l31) * XC_ROWB + half * 16;
        fb[a] = (TS + (cb0 + a) * 32 + l31) * XC_ROWB + half * 16;
    }
    f32x16 accm[G::NB][G::NB], accx[G::NB][G::NB];
#pragma unroll
    for (int a = 0; a < G::NB; ++a)
#pragma unroll
        for (int b = 0; b < G::NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accm[a][b][r] = 0.f; accx[a][b][r] = 0.f; }

    if (nchunks > 0) {
        load();
        store(0);
        if (nchunks > 1) load();
    }
    __syncthreads();
    // per accumulator pair the Gram pass's order: chunk by chunk, k-step 0 then 1, in a k-step cross (lo x hi), main (hi x hi),
    // cross (hi x lo)
    for (int c = 0; c < nchunks; ++c) {
        const int cbuf = c & 1;
        if (c + 1 < nchunks) {
            store(cbuf ^ 1);                  // the other buffer was last read in chunk c-1, which every wave has left
            if (c + 2 < nchunks) load();
        }
        const unsigned char* base = smem_xc + cbuf * G::BUF_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f16x8 A[G::NB][2], B[G::NB][2];      // [block][piece: hi, lo]
#pragma unroll
            for (int a = 0; a < G::NB; ++a)
#pragma unroll
                for (int pc = 0; pc < 2; ++pc) {
                    A[a][pc] = *reinterpret_cast<const f16x8*>(base + fa[a] + pc * 64 + ks * 32);
                    B[a][pc] = *reinterpret_cast<const f16x8*>(base + fb[a] + pc * 64 + ks * 32);
                }
#pragma unroll
            for (int a = 0; a < G::NB; ++a)
#pragma unroll
                for (int b = 0; b < G::NB; ++b) {
                    accx[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[a][1], B[b][0], accx[a][b], 0, 0, 0);
                    accm[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[a][0], B[b][0], accm[a][b], 0, 0, 0);
                    accx[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[a][0], B[b][1], accx[a][b], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    const float inv2 = inv * inv;
    float* slab = it.part + (size_t)split * C * C;
#pragma unroll
    for (int a = 0; a < G::NB; ++a)
#pragma unroll
        for (int b = 0; b < G::NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int row = ti * TS + (rb0 + a) * 32 + m;
                const int col = tj * TS + (cb0 + b) * 32 + l31;
                slab[(size_t)row * C + col] = fmaf(accx[a][b][r], 1.f / 2048.f, accm[a][b][r]) * inv2;
            }
}

// every (level, map, shift) of a closure in one grid: the workgroups are numbered item by item
__global__ __launch_bounds__(256, 2) void xcorr_partial_kernel(XcorrBatch b) {
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].part_end) ++i;
    const XcorrItem& it = b.it[i];
    const int bid = (int)blockIdx.x - (i ? b.it[i - 1].part_end : 0);
    if (it.C == 64) xcorr_body<64>(it, bid);
    else xcorr_body<128>(it, bid);
}

// G_d = (the slabs, added in slab order) / Z_d, the full matrix; with a target S_d = coef (G_d - Gt_d), its transpose, and the
// block's sum of (G_d - Gt_d)^2 in double (a fixed tree).  A block owns XCORR_FINISH_EPB consecutive elements, four per thread.
__global__ __launch_bounds__(256) void xcorr_finish_kernel(XcorrBatch b) {
    __shared__ double shd[256];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].finish_end) ++i;
    const XcorrItem& it = b.it[i];
    const unsigned bid = blockIdx.x - (unsigned)(i ? b.it[i - 1].finish_end : 0);
    const int C = it.C;
    const size_t CC = (size_t)C * C;
    const size_t e0 = (size_t)bid * XCORR_FINISH_EPB + (size_t)threadIdx.x * 4;      // (C % 4 == 0: the four share a row)
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 4 <= it.nsplit; k += 4) {
        f32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const f32x4*>(it.part + (size_t)(k + q) * CC + e0);
#pragma unroll
        for (int q = 0; q < 4; ++q) s += v[q];
    }
    for (; k < it.nsplit; ++k) s += *reinterpret_cast<const f32x4*>(it.part + (size_t)k * CC + e0);
    const int row = (int)(e0 / C), col = (int)(e0 % C);
    double sq = 0.0;
    f32x4 g, sv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        g[q] = s[q] / it.divisor;
        if (it.target) {
            const float d = g[q] - it.target[e0 + q];
            sq += (double)d * (double)d;
            sv[q] = it.coef * d;
            if (it.St) it.St[(size_t)(col + q) * C + row] = sv[q];
        }
    }
    if (it.G) *reinterpret_cast<f32x4*>(it.G + e0) = g;
    if (it.target && it.S) *reinterpret_cast<f32x4*>(it.S + e0) = sv;
    if (it.sq) {
        shd[threadIdx.x] = sq;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) shd[threadIdx.x] += shd[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) it.sq[bid] = shd[0];
    }
}

// xcorr_i = (1/|D|) sum_d mean_{c,e} (G_d - Gt_d)^2 of one map from the finish pass's partials (sq: |D| x nblk doubles): per
// shift thread t takes block t (nblk <= 256) and a fixed tree joins them, the shifts are added in ascending order
__global__ __launch_bounds__(256) void xcorr_value_kernel(XcorrValueBatch b) {
    __shared__ double shd[256];
    const XcorrValueItem& it = b.it[blockIdx.x];
    double acc = 0.0;
    for (int d = 0; d < it.nd; ++d) {
        double v = 0.0;
        for (int k = threadIdx.x; k < it.nblk; k += 256) v += it.sq[(size_t)d * it.nblk + k];
        shd[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) shd[threadIdx.x] += shd[threadIdx.x + o];
            __syncthreads();
        }
        acc += shd[0] / it.cc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *it.out = (float)(acc / (double)it.nd);
}

// the term's share of the loss rows (XcorrRows in nst_kernels.h): one thread, the additions in the definition's order
__global__ void xcorr_rows_kernel(XcorrRows r) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    bool first = true;
    float tot = 0.f;
    for (int l = 0; l < r.levels; ++l) {
        if (!r.lv[l].owned) {
            // (a level outside the closure's mask: its unweighted values read as zeros, as the loss assembly leaves the other terms')
            for (int i = 0; i < 6 && r.lv[l].vals; ++i) r.lv[l].vals[i] = 0.f;
            continue;
        }
        float total = r.out[4 * l];
        if (r.lv[l].vals) {
            for (int i = 0; i < 6; ++i)
                if (r.lv[l].w[i] > 0.f) total = total + r.lv[l].w[i] * r.lv[l].vals[i];
            r.out[4 * l] = total;
        }
        tot = first ? total : (1.0f * tot + total);
        first = false;
    }
    r.out[4 * r.levels] = first ? 0.f : tot;
}

// ---- gradient ------------------------------------------------------------------------------------------------------------
// out[q][n] (+)= sum over shifts d, the two segments and the channels k of A[q][k] B[k][n]:
//   segment 0: A = F(q - d) where x >= dx and y >= dy, else 0;   B[k][n] = S_d[n][k]  (read from the transposed stack St)
//   segment 1: A = F(q + d) where x < w - dx and y < h - dy, else 0;   B[k][n] = S_d[k][n]
// A workgroup owns 128 pixels x BN channels (BN = 128, or 64 for C = 64); its 2 x 2 waves 64 pixels x BN / 2 channels each.  A
// step stages 16 channels of k: the pixel rows transposed to [k][pixel] (lane l of the MFMA wants A[pixel l & 31][k = l >> 5]),
// the rows of S as they lie.  Registers prefetch step s + 1 while step s is multiplied; two LDS buffers, one barrier a step.
constexpr int XG_BM = 128, XG_BK = 16;
template <int BN>
__global__ __launch_bounds__(256) void xcorr_grad_kernel(XcorrGrad g) {
    constexpr int NT = BN / 64;               // 32-wide column blocks per wave
    constexpr int BV = BN / 64;               // f32x4 per thread of a staged S tile (16 rows x BN)
    __shared__ __attribute__((aligned(16))) float As[2][XG_BK * XG_BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][XG_BK * BN];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int C = g.C, w = g.w, h = g.h;
    const int N = h * w;
    const int ntn = C / BN;
    const int q0 = ((int)blockIdx.x / ntn) * XG_BM;
    const int n0 = ((int)blockIdx.x % ntn) * BN;
    const size_t CC = (size_t)C * C;

    // the pixel this thread stages (8 channels of it per step)
    const int am = tid & 127, akh = tid >> 7;
    const int q = q0 + am;
    const int qx = q % w, qy = q / w;
    // the S row and columns this thread stages
    const int br = tid >> 4, bc = (tid & 15) * (BN / 16);

    const int nkc = C / XG_BK;
    const int nsteps = g.nd * 2 * nkc;
    f32x4 ra[2], rb[BV];
    auto load = [&](int s) {
        const int ds = s / nkc, k0 = (s - ds * nkc) * XG_BK;
        const int d = ds >> 1, seg = ds & 1;
        const int dx = g.dx[d], dy = g.dy[d];
        const int o = dy * w + dx;
        const bool ok = q < N && (seg == 0 ? (qx >= dx && qy >= dy) : (qx < w - dx && qy < h - dy));
        ra[0] = f32x4{0.f, 0.f, 0.f, 0.f};
        ra[1] = ra[0];
        if (ok) {
            const float* src = g.f + (size_t)(seg == 0 ? q - o : q + o) * C + k0 + akh * 8;
            ra[0] = *reinterpret_cast<const f32x4*>(src);
            ra[1] = *reinterpret_cast<const f32x4*>(src + 4);
        }
        const float* sb = (seg == 0 ? g.St : g.S) + (size_t)d * CC + (size_t)(k0 + br) * C + n0 + bc;
#pragma unroll
        for (int v = 0; v < BV; ++v) rb[v] = *reinterpret_cast<const f32x4*>(sb + v * 4);
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) As[buf][(akh * 8 + v * 4 + j) * XG_BM + am] = ra[v][j];
#pragma unroll
        for (int v = 0; v < BV; ++v) *reinterpret_cast<f32x4*>(&Bs[buf][br * BN + bc + v * 4]) = rb[v];
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    if (nsteps > 0) load(0);
    int cur = 0;
    for (int s = 0; s < nsteps; ++s) {
        store(cur);
        __syncthreads();
        if (s + 1 < nsteps) load(s + 1);
        const float* arow = &As[cur][half * XG_BM + wm * 64 + l31];
        const float* brow = &Bs[cur][half * BN + wn * (NT * 32) + l31];
#pragma unroll
        for (int k2 = 0; k2 < XG_BK / 2; ++k2) {
            const float a0 = arow[k2 * 2 * XG_BM];
            const float a1 = arow[k2 * 2 * XG_BM + 32];
            float bv[NT];
#pragma unroll
            for (int b = 0; b < NT; ++b) bv[b] = brow[k2 * 2 * BN + b * 32];
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                acc[0][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[b], acc[0][b], 0, 0, 0);
                acc[1][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[b], acc[1][b], 0, 0, 0);
            }
        }
        cur ^= 1;
    }

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int qo = q0 + wm * 64 + a * 32 + m;
                if (qo >= N) continue;
                float* o = g.out + (size_t)qo * C + n0 + wn * (NT * 32) + b * 32 + l31;
                *o = g.accumulate ? *o + acc[a][b][r] : acc[a][b][r];
            }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
bool xcorr_geometry(int C, int h, int w, int dx, int dy, XcorrGeometry* g) {
    if (!(C == 64 || C == 128 || C == 256 || C == 512) || h < 1 || w < 1) return false;
    if (dx < 0 || dy < 0 || (dx == 0 && dy == 0) || dx >= w || dy >= h) return false;
    if ((size_t)h * w * C >= ((size_t)1 << 31)) return false;
    const size_t np = (size_t)(h - dy) * w - dx;
    const size_t chunks = (np + XCORR_KP - 1) / XCORR_KP;
    const int T = C / (C == 64 ? 64 : 128);
    // the items of a closure fill the chip together: 64 workgroups an item, and never more than 8 MiB of slabs
    size_t ns = (size_t)(64 / (T * T));
    const size_t by_bytes = ((size_t)8 << 20) / ((size_t)C * C * 4);
    if (ns > by_bytes) ns = by_bytes;
    if (ns > chunks) ns = chunks;
    if (ns < 1) ns = 1;
    const size_t cps = (chunks + ns - 1) / ns;
    g->nsplit = (int)((chunks + cps - 1) / cps);
    g->pix_per_split = (int)(cps * XCORR_KP);
    return (size_t)g->pix_per_split * (size_t)C * 4 < 0xFFFFFF00ull;
}

hipError_t xcorr_init_device() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&xcorr_partial_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, XC_LDS_BYTES);
    return e;
}

hipError_t launch_xcorr_batch(const XcorrBatch& b0, hipStream_t stream) {
    if (b0.n < 1 || b0.n > XCORR_BATCH_MAX) return hipErrorInvalidValue;
    XcorrBatch b = b0;
    for (int i = 0; i < b.n; ++i) {
        XcorrItem& it = b.it[i];
        XcorrGeometry geo;
        if (!it.f || !it.amax || !it.part || !xcorr_geometry(it.C, it.h, it.w, it.dx, it.dy, &geo)) return hipErrorInvalidValue;
        if (it.target && (!it.S || !it.St)) return hipErrorInvalidValue;
        const int T = it.C / (it.C == 64 ? 64 : 128);
        it.nsplit = geo.nsplit; it.pix_per_split = geo.pix_per_split;
        it.part_end = (i ? b.it[i - 1].part_end : 0) + T * T * geo.nsplit;
        it.finish_end = (i ? b.it[i - 1].finish_end : 0) + xcorr_finish_blocks(it.C);
    }
    hipLaunchKernelGGL(xcorr_partial_kernel, dim3(b.it[b.n - 1].part_end), dim3(256), XC_LDS_BYTES, stream, b);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(xcorr_finish_kernel, dim3(b.it[b.n - 1].finish_end), dim3(256), 0, stream, b);
    return hipGetLastError();
}

hipError_t launch_xcorr_values(const XcorrValueBatch& b, hipStream_t stream) {
    if (b.n < 1 || b.n > XCORR_VALUE_MAX) return hipErrorInvalidValue;
    for (int i = 0; i < b.n; ++i)
        if (!b.it[i].sq || !b.it[i].out || b.it[i].nd < 1 || b.it[i].nblk < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(xcorr_value_kernel, dim3(b.n), dim3(256), 0, stream, b);
    return hipGetLastError();
}

hipError_t launch_xcorr_rows(const XcorrRows& r, hipStream_t stream) {
    if (!r.out || r.levels < 1 || r.levels > 8) return hipErrorInvalidValue;
    hipLaunchKernelGGL(xcorr_rows_kernel, dim3(1), dim3(64), 0, stream, r);
    return hipGetLastError();
}

hipError_t launch_xcorr_grad(const XcorrGrad& g, hipStream_t stream) {
    if (!g.f || !g.S || !g.St || !g.out || g.nd < 1 || g.nd > XCORR_MAX_SHIFTS) return hipErrorInvalidValue;
    XcorrGeometry geo;
    for (int d = 0; d < g.nd; ++d)
        if (!xcorr_geometry(g.C, g.h, g.w, g.dx[d], g.dy[d], &geo)) return hipErrorInvalidValue;
    const int N = g.h * g.w;
    const int mt = (N + XG_BM - 1) / XG_BM;
    if (g.C == 64) hipLaunchKernelGGL(xcorr_grad_kernel<64>, dim3(mt), dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(xcorr_grad_kernel<128>, dim3(mt * (g.C / 128)), dim3(256), 0, stream, g);
    return hipGetLastError();
}

}  // namespace nst
