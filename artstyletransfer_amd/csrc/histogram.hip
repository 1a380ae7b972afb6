// The histogram loss (Risser, Wilmot & Barnes 2017; include/nst_hip.h has the definition): every channel of a tapped map is
// remapped so that its histogram becomes the style's, and the map is pulled towards its remap.  Kernels for gfx950:
//   hist_range_kernel     per-channel minimum and maximum of an NHWC map, one pass with 16-byte loads; a workgroup combines in
//                         LDS and the workgroups by integer atomicMin / atomicMax on the order-preserving bit pattern of the
//                         values (the MRF keys' pattern), so the range is exact and independent of arrival order
//   hist_counts_kernel    a workgroup owns a slab of 32 channels and a range of pixels; the slab's bins live in LDS as uint32
//                         [bin][32 channels], added to with LDS integer atomics, flushed with global integer adds
//   hist_tables_kernel    one workgroup per channel: prefix sums of the image's and the style's counts (uint64) and the two ends
//                         of every non-empty image bin, from integers and doubles
//   hist_value_kernel     sum (F - R)^2 in double, two ordered stages (hist_value_finish_kernel: the second)
//   hist_grad_kernel      dF = coef (F - R), written or added
// The LDS image of the counts pass.  Write-class LDS instructions bank by (address / 4) mod 32 and conflict within the two
// 32-lane halves of a wave.  Word bin * 32 + channel has bank = channel whatever the bin, and the 32 lanes of a half hold 32
// different channels in every atomic instruction: a lane has four channels 4 q .. 4 q + 3 (q = lane mod 8) of pixel r =
// lane / 8, and its k-th atomic takes channel 4 q + ((k + r) mod 4); over q = 0..7 and r mod 4 = 0..3 these are the 32
// channels once each.  So no atomic instruction has two lanes on one bank, not even where half of a post-ReLU map falls into
// bin 0.  32 channels x 1024 bins x 4 bytes = 128 KB, inside the CU's 160 KB.
// Reproducibility: range and counts combine by integer atomics only, the tables are integer and double arithmetic of one
// thread per bin, the value is summed in a fixed order.  No float atomic takes part.
#include <hip/hip_runtime.h>

#include "nst_kernels.h"

// every step of the definition is rounded once: no product of this file may fuse with the sum or difference that follows it
// (x - b after x = (v - lo) scale, start + f (end - start), slo + (j + t) width).  Plain operators under this pragma: the
// rounding intrinsics are inlined from a header compiled under the default contraction and fuse all the same.
#pragma clang fp contract(off)

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int HIST_RANGE_BLOCKS = 1024;
constexpr int HIST_GRAD_BLOCKS = 4096;
constexpr int HIST_COUNT_THREADS = 1024;    // one workgroup of the counts pass: 128 pixels x 8 lanes of four channels a step
constexpr int HIST_COUNT_GROUPS = 256;      // its workgroups over all slabs, at most: every one flushes bins x 32 words, and at
                                            // 1024 bins (128 KB of LDS) a CU holds one

__device__ __forceinline__ unsigned range_key(float v) {
    const unsigned u = __float_as_uint(v + 0.f);      // (-0 counts as +0)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float range_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);      // a fixed tree: every lane ends with the same sum
    return v;
}

// scale_c of the definition; 0 marks a flat channel (hi == lo: no term)
__device__ __forceinline__ float bin_scale(float lo, float hi, int bins) {
    return hi == lo ? 0.f : (float)((double)bins / ((double)hi - (double)lo));
}
// bin b and fraction f of value v
__device__ __forceinline__ void bin_of(float v, float lo, float scale, int bins, int& b, float& f) {
    const float d = v - lo;
    const float x = d * scale;
    b = (int)x;
    b = b > bins - 1 ? bins - 1 : (b < 0 ? 0 : b);
    f = fminf(1.f, x - (float)b);
}

// ---- the range -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hist_range_init_kernel(unsigned* __restrict__ keys, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * C) keys[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
}

// keys: C x 2 words (minimum key, maximum key).  The grid's stride is a multiple of C / 4, so a thread keeps its four channels.
__global__ __launch_bounds__(256) void hist_range_kernel(const float* __restrict__ f, size_t N, int C, unsigned* __restrict__ keys) {
    __shared__ unsigned sh[2 * 512];
    for (int i = threadIdx.x; i < 2 * C; i += 256) sh[i] = (i & 1) ? 0u : 0xFFFFFFFFu;
    __syncthreads();
    const int c4n = C >> 2;
    const size_t total = N * c4n;
    const size_t u0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u0 < total) {
        const int c4 = (int)(u0 % c4n);
        f32x4 mn = *reinterpret_cast<const f32x4*>(f + u0 * 4), mx = mn;
        for (size_t u = u0 + (size_t)gridDim.x * 256; u < total; u += (size_t)gridDim.x * 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(f + u * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mn[k] = fminf(mn[k], v[k]);
                mx[k] = fmaxf(mx[k], v[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicMin(&sh[2 * (c4 * 4 + k)], range_key(mn[k]));
            atomicMax(&sh[2 * (c4 * 4 + k) + 1], range_key(mx[k]));
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256) {
        if (i & 1) atomicMax(&keys[i], sh[i]);
        else atomicMin(&keys[i], sh[i]);
    }
}

__global__ __launch_bounds__(256) void hist_range_decode_kernel(unsigned* __restrict__ keys, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * C) keys[i] = __float_as_uint(range_value(keys[i]));
}

// ---- the counts ------------------------------------------------------------------------------------------------------------
// grid (pixel ranges, C / 32 slabs); `share` pixels per workgroup; dynamic LDS: bins x 32 words.  Four 16-byte loads of a lane
// are in flight before their atomics: 16 waves a CU keep 64 KB on the way.
__global__ __launch_bounds__(HIST_COUNT_THREADS) void hist_counts_kernel(const float* __restrict__ f, size_t N, int C, int bins, size_t share,
                                                          const float* __restrict__ lo_hi, unsigned* __restrict__ counts) {
    extern __shared__ unsigned img[];
    const int words = bins * HIST_SLAB;
    for (int i = threadIdx.x; i < words; i += HIST_COUNT_THREADS) img[i] = 0u;
    __syncthreads();
    constexpr int PIX = HIST_COUNT_THREADS / 8;
    const int q = threadIdx.x & 7, r = threadIdx.x >> 3;
    const int c0 = blockIdx.y * HIST_SLAB, cq = c0 + 4 * q;
    float lo[4], scale[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = lo_hi[2 * (cq + k)];
        scale[k] = bin_scale(lo[k], lo_hi[2 * (cq + k) + 1], bins);
    }
    const size_t p0 = (size_t)blockIdx.x * share;
    size_t p1 = p0 + share;
    if (p1 > N) p1 = N;
    const int rot = r & 3;
    for (size_t p = p0 + r; p < p1; p += 4 * PIX) {
        f32x4 vs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (p + u * PIX < p1) vs[u] = *reinterpret_cast<const f32x4*>(f + (p + u * PIX) * C + cq);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p + u * PIX >= p1) break;
            const f32x4 v = vs[u];
            int b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float fr;
                bin_of(v[k], lo[k], scale[k], bins, b[k], fr);
                if (scale[k] == 0.f) b[k] = -1;          // a flat channel counts nothing
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // the lane's k-th atomic takes its channel (k + r) mod 4: the 32 lanes of a half on 32 banks
                const int kk = (k + rot) & 3;
                const int bb = kk == 0 ? b[0] : (kk == 1 ? b[1] : (kk == 2 ? b[2] : b[3]));
                if (bb >= 0) atomicAdd(&img[bb * HIST_SLAB + 4 * q + kk], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += HIST_COUNT_THREADS) {
        const unsigned v = img[i];
        if (v) atomicAdd(&counts[(size_t)(c0 + (i & (HIST_SLAB - 1))) * bins + (i >> 5)], v);
    }
}

// ---- the tables ------------------------------------------------------------------------------------------------------------
// exclusive prefix sums of cnt[0..bins) into cum[0..bins] by 256 threads: chunks of K = ceil(bins / 256), then the chunk totals
__device__ __forceinline__ void prefix_sums(const unsigned* __restrict__ cnt, int bins, unsigned long long* cum, unsigned long long* tot) {
    const int K = (bins + 255) / 256, t = threadIdx.x;
    unsigned long long s = 0;
    for (int k = 0; k < K; ++k) {
        const int b = t * K + k;
        if (b < bins) s += cnt[b];
    }
    tot[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned long long add = t >= off ? tot[t - off] : 0ull;
        __syncthreads();
        tot[t] += add;
        __syncthreads();
    }
    unsigned long long run = t ? tot[t - 1] : 0ull;
    for (int k = 0; k < K; ++k) {
        const int b = t * K + k;
        if (b < bins) {
            cum[b] = run;
            run += cnt[b];
        }
    }
    if (t == 255) cum[bins] = tot[255];
    __syncthreads();
}

// one end: the smallest j with scum[j + 1] N > X (strict) or >= X, then (float)(slo + (j + t) width)
__device__ __forceinline__ float table_end(const unsigned long long* scum, const unsigned* __restrict__ scnt, int bins, unsigned long long X,
                                           unsigned long long N, bool strict, double slo, double width) {
    int a = 0, z = bins - 1;
    while (a < z) {
        const int mid = (a + z) >> 1;
        const unsigned long long v = scum[mid + 1] * N;
        if (strict ? v > X : v >= X) z = mid;
        else a = mid + 1;
    }
    const int j = a;
    const unsigned long long num = X - scum[j] * N, den = (unsigned long long)scnt[j] * N;
    const double t = den ? (double)num / (double)den : 0.0;
    const double pos = ((double)j + t) * width;
    return (float)(slo + pos);
}

__global__ __launch_bounds__(256) void hist_tables_kernel(const unsigned* __restrict__ counts, unsigned long long N,
                                                          const float* __restrict__ s_lo_hi, const unsigned* __restrict__ s_counts,
                                                          unsigned long long Ns, int bins, float* __restrict__ ends) {
    __shared__ unsigned long long cum[1025], scum[1025], tot[256];
    const int c = blockIdx.x;
    const unsigned* cnt = counts + (size_t)c * bins;
    const unsigned* scnt = s_counts + (size_t)c * bins;
    prefix_sums(cnt, bins, cum, tot);
    prefix_sums(scnt, bins, scum, tot);
    const float slo = s_lo_hi[2 * c], shi = s_lo_hi[2 * c + 1];
    const double width = ((double)shi - (double)slo) / (double)bins;
    const bool sflat = shi == slo || scum[bins] == 0ull;
    f32x2* out = reinterpret_cast<f32x2*>(ends) + (size_t)c * bins;
    for (int b = threadIdx.x; b < bins; b += 256) {
        f32x2 e = {0.f, 0.f};
        if (cnt[b]) {
            if (sflat) {
                e[0] = slo; e[1] = slo;
            } else {
                e[0] = table_end(scum, scnt, bins, cum[b] * Ns, N, true, (double)slo, width);
                e[1] = table_end(scum, scnt, bins, cum[b + 1] * Ns, N, false, (double)slo, width);
            }
        }
        out[b] = e;
    }
}

// ---- value and gradient ----------------------------------------------------------------------------------------------------
// R(v) of the definition: start + f (end - start), three roundings
__device__ __forceinline__ float remap(float v, float lo, float scale, int bins, const f32x2* __restrict__ ends_c) {
    int b;
    float fr;
    bin_of(v, lo, scale, bins, b, fr);
    const f32x2 e = ends_c[b];
    const float d = e[1] - e[0];
    const float p = fr * d;
    return e[0] + p;
}

// stage one: HIST_VALUE_BLOCKS x 256 threads walk the map's 16-byte units with the grid's stride (a multiple of C / 4: a thread
// keeps its channels); the lanes by a fixed tree, the four waves in wave order
__global__ __launch_bounds__(256) void hist_value_kernel(HistTerm t, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4n = t.C >> 2;
    const size_t total = t.N * c4n, stride = (size_t)HIST_VALUE_BLOCKS * 256;
    const size_t u0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    double acc = 0.0;
    if (u0 < total) {
        const int c = (int)(u0 % c4n) * 4;
        float lo[4], scale[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo[k] = t.lo_hi[2 * (c + k)];
            scale[k] = bin_scale(lo[k], t.lo_hi[2 * (c + k) + 1], t.bins);
        }
        const f32x2* e = reinterpret_cast<const f32x2*>(t.ends) + (size_t)c * t.bins;
        // (four loads of a lane in flight before the table gathers that depend on them; the order of the sum stays fixed)
        for (size_t u = u0; u < total; u += 4 * stride) {
            f32x4 vs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (u + j * stride < total) vs[j] = *reinterpret_cast<const f32x4*>(t.f + (u + j * stride) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (u + j * stride >= total) break;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (scale[k] == 0.f) continue;
                    const double d = (double)vs[j][k] - (double)remap(vs[j][k], lo[k], scale[k], t.bins, e + (size_t)k * t.bins);
                    acc += d * d;
                }
            }
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) sh[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// stage two: a thread adds its run of partials in order, the threads by a fixed tree -> (float)(sum / (C N))
__global__ __launch_bounds__(256) void hist_value_finish_kernel(const double* __restrict__ partial, double denom, float* __restrict__ out) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    constexpr int per = HIST_VALUE_BLOCKS / 256;
    double s = 0.0;
    for (int k = 0; k < per; ++k) s += partial[tid * per + k];
    sh[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    if (tid == 0) *out = (float)(sh[0] / denom);
}

__global__ __launch_bounds__(256) void hist_grad_kernel(HistTerm t, float coef, float* __restrict__ out, int accumulate) {
    const int c4n = t.C >> 2;
    const size_t total = t.N * c4n, stride = (size_t)gridDim.x * 256;
    const size_t u0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u0 >= total) return;
    // (the stride is a multiple of C / 4 or the grid covers the map in one step: a thread keeps its channels)
    const int c = (int)(u0 % c4n) * 4;
    float lo[4], scale[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = t.lo_hi[2 * (c + k)];
        scale[k] = bin_scale(lo[k], t.lo_hi[2 * (c + k) + 1], t.bins);
    }
    const f32x2* e = reinterpret_cast<const f32x2*>(t.ends) + (size_t)c * t.bins;
    for (size_t u4 = u0; u4 < total; u4 += 4 * stride) {
        f32x4 vs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (u4 + j * stride < total) vs[j] = *reinterpret_cast<const f32x4*>(t.f + (u4 + j * stride) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t u = u4 + j * stride;
            if (u >= total) break;
            const f32x4 v = vs[j];
            f32x4 g;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                g[k] = scale[k] == 0.f ? 0.f : coef * (v[k] - remap(v[k], lo[k], scale[k], t.bins, e + (size_t)k * t.bins));
            float* dst = out + u * 4;
            if (accumulate) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k] = o[k] + g[k];
            }
            *reinterpret_cast<f32x4*>(dst) = g;
        }
    }
}

bool hist_shape_ok(size_t N, int C, int bins) {
    return hist_channels_ok(C) && N >= 1 && bins >= 2 && bins <= 1024 && (double)N * C < 2147483648.0;
}

}  // namespace

bool hist_channels_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

// once per device, before the first launch there (the counts kernel takes more than 64 KB of dynamic LDS above 512 bins)
hipError_t hist_init_device() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&hist_counts_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               1024 * HIST_SLAB * (int)sizeof(unsigned));
}

hipError_t launch_hist_counts(const float* f, size_t N, int C, int bins, float* lo_hi, unsigned* counts, hipStream_t stream) {
    if (!f || !lo_hi || !counts || !hist_shape_ok(N, C, bins)) return hipErrorInvalidValue;
    unsigned* keys = reinterpret_cast<unsigned*>(lo_hi);
    const unsigned cb = (unsigned)((2 * C + 255) / 256);
    hipLaunchKernelGGL(hist_range_init_kernel, dim3(cb), dim3(256), 0, stream, keys, C);
    const size_t want = (N * (size_t)(C / 4) + 255) / 256;
    hipLaunchKernelGGL(hist_range_kernel, dim3((unsigned)(want < HIST_RANGE_BLOCKS ? want : HIST_RANGE_BLOCKS)), dim3(256), 0, stream, f, N, C, keys);
    hipLaunchKernelGGL(hist_range_decode_kernel, dim3(cb), dim3(256), 0, stream, keys, C);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_zero(counts, (size_t)C * bins, stream);
    if (e != hipSuccess) return e;
    const int slabs = C / HIST_SLAB;
    size_t groups = (N + HIST_COUNT_THREADS - 1) / HIST_COUNT_THREADS;
    const size_t cap = (size_t)(HIST_COUNT_GROUPS / slabs);
    if (groups > cap) groups = cap;
    const size_t share = (N + groups - 1) / groups;
    hipLaunchKernelGGL(hist_counts_kernel, dim3((unsigned)groups, (unsigned)slabs), dim3(HIST_COUNT_THREADS), (size_t)bins * HIST_SLAB * sizeof(unsigned), stream, f, N,
                       C, bins, share, (const float*)lo_hi, counts);
    return hipGetLastError();
}

hipError_t launch_hist_tables(const unsigned* counts, size_t N, const float* s_lo_hi, const unsigned* s_counts, size_t Ns, int C, int bins,
                              float* ends, hipStream_t stream) {
    if (!counts || !s_lo_hi || !s_counts || !ends || !hist_shape_ok(N, C, bins) || !hist_shape_ok(Ns, C, bins)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hist_tables_kernel, dim3((unsigned)C), dim3(256), 0, stream, counts, (unsigned long long)N, s_lo_hi, s_counts,
                       (unsigned long long)Ns, bins, ends);
    return hipGetLastError();
}

static bool hist_term_ok(const HistTerm& t) { return t.f && t.lo_hi && t.ends && hist_shape_ok(t.N, t.C, t.bins); }

hipError_t launch_hist_value_partials(const HistTerm& t, double* partial, hipStream_t stream) {
    if (!hist_term_ok(t) || !partial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hist_value_kernel, dim3(HIST_VALUE_BLOCKS), dim3(256), 0, stream, t, partial);
    return hipGetLastError();
}

hipError_t launch_hist_value(const double* partial, double denom, float* out, hipStream_t stream) {
    if (!partial || !out || !(denom > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hist_value_finish_kernel, dim3(1), dim3(256), 0, stream, partial, denom, out);
    return hipGetLastError();
}

hipError_t launch_hist_grad(const HistTerm& t, float coef, float* out, int accumulate, hipStream_t stream) {
    if (!hist_term_ok(t) || !out) return hipErrorInvalidValue;
    const size_t want = (t.N * (size_t)(t.C / 4) + 255) / 256;
    hipLaunchKernelGGL(hist_grad_kernel, dim3((unsigned)(want < HIST_GRAD_BLOCKS ? want : HIST_GRAD_BLOCKS)), dim3(256), 0, stream, t, coef, out,
                       accumulate);
    return hipGetLastError();
}

}  // namespace nst
