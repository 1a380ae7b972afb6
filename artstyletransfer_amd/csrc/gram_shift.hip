// gram_shift.hip - activation-shifted and mean-centred Gram matrices (include/nst_hip.h has the definition):
// G_o = sum_p (F_p + o)(F_p + o)^T / (C N) with a per-channel offset o - a constant s (Novak & Nikulin 2016, s = -1) or
// minus the map's own channel means (the covariance: Li et al. 2017).  Here: the offsets with the record that bounds the
// shifted operand, and the row bias r = o S of the backward, dF_p = (F_p + o) S = F_p S + r.  The partial products are the
// SHIFT form of gram.hip's fp16-piece kernel; the bias rides in the epilogue of the launches that carry F S (conv_h2.hip).
//
// Everything is summed in a fixed order (no float atomics): a closure with the option is as reproducible as one without.
#include <hip/hip_runtime.h>

#include "nst_kernels.h"

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- stage one: per-channel sums of a pixel range ----------------------------------------------------------------------
// A block owns pix_per_blk consecutive pixels of one centred item.  C / 4 lanes cover a pixel (16 bytes each, so a wave reads
// whole 256-byte segments), 256 / (C / 4) pixels are in flight per step; each lane keeps four double sums, and the pixel
// groups are then added in group order through LDS.  part[block][C] doubles.
__global__ __launch_bounds__(256) void gram_offset_sums_kernel(OffsetBatch b) {
    __shared__ double sh[256 * 4];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].blk_end) ++i;
    const OffsetItem& it = b.it[i];
    const int bid = (int)blockIdx.x - (i ? b.it[i - 1].blk_end : 0);
    const int C = it.C, tpp = C >> 2;
    const int groups = 256 / tpp;                  // (C <= 1024: at least one)
    const int g = (int)threadIdx.x / tpp, q = (int)threadIdx.x - g * tpp;
    const size_t p0 = (size_t)bid * it.pix_per_blk;
    size_t p1 = p0 + it.pix_per_blk;
    if (p1 > it.N) p1 = it.N;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (g < groups) {
        // four pixels of the lane in flight per step (one would leave the pass latency-bound); added in ascending pixel order
        size_t p = p0 + g;
        const size_t st = (size_t)groups;
        for (; p + 3 * st < p1; p += 4 * st) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(it.f + (p + u * st) * C + q * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] += (double)v[u][k];
        }
        for (; p < p1; p += st) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(it.f + p * C + q * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += (double)v[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[g * C + q * 4 + k] = acc[k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double t = sh[c];
        for (int k = 1; k < groups; ++k) t += sh[k * C + c];
        it.part[(size_t)bid * C + c] = t;
    }
}

// ---- stage two: the offsets and the record of the shifted operand, one block per item -------------------------------------
// centred: channel c's block sums are added in four consecutive slices (each in block order), the slices in slice order;
// o_c = -(sum / N) rounded to fp32.  Record: absmax(F) + max_c |o_c|, rounded up - |F + o| <= |F| + |o| whatever the signs.
__global__ __launch_bounds__(256) void gram_offset_finish_kernel(OffsetBatch b) {
    __shared__ double shs[4][64];
    __shared__ float shm[256];
    const OffsetItem& it = b.it[blockIdx.x];
    const int C = it.C, tid = threadIdx.x;
    float omax = 0.f;
    if (it.center) {
        const int per = (it.nblk + 3) / 4;
        for (int c0 = 0; c0 < C; c0 += 64) {
            // 64 channels x 4 slices per pass
            const int c = c0 + (tid & 63), sl = tid >> 6;
            double t = 0.0;
            const int k1 = (sl + 1) * per < it.nblk ? (sl + 1) * per : it.nblk;
            for (int k = sl * per; k < k1; ++k) t += it.part[(size_t)k * C + c];
            shs[sl][tid & 63] = t;
            __syncthreads();
            if (tid < 64) {
                const double sum = ((shs[0][tid] + shs[1][tid]) + shs[2][tid]) + shs[3][tid];
                const float o = (float)(-(sum / (double)it.N));
                it.offset[c0 + tid] = o;
                omax = fmaxf(omax, fabsf(o));
            }
            __syncthreads();
        }
    } else {
        for (int c = tid; c < C; c += 256) it.offset[c] = it.shift;
        omax = fabsf(it.shift);
    }
    shm[tid] = omax;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) shm[tid] = fmaxf(shm[tid], shm[tid + off]);
        __syncthreads();
    }
    if (tid < NST_AMAX_SLOTS) {
        unsigned m = 0;
        for (int k = 0; k < NST_AMAX_SLOTS; ++k) m = it.amax[k] > m ? it.amax[k] : m;       // (non-negative floats order as their bits)
        // (the sum rounds to nearest: one ulp up makes it a bound again)
        const float bound = __uint_as_float(m) + shm[0];
        it.amax_out[tid] = (bound > 0.f && bound < __builtin_inff()) ? __float_as_uint(bound) + 1u : __float_as_uint(bound);
    }
}

int gram_offset_blocks(int C, size_t N) {
    // at least 64 pixels per block, and no more partial sums than the scratch of an item holds
    size_t nb = (N + 63) / 64;
    const size_t cap = (size_t)GS_PART_DOUBLES / (size_t)C;
    if (nb > cap) nb = cap;
    return (int)(nb < 1 ? 1 : nb);
}

hipError_t launch_gram_offsets(const OffsetBatch& b0, hipStream_t stream) {
    if (b0.n < 1 || b0.n > NST_GRAM_BATCH_MAX) return hipErrorInvalidValue;
    OffsetBatch b = b0;      // stage two: every item, in the caller's order
    OffsetBatch c{};         // stage one: the centred items
    for (int i = 0; i < b.n; ++i) {
        OffsetItem& it = b.it[i];
        if (!it.f || !it.amax || !it.offset || !it.amax_out || it.N < 1) return hipErrorInvalidValue;
        if (!(it.C == 64 || it.C % 128 == 0) || it.C > 1024) return hipErrorInvalidValue;
        it.nblk = 0; it.pix_per_blk = 0; it.blk_end = 0;
        if (!it.center) continue;
        if (!it.part) return hipErrorInvalidValue;
        const int want = gram_offset_blocks(it.C, it.N);
        it.pix_per_blk = (it.N + want - 1) / want;
        it.nblk = (int)((it.N + it.pix_per_blk - 1) / it.pix_per_blk);
        OffsetItem& d = c.it[c.n];
        d = it;
        d.blk_end = (c.n ? c.it[c.n - 1].blk_end : 0) + it.nblk;
        ++c.n;
    }
    if (c.n > 0) {
        hipLaunchKernelGGL(gram_offset_sums_kernel, dim3(c.it[c.n - 1].blk_end), dim3(256), 0, stream, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gram_offset_finish_kernel, dim3(b.n), dim3(256), 0, stream, b);
    return hipGetLastError();
}

// ---- the row bias r = o S ---------------------------------------------------------------------------------------------
// A block owns 64 columns of one item: four slices of k (each in ascending k, in double), added in slice order.
__global__ __launch_bounds__(256) void gram_row_bias_kernel(RowBiasBatch b) {
    __shared__ double sh[4][64];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].blk_end) ++i;
    const RowBiasItem& it = b.it[i];
    const int bid = (int)blockIdx.x - (i ? b.it[i - 1].blk_end : 0);
    const int C = it.C;
    const int col = bid * 64 + ((int)threadIdx.x & 63), sl = (int)threadIdx.x >> 6;
    const int per = C >> 2;
    double t = 0.0;
    for (int k = sl * per; k < (sl + 1) * per; ++k) t += (double)it.offset[k] * (double)it.S[(size_t)k * C + col];
    sh[sl][threadIdx.x & 63] = t;
    __syncthreads();
    if (threadIdx.x < 64) it.r[col] = (float)(((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x]);
}

hipError_t launch_gram_row_bias(const RowBiasBatch& b0, hipStream_t stream) {
    if (b0.n < 1 || b0.n > NST_GRAM_BATCH_MAX) return hipErrorInvalidValue;
    RowBiasBatch b = b0;
    for (int i = 0; i < b.n; ++i) {
        RowBiasItem& it = b.it[i];
        if (!it.offset || !it.S || !it.r || it.C < 64 || it.C % 64 != 0) return hipErrorInvalidValue;
        it.blk_end = (i ? b.it[i - 1].blk_end : 0) + it.C / 64;
    }
    hipLaunchKernelGGL(gram_row_bias_kernel, dim3(b.it[b.n - 1].blk_end), dim3(256), 0, stream, b);
    return hipGetLastError();
}

}  // namespace nst
