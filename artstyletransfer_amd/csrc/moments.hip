// moments.hip - the moment loss (include/nst_hip.h has the definition): the channel means and deviations of a style map
// matched to the style's - the "BN statistics matching" of Li et al. 2017, the style loss of Huang & Belongie 2017.  Here:
// per-channel sums and sums of squares in double through two ordered stages (the stages of gram_shift.hip's channel sums,
// with a second accumulator), and the fold of the term into the Gram backward.  The backward of the term at a map is a
// per-channel affine function of the map, dF[p][c] = b_c F[p][c] + (a_c - b_c mu_c), and the launches that carry F S + r
// take it as S += diag(b), r += a - b o mu: no convolution kernel knows of the term.
//
// Everything is summed in a fixed order (no float atomics): a closure with the term is as reproducible as one without.
#include <hip/hip_runtime.h>

#include "nst_kernels.h"

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- stage one: per-channel sums and sums of squares of a pixel range ----------------------------------------------------
// A block owns pix_per_blk consecutive pixels of one item.  C / 4 lanes cover a pixel (16 bytes each), 256 / (C / 4) pixels
// are in flight per step, four steps per lane; each lane keeps four double sums and four double sums of squares (the square
// of an fp32 value is exact in double), and the pixel groups are then added in group order through LDS.
// part[block][2][C] doubles.
__global__ __launch_bounds__(256) void moment_sums_kernel(MomentBatch b) {
    __shared__ double sh[2][256 * 4];
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i].blk_end) ++i;
    const MomentItem& it = b.it[i];
    const int bid = (int)blockIdx.x - (i ? b.it[i - 1].blk_end : 0);
    const int C = it.C, tpp = C >> 2;
    const int groups = 256 / tpp;                  // (C <= 1024: at least one)
    const int g = (int)threadIdx.x / tpp, q = (int)threadIdx.x - g * tpp;
    const size_t p0 = (size_t)bid * it.pix_per_blk;
    size_t p1 = p0 + it.pix_per_blk;
    if (p1 > it.N) p1 = it.N;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, acq[4] = {0.0, 0.0, 0.0, 0.0};
    if (g < groups) {
        size_t p = p0 + g;
        const size_t st = (size_t)groups;
        for (; p + 3 * st < p1; p += 4 * st) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(it.f + (p + u * st) * C + q * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double x = (double)v[u][k];
                    acc[k] += x;
                    acq[k] += x * x;
                }
        }
        for (; p < p1; p += st) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(it.f + p * C + q * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double x = (double)v[k];
                acc[k] += x;
                acq[k] += x * x;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sh[0][g * C + q * 4 + k] = acc[k];
            sh[1][g * C + q * 4 + k] = acq[k];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * C; c += 256) {
        const int w = c >= C ? 1 : 0, cc = c - w * C;
        double t = sh[w][cc];
        for (int k = 1; k < groups; ++k) t += sh[w][k * C + cc];
        it.part[(size_t)bid * 2 * C + c] = t;
    }
}

// ---- stage two: mu and sigma, one block per item ------------------------------------------------------------------------
// Channel c's block sums are added in four consecutive slices (each in block order), the slices in slice order, as the
// channel sums of the centred Gram are.  mu = sum / N, var = sumsq / N - mu^2 clamped at 0, sigma = sqrt(var + epsilon), in
// double: stat[0 .. C) = mu, stat[C .. 2C) = sigma.  mean_out / std_out (nullable): the same rounded to fp32 and scaled by
// alpha - written, or (accumulate) added to what is there, product and sum each rounded: the blend of several styles.
__global__ __launch_bounds__(256) void moment_finish_kernel(MomentBatch b) {
#pragma clang fp contract(off)
    __shared__ double shs[2][4][64];
    const MomentItem& it = b.it[blockIdx.x];
    const int C = it.C, tid = threadIdx.x;
    const int per = (it.nblk + 3) / 4;
    for (int c0 = 0; c0 < C; c0 += 64) {
        // 64 channels x 4 slices per pass
        const int c = c0 + (tid & 63), sl = tid >> 6;
        double t = 0.0, tq = 0.0;
        const int k1 = (sl + 1) * per < it.nblk ? (sl + 1) * per : it.nblk;
        for (int k = sl * per; k < k1; ++k) {
            t += it.part[(size_t)k * 2 * C + c];
            tq += it.part[(size_t)k * 2 * C + C + c];
        }
        shs[0][sl][tid & 63] = t;
        shs[1][sl][tid & 63] = tq;
        __syncthreads();
        if (tid < 64) {
            const double sum = ((shs[0][0][tid] + shs[0][1][tid]) + shs[0][2][tid]) + shs[0][3][tid];
            const double sq = ((shs[1][0][tid] + shs[1][1][tid]) + shs[1][2][tid]) + shs[1][3][tid];
            const double mu = sum / (double)it.N;
            double var = sq / (double)it.N - mu * mu;
            if (!(var > 0.0)) var = 0.0;
            const double sigma = sqrt(var + it.epsilon);
            it.stat[c0 + tid] = mu;
            it.stat[C + c0 + tid] = sigma;
            if (it.mean_out) {
                const float m = it.alpha * (float)mu;
                it.mean_out[c0 + tid] = it.accumulate ? it.mean_out[c0 + tid] + m : m;
            }
            if (it.std_out) {
                const float sg = it.alpha * (float)sigma;
                it.std_out[c0 + tid] = it.accumulate ? it.std_out[c0 + tid] + sg : sg;
            }
        }
        __syncthreads();
    }
}

int moment_blocks(int C, size_t N) {
    // at least 64 pixels per block, and no more partial sums than the scratch of an item holds
    size_t nb = (N + 63) / 64;
    const size_t cap = (size_t)MOM_PART_DOUBLES / (size_t)(2 * C);
    if (nb > cap) nb = cap;
    return (int)(nb < 1 ? 1 : nb);
}

hipError_t launch_moment_stats(const MomentBatch& b0, hipStream_t stream) {
    if (b0.n < 1 || b0.n > NST_GRAM_BATCH_MAX) return hipErrorInvalidValue;
    MomentBatch b = b0;
    for (int i = 0; i < b.n; ++i) {
        MomentItem& it = b.it[i];
        if (!it.f || !it.part || !it.stat || it.N < 1 || !(it.epsilon > 0.0)) return hipErrorInvalidValue;
        if (!(it.C == 64 || it.C % 128 == 0) || it.C > 1024) return hipErrorInvalidValue;
        const int want = moment_blocks(it.C, it.N);
        it.pix_per_blk = (it.N + want - 1) / want;
        it.nblk = (int)((it.N + it.pix_per_blk - 1) / it.pix_per_blk);
        it.blk_end = (i ? b.it[i - 1].blk_end : 0) + it.nblk;
    }
    hipLaunchKernelGGL(moment_sums_kernel, dim3(b.it[b.n - 1].blk_end), dim3(256), 0, stream, b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(moment_finish_kernel, dim3(b.n), dim3(256), 0, stream, b);
    return hipGetLastError();
}

// ---- the fold: the term's values and its gradient into S and the row bias, one block per item ---------------------------
// Per channel, in double: dm = mu - mu^t, ds = sigma - sigma^t, a = wm 2 dm / (C N), b = ws 2 ds / (C N sigma).  The
// diagonal: S[c][c] <- fl(S[c][c] + (float)b); what the launch then multiplies F by is b' = that sum minus the old entry
// (exact in double), and the bias is made with b': r[c] = r0[c] + (float)(a - b' mu), so that F S + r is a + b' (F - mu)
// whatever the rounding of the sum.  The S record is raised by atomicMax of the bit pattern (order-independent).  The two
// values: sum_c dm^2 / C and sum_c ds^2 / C, by a fixed tree.
__global__ __launch_bounds__(256) void moment_fold_kernel(MomentFoldBatch b) {
#pragma clang fp contract(off)
    __shared__ double shd[2][256];
    __shared__ float shm[256];
    const MomentFoldItem& it = b.it[blockIdx.x];
    const int C = it.C, tid = threadIdx.x;
    const double cn = (double)C * (double)it.N;
    double sm = 0.0, ss = 0.0;
    float amax = 0.f;
    for (int c = tid; c < C; c += 256) {
        const double mu = it.stat[c], sigma = it.stat[C + c];
        const double dm = mu - (double)it.mean_t[c], ds = sigma - (double)it.std_t[c];
        sm += dm * dm;
        ss += ds * ds;
        const double a = (double)it.wm * 2.0 * dm / cn;
        const float bf = (float)((double)it.ws * 2.0 * ds / (cn * sigma));
        const size_t e = (size_t)c * C + c;
        const float s_old = it.S[e];
        const float s_new = s_old + bf;
        it.S[e] = s_new;
        if (it.S_bf) {
            // the same value cut into three bf16 pieces in conv_bf3's weight layout (as the Gram finish pass writes it)
            const unsigned uh = __float_as_uint(s_new) & 0xFFFF0000u;
            const float r1 = s_new - __uint_as_float(uh);
            const unsigned um = __float_as_uint(r1) & 0xFFFF0000u;
            const float r2 = r1 - __uint_as_float(um);
            const size_t base = (((size_t)c * (C / 32) + c / 32) * 3) * 32 + (c & 31);
            it.S_bf[base] = (unsigned short)(uh >> 16);
            it.S_bf[base + 32] = (unsigned short)(um >> 16);
            it.S_bf[base + 64] = (unsigned short)(__float_as_uint(r2) >> 16);
        }
        amax = fmaxf(amax, fabsf(s_new));
        const double beff = (double)s_new - (double)s_old;
        const float r = (float)(a - beff * mu);
        it.bias[c] = it.bias0 ? it.bias0[c] + r : r;
    }
    shd[0][tid] = sm; shd[1][tid] = ss; shm[tid] = amax;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            shd[0][tid] += shd[0][tid + off];
            shd[1][tid] += shd[1][tid + off];
            shm[tid] = fmaxf(shm[tid], shm[tid + off]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        it.loss[0] = shd[0][0] / (double)C;
        it.loss[1] = shd[1][0] / (double)C;
        if (it.S_amax) atomicMax(it.S_amax, __float_as_uint(shm[0]));      // (non-negative floats order as their bits)
    }
}

hipError_t launch_moment_fold(const MomentFoldBatch& b, hipStream_t stream) {
    if (b.n < 1 || b.n > NST_GRAM_BATCH_MAX) return hipErrorInvalidValue;
    for (int i = 0; i < b.n; ++i) {
        const MomentFoldItem& it = b.it[i];
        if (!it.stat || !it.mean_t || !it.std_t || !it.S || !it.bias || !it.loss || it.N < 1 || it.C < 32 || it.C % 32 != 0)
            return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(moment_fold_kernel, dim3(b.n), dim3(256), 0, stream, b);
    return hipGetLastError();
}

}  // namespace nst
