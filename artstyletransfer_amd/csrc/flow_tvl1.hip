// flow_tvl1.hip - TV-L1 optical flow in its dual form (Zach, Pock & Bischof 2007; Sanchez, Meinhardt-Llopis & Facciolo, IPOL
// 2013) on the pyramid, the warps and the linearisation of flow.hip (include/nst_hip.h, nst_flow_tvl1_estimate, has the
// normative definitions and the order of operations).  What is new here is the iteration and its driver:
//   flow_tvl1_kernel        one iteration - the thresholding step, u' = v + theta div p, and the dual update of the four planes
//                           p11, p12 (of u) and p21, p22 (of v) - in ONE launch: the hot loop, `iterations` launches per warp
// The dual update of a pixel reads u' at its right and lower neighbours.  The kernel forms those again from the inputs (the
// same operations, so the same bits) rather than reading them from a plane a launch before wrote: an iteration is one launch
// instead of two and moves 15 planes (u, v, Ix, Iy, rho, four duals in; u', v', four duals out) instead of 21, at the price of
// a second copy of the flow and of the duals to alternate with.  Nothing is reduced and nothing is added atomically: every run
// gives the same bits.
// A row is covered as flow_sweep_kernel covers it: groups of four pixels that start where the output row reaches a 16-byte
// boundary; a group loads and stores 16 bytes per lane where all fifteen planes lie on a boundary there (the rows above and
// below too when w is a multiple of 4) and single floats elsewhere.  The planes of a flow and of the duals are h w floats
// apart: with h w % 4 != 0 no group has them all on a boundary and the whole iteration takes single floats.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "nst_flow.h"
#include "nst_kernels.h"

namespace nst {

namespace {

struct TvPoint { float u, v; };

// the pixels x0 ... x0 + 3 of one row, columns clamped to the row.  wide: x0 + 3 < w and row + x0 lies on a 16-byte boundary
__device__ __forceinline__ void tv_four(const float* __restrict__ row, int x0, int w, bool wide, float o[4]) {
    if (wide) {
        const float4 q = *reinterpret_cast<const float4*>(row + x0);
        o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = row[min(x0 + k, w - 1)];
    }
}
// column c of one row, clamped to the row (what lies outside is never used unmasked)
__device__ __forceinline__ float tv_at(const float* __restrict__ row, int c, int w) { return row[min(max(c, 0), w - 1)]; }

template <bool WIDE>
__device__ __forceinline__ void tv_store(float* __restrict__ row, int x0, int n, const float o[4]) {
    if (WIDE) {
        *reinterpret_cast<float4*>(row + x0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) row[x0 + k] = o[k];
    }
}

// u', v' of one pixel.  p11, p12, p21, p22: the duals there; p11w, p21w: at the pixel to the left, p12n, p22n: at the pixel
// above - each as the definitions read it (0 outside the image, and 0 in the last column / the last row of its plane).
__device__ __forceinline__ TvPoint tv_primal(float u, float v, float ix, float iy, float rho, float p11, float p11w, float p12,
                                             float p12n, float p21, float p21w, float p22, float p22n, float lt, float theta) {
#pragma clang fp contract(off)
    const float g2 = ix * ix + iy * iy;
    const float r = (rho + ix * u) + iy * v;
    const float b = lt * g2;
    const float inner = g2 >= 1e-10f ? (-r) / g2 : 0.f;
    const float k = r < -b ? lt : (r > b ? -lt : inner);
    const float v1 = u + k * ix, v2 = v + k * iy;
    TvPoint o;
    o.u = v1 + theta * ((p11 - p11w) + (p12 - p12n));
    o.v = v2 + theta * ((p21 - p21w) + (p22 - p22n));
    return o;
}
// the two duals of one flow plane at one pixel from its forward differences (gx, gy) there
__device__ __forceinline__ void tv_dual(float p1, float p2, float gx, float gy, float taut, float& q1, float& q2) {
#pragma clang fp contract(off)
    const float n1 = 1.f + taut * sqrtf(gx * gx + gy * gy);
    q1 = (p1 + taut * gx) / n1;
    q2 = (p2 + taut * gy) / n1;
}

// The pixels x0 ... x0 + n - 1 of row y, n <= 4.  f: the flow (u, v), p: the duals (p11, p12, p21, p22), planes hw floats
// apart; fo, po: the new ones.  WIDE: n = 4 and all fifteen planes lie on a 16-byte boundary at (y, x0); ROWS: the rows above
// and below lie on one there too (w is a multiple of 4) - a template parameter, because the compiler turns a run-time choice
// between 16 bytes and four clamped floats into the floats.
template <bool WIDE, bool ROWS>
__device__ __forceinline__ void tv_group(const float* __restrict__ f, const float* __restrict__ p, const float* __restrict__ Ix,
                                         const float* __restrict__ Iy, const float* __restrict__ rho, int h, int w, size_t hw,
                                         float lt, float theta, float taut, float* __restrict__ fo, float* __restrict__ po, int y,
                                         int x0, int n) {
#pragma clang fp contract(off)
    const size_t off = (size_t)y * w, up = (size_t)max(y - 1, 0) * w, dn = (size_t)min(y + 1, h - 1) * w;
    constexpr bool rows = WIDE && ROWS;
    // row y, columns x0 ... x0 + 4 (k = 0 ... 4): u' is needed one pixel past the group
    float U[5], V[5], GX[5], GY[5], R[5];
    const float* const centre[5] = {f, f + hw, Ix, Iy, rho};
    float* const into[5] = {U, V, GX, GY, R};
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        tv_four(centre[a] + off, x0, w, WIDE, into[a]);
        into[a][4] = tv_at(centre[a] + off, x0 + 4, w);
    }
    // the duals of row y: p11, p21 at columns x0 - 1 ... x0 + 4 (index k + 1), p12, p22 at x0 ... x0 + 4 and on the row above
    float a11[6], a21[6], a12[5], a22[5], n12[5], n22[5];
    a11[0] = tv_at(p + off, x0 - 1, w);
    a21[0] = tv_at(p + 2 * hw + off, x0 - 1, w);
    tv_four(p + off, x0, w, WIDE, a11 + 1);
    tv_four(p + 2 * hw + off, x0, w, WIDE, a21 + 1);
    a11[5] = tv_at(p + off, x0 + 4, w);
    a21[5] = tv_at(p + 2 * hw + off, x0 + 4, w);
    tv_four(p + hw + off, x0, w, WIDE, a12);
    tv_four(p + 3 * hw + off, x0, w, WIDE, a22);
    a12[4] = tv_at(p + hw + off, x0 + 4, w);
    a22[4] = tv_at(p + 3 * hw + off, x0 + 4, w);
    tv_four(p + hw + up, x0, w, rows, n12);
    tv_four(p + 3 * hw + up, x0, w, rows, n22);
    n12[4] = tv_at(p + hw + up, x0 + 4, w);
    n22[4] = tv_at(p + 3 * hw + up, x0 + 4, w);
    // as the definitions read them: p11, p21 are 0 left of the image and in the last column; p12, p22 above it and in the last row
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int c = x0 - 1 + k;
        const bool in = c >= 0 && c < w - 1;
        a11[k] = in ? a11[k] : 0.f;
        a21[k] = in ? a21[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        a12[k] = y < h - 1 ? a12[k] : 0.f;
        a22[k] = y < h - 1 ? a22[k] : 0.f;
        n12[k] = y >= 1 ? n12[k] : 0.f;
        n22[k] = y >= 1 ? n22[k] : 0.f;
    }
    TvPoint here[5];
#pragma unroll
    for (int k = 0; k < 5; ++k)
        here[k] = tv_primal(U[k], V[k], GX[k], GY[k], R[k], a11[k + 1], a11[k], a12[k], n12[k], a21[k + 1], a21[k], a22[k], n22[k],
                            lt, theta);
    // row y + 1, columns x0 ... x0 + 3: u' below each pixel of the group (a clamped row, never used, on the last row)
    float U1[4], V1[4], GX1[4], GY1[4], R1[4], b11[5], b21[5], b12[4], b22[4];
    float* const into1[5] = {U1, V1, GX1, GY1, R1};
#pragma unroll
    for (int a = 0; a < 5; ++a) tv_four(centre[a] + dn, x0, w, rows, into1[a]);
    b11[0] = tv_at(p + dn, x0 - 1, w);
    b21[0] = tv_at(p + 2 * hw + dn, x0 - 1, w);
    tv_four(p + dn, x0, w, rows, b11 + 1);
    tv_four(p + 2 * hw + dn, x0, w, rows, b21 + 1);
    tv_four(p + hw + dn, x0, w, rows, b12);
    tv_four(p + 3 * hw + dn, x0, w, rows, b22);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int c = x0 - 1 + k;
        const bool in = c >= 0 && c < w - 1;
        b11[k] = in ? b11[k] : 0.f;
        b21[k] = in ? b21[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b12[k] = y + 1 < h - 1 ? b12[k] : 0.f;
        b22[k] = y + 1 < h - 1 ? b22[k] : 0.f;
    }
    float ou[4], ov[4], q11[4], q12[4], q21[4], q22[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const TvPoint below = tv_primal(U1[k], V1[k], GX1[k], GY1[k], R1[k], b11[k + 1], b11[k], b12[k], a12[k], b21[k + 1], b21[k],
                                        b22[k], a22[k], lt, theta);
        const bool right = x0 + k + 1 < w, down = y + 1 < h;      // the forward differences are 0 in the last column / row
        const float ux = right ? here[k + 1].u - here[k].u : 0.f, uy = down ? below.u - here[k].u : 0.f;
        const float vx = right ? here[k + 1].v - here[k].v : 0.f, vy = down ? below.v - here[k].v : 0.f;
        ou[k] = here[k].u;
        ov[k] = here[k].v;
        tv_dual(a11[k + 1], a12[k], ux, uy, taut, q11[k], q12[k]);
        tv_dual(a21[k + 1], a22[k], vx, vy, taut, q21[k], q22[k]);
    }
    tv_store<WIDE>(fo + off, x0, n, ou);
    tv_store<WIDE>(fo + hw + off, x0, n, ov);
    tv_store<WIDE>(po + off, x0, n, q11);
    tv_store<WIDE>(po + hw + off, x0, n, q12);
    tv_store<WIDE>(po + 2 * hw + off, x0, n, q21);
    tv_store<WIDE>(po + 3 * hw + off, x0, n, q22);
}

// The groups without 16-byte accesses, out of line (flow_sweep_kernel's reason: inlined beside the wide path the compiler
// merges the tails of the two).
__device__ __noinline__ void tv_group_narrow(const float* __restrict__ f, const float* __restrict__ p, const float* __restrict__ Ix,
                                             const float* __restrict__ Iy, const float* __restrict__ rho, int h, int w, size_t hw,
                                             float lt, float theta, float taut, float* __restrict__ fo, float* __restrict__ po,
                                             int y, int x0, int n) {
    tv_group<false, false>(f, p, Ix, Iy, rho, h, w, hw, lt, theta, taut, fo, po, y, x0, n);
}

}  // namespace

__global__ __launch_bounds__(FLOW_THREADS) void flow_tvl1_kernel(const float* __restrict__ f, const float* __restrict__ p,
                                                                 const float* __restrict__ Ix, const float* __restrict__ Iy,
                                                                 const float* __restrict__ rho, int h, int w, float lt, float theta,
                                                                 float taut, float* __restrict__ fo, float* __restrict__ po) {
    const size_t hw = (size_t)h * w;
    const size_t groups = (size_t)(w + 3) / 4 + 1;      // of one row: the pixels before the first boundary, then fours
    const size_t items = (size_t)h * groups;
    const bool planes = (hw & 3) == 0;                  // the planes of a flow and of the duals lie on a boundary together
    for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(it / groups), g = (int)(it - (size_t)y * groups);
        const size_t off = (size_t)y * w;
        // pixels of the row before the output row's first 16-byte boundary
        const int head = min((int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(fo + off) & 15u)) & 15u) >> 2), w);
        const int x0 = g == 0 ? 0 : head + 4 * (g - 1);
        const int x1 = g == 0 ? head : min(x0 + 4, w);
        const int n = x1 - x0;
        if (n <= 0) continue;
        const size_t c = off + x0;
        const bool wide = n == 4 && planes && aligned16(fo + c) && aligned16(po + c) && aligned16(f + c) && aligned16(p + c) &&
                          aligned16(Ix + c) && aligned16(Iy + c) && aligned16(rho + c);
        if (wide && (w & 3) == 0) tv_group<true, true>(f, p, Ix, Iy, rho, h, w, hw, lt, theta, taut, fo, po, y, x0, n);
        else if (wide) tv_group<true, false>(f, p, Ix, Iy, rho, h, w, hw, lt, theta, taut, fo, po, y, x0, n);
        else tv_group_narrow(f, p, Ix, Iy, rho, h, w, hw, lt, theta, taut, fo, po, y, x0, n);
    }
}

// n iterations from (fin, pin); iteration k writes (fout, pout) when n - k is even and (ftmp, ptmp) otherwise, so the last one
// writes (fout, pout).  The first must not write what it reads; a later one may overwrite the inputs (the driver's two copies).
hipError_t launch_flow_tvl1_iterations(const float* Ix, const float* Iy, const float* rho, const float* fin, const float* pin, int h,
                                       int w, float lt, float theta, float taut, int n, float* fout, float* pout, float* ftmp,
                                       float* ptmp, hipStream_t stream) {
    if (h < 1 || w < 1 || n < 1 || !Ix || !Iy || !rho || !fin || !pin || !fout || !pout || (n > 1 && (!ftmp || !ptmp)) ||
        fout == ftmp || pout == ptmp || fin == (((n - 1) & 1) ? ftmp : fout) || pin == (((n - 1) & 1) ? ptmp : pout))
        return hipErrorInvalidValue;
    const size_t items = (size_t)h * ((size_t)(w + 3) / 4 + 1);
    const float* fs = fin;
    const float* ps = pin;
    for (int k = 1; k <= n; ++k) {
        float* fd = ((n - k) & 1) ? ftmp : fout;
        float* pd = ((n - k) & 1) ? ptmp : pout;
        hipLaunchKernelGGL(flow_tvl1_kernel, dim3(flow_blocks(items)), dim3(FLOW_THREADS), 0, stream, fs, ps, Ix, Iy, rho, h, w, lt,
                           theta, taut, fd, pd);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        fs = fd;
        ps = pd;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------ the driver
int flow_tvl1_layout(int h, int w, int scales, FlowTvl1Layout* out) {
    if (!out || flow_layout(h, w, scales, &out->hs) != 0) return -1;
    const size_t duals = round4(4 * (size_t)h * w);
    out->dual[0] = out->hs.floats;
    out->dual[1] = out->dual[0] + duals;
    out->floats = out->dual[1] + duals;
    return 0;
}

hipError_t launch_flow_tvl1_estimate(const float* from, const float* to, const FlowTvl1Layout& t, float lt, float theta, float taut,
                                     int warps, int iterations, float* flow, float* ws, hipStream_t stream) {
    const FlowLayout& l = t.hs;
    if (!from || !to || !flow || !ws || warps < 1 || iterations < 1 || l.scales < 1) return hipErrorInvalidValue;
    const int S = l.scales;
    const float* A[NST_FLOW_MAX_SCALES];
    const float* B[NST_FLOW_MAX_SCALES];
    A[0] = from; B[0] = to;
    for (int s = 1; s < S; ++s) {
        hipError_t e = launch_flow_reduce(A[s - 1], l.h[s - 1], l.w[s - 1], ws + l.from[s], stream);
        if (e == hipSuccess) e = launch_flow_reduce(B[s - 1], l.h[s - 1], l.w[s - 1], ws + l.to[s], stream);
        if (e != hipSuccess) return e;
        A[s] = ws + l.from[s]; B[s] = ws + l.to[s];
    }
    // The state of a scale - its flow and its duals - lies in one of two copies: (the caller's `flow`, dual[0]) and the
    // workspace's (other, dual[1]).  An iteration leaves it in the other copy, and so does a prolongation (of the flow: the
    // duals of a scale start at zero); the coarsest scale starts in the copy from which the finest ends in `flow`.
    float* fbuf[2] = {flow, ws + l.other};
    float* pbuf[2] = {ws + t.dual[0], ws + t.dual[1]};
    const int flip = (iterations & 1) & (warps & 1);      // copies changed by the warps of one scale, mod 2
    int cur = (S * flip + (S - 1)) & 1;
    hipError_t e = hipMemsetAsync(fbuf[cur], 0, 2 * (size_t)l.h[S - 1] * l.w[S - 1] * sizeof(float), stream);
    if (e != hipSuccess) return e;
    for (int s = S - 1; s >= 0; --s) {
        const int h = l.h[s], w = l.w[s];
        const size_t hw = (size_t)h * w;
        e = hipMemsetAsync(pbuf[cur], 0, 4 * hw * sizeof(float), stream);
        if (e != hipSuccess) return e;
        for (int k = 0; k < warps; ++k) {
            e = launch_flow_linearize(A[s], B[s], fbuf[cur], fbuf[cur] + hw, h, w, ws + l.ix, ws + l.iy, ws + l.rho, stream);
            if (e != hipSuccess) return e;
            // an even count ends where it began (the first iteration then writes the other copy), an odd one in the other copy
            const int out = (iterations & 1) ? cur ^ 1 : cur, tmp = out ^ 1;
            e = launch_flow_tvl1_iterations(ws + l.ix, ws + l.iy, ws + l.rho, fbuf[cur], pbuf[cur], h, w, lt, theta, taut, iterations,
                                            fbuf[out], pbuf[out], iterations == 1 ? nullptr : fbuf[tmp],
                                            iterations == 1 ? nullptr : pbuf[tmp], stream);
            if (e != hipSuccess) return e;
            cur = out;
        }
        if (s > 0) {
            e = launch_flow_prolong(fbuf[cur], l.h[s - 1], l.w[s - 1], fbuf[cur ^ 1], stream);
            if (e != hipSuccess) return e;
            cur ^= 1;
        }
    }
    return cur == 0 ? hipSuccess : hipErrorUnknown;
}

}  // namespace nst
