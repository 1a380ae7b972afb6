// nst_sample.h - the bilinear sample of the warp (include/nst_hip.h, nst_warp_bilinear): the ONE position rule of the project.
// Device code only; temporal.hip (warp, flow weights) and flow.hip (the linearisation of the flow estimator) include it.
#pragma once
#include <hip/hip_runtime.h>

namespace nst {

// The sample position of one axis: pixel index x plus displacement d, as integer part and fraction of d ALONE - x + d is
// never formed in fp32, so the fraction is as accurate at every image size.  i0, i1: the two taps clamped to [0, n - 1]; t: the
// weight of the second; inside: both taps lie in the image before clamping.  d must be finite.
struct AxisTap { int i0, i1; float t; bool inside; };
__device__ __forceinline__ AxisTap axis_tap(int x, float d, int n) {
    const float f = floorf(d);
    AxisTap r;
    r.t = d - f;                                  // in [0, 1]; exact for d >= 0, one rounding of at most 2^-25 for d < 0 - whatever x is
    // a displacement beyond the image on either side: every tap clamps to the border whatever the integer part is
    const float lim = (float)n + 1.f;
    const int k = (int)fminf(fmaxf(f, -lim), lim);
    const int a = x + k, b = a + 1;
    r.inside = a >= 0 && b <= n - 1;
    r.i0 = min(max(a, 0), n - 1);
    r.i1 = min(max(b, 0), n - 1);
    return r;
}
// (v00 (1 - tx) + v01 tx)(1 - ty) + (v10 (1 - tx) + v11 tx) ty, every operation rounded once; v<row><column> of the taps
__device__ __forceinline__ float bilinear_mix(float v00, float v01, float v10, float v11, float tx, float ty) {
#pragma clang fp contract(off)
    const float ux = 1.f - tx, uy = 1.f - ty;
    const float top = v00 * ux + v01 * tx;
    const float bot = v10 * ux + v11 * tx;
    return top * uy + bot * ty;
}
__device__ __forceinline__ float bilinear(const float* __restrict__ plane, int w, const AxisTap& ax, const AxisTap& ay) {
    const float* r0 = plane + (size_t)ay.i0 * w;
    const float* r1 = plane + (size_t)ay.i1 * w;
    return bilinear_mix(r0[ax.i0], r0[ax.i1], r1[ax.i0], r1[ax.i1], ax.t, ay.t);
}

}  // namespace nst
