// nst_pieces.h - what the two nearest-neighbour searches (patch_match.hip, remd.hip) share: the f16x2 operand pieces of
// conv_h2.hip (the power-of-two scale of a map's absmax record, the cut into a hi and a lo fp16 piece), the order-preserving
// bit pattern of a score, and the fixed-tree wave sum of the double reductions.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace nst {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr float LO_UP = 2048.f;   // 2^11
constexpr float LO_DOWN = 1.f / 2048.f;

// conv_h2.hip's scale: the power of two that brings the recorded absmax into [2^14, 2^15), and its inverse
__device__ __forceinline__ void tensor_scale(const unsigned* __restrict__ slots, int lane, float& s, float& inv) {
    unsigned m = slots[lane];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    int e = (int)((m >> 23) & 0xFFu);
    e = e < 32 ? 32 : (e > 250 ? 250 : e);
    s = __uint_as_float((unsigned)(268 - e) << 23);
    inv = __uint_as_float((unsigned)(e - 14) << 23);
}

// conv_h2.hip's cut: four scaled fp32 values -> their hi pieces and lo pieces (each 4 x fp16 = 8 bytes)
__device__ __forceinline__ void cut2x4(const f32x4 v, const float s, u32x2& hi, u32x2& lo) {
    const f32x2 x01 = {v[0] * s, v[1] * s}, x23 = {v[2] * s, v[3] * s};
    const f16x2 h01 = __builtin_convertvector(x01, f16x2), h23 = __builtin_convertvector(x23, f16x2);
    const f32x2 b01 = __builtin_convertvector(h01, f32x2), b23 = __builtin_convertvector(h23, f32x2);
    const f32x2 r01 = (x01 - b01) * LO_UP, r23 = (x23 - b23) * LO_UP;
    const f16x2 l01 = __builtin_convertvector(r01, f16x2), l23 = __builtin_convertvector(r23, f16x2);
    hi = u32x2{__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23)};
    lo = u32x2{__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23)};
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);      // a fixed tree: every lane ends with the same sum
    return v;
}

// the bit pattern whose unsigned order is the float order of v
__device__ __forceinline__ unsigned score_order(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

}  // namespace
}  // namespace nst
