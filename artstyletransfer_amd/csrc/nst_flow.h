// nst_flow.h - what the kernels of the two flow estimators share (flow.hip: Horn-Schunck; flow_tvl1.hip: TV-L1): the launch
// geometry of their streaming kernels, the rounding of workspace planes and the 16-byte boundary test of the wide accesses.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace nst {

constexpr int FLOW_THREADS = 256;
constexpr size_t FLOW_MAX_BLOCKS = 4096;      // grids are capped and strided (launch_warp_bilinear's rule)

inline unsigned flow_blocks(size_t items) {
    const size_t want = (items + FLOW_THREADS - 1) / FLOW_THREADS;
    return (unsigned)(want < FLOW_MAX_BLOCKS ? (want < 1 ? 1 : want) : FLOW_MAX_BLOCKS);
}
inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }      // workspace planes start on 16-byte boundaries

__device__ __forceinline__ bool aligned16(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace nst
