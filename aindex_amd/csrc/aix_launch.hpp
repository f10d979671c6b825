// aix_launch.hpp — private to the library: what the files with flat grid-stride kernels of 256 lanes share (aix_lookup.hip, aix_index.hip,
// aix_count.hip, aix_api.hip): the workgroup size, the grid sizing, the wave-uniform loop, the launch and the lanes-per-bucket dispatch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "aix_env.hpp"

namespace aix {

static constexpr int kBlock = 256;
inline unsigned grid_for(uint64_t work, unsigned per_block = kBlock) {
    // Grid-stride kernels. Up to 8192 workgroups one trip each; beyond that a quarter of the trips' worth of workgroups — a wave keeps at
    // least four trips, which is what the lookups' FilterGauge needs to adapt — up to 256 per CU: finer workgroups balance the tail better
    // than 32 per CU did (100 M lookups 2.116 against 2.16 ms, coverage 29.9 against 31.4 ms, count23 38.3 against 38.7 ms, one box).
    static const uint64_t per_cu = (uint64_t)env_int("AIX_GRID_PER_CU", 1, 1024, 256);   // A/B switch
    const uint64_t need = (work + per_block - 1) / per_block, cap = 256ull * per_cu;
    uint64_t b = std::max(std::min<uint64_t>(need, 8192), need / 4);
    if (b > cap) b = cap;
    if (b == 0) b = 1;
    return (unsigned)b;
}

// wave-uniform grid-stride loops: every lane of a wave runs the same number of trips (the probes are wave-cooperative)
#define AIX_WAVE_LOOP(i, N)                                                                                    \
    for (uint64_t i##_base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u), i = i##_base + (threadIdx.x & 63u); i##_base < (N); \
         i##_base += (uint64_t)gridDim.x * kBlock, i += (uint64_t)gridDim.x * kBlock)

// kernel(args...) on grid_for(work) workgroups of kBlock lanes, asynchronous on `stream`; returns hipGetLastError()
template <class K, class... A>
inline hipError_t launch_flat_lds(K kernel, uint64_t work, unsigned lds_bytes, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(work)), dim3(kBlock), lds_bytes, stream, args...);
    return hipGetLastError();
}
template <class K, class... A>
inline hipError_t launch_flat(K kernel, uint64_t work, hipStream_t stream, const A&... args) {
    return launch_flat_lds(kernel, work, 0, stream, args...);
}

// lanes that share one bucket read: a launch-time choice (IndexDev::bk_lpp) among the instantiated widths. f(std::integral_constant<int, L>)
template <class F>
inline auto with_lpp(uint32_t lpp, F&& f) {
    switch (lpp) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

}  // namespace aix
