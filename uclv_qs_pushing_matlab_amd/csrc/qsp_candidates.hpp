// qsp_candidates.hpp — the thread mapping of the kernels that run one thread per (lane, candidate):
// the rollout costs (qsp_rollout.hip) and the open-loop simulation (qsp_openloop.hip).
//
// A lane's candidates are adjacent threads.  With ONE_LANE_M candidates per lane or more a workgroup
// serves one lane and stages the lane's shape in LDS (stage_shape) at the head of its dynamic LDS;
// with fewer, a workgroup serves floor(threads / M) lanes and reads the shapes through the vector
// cache.  How a lane's candidates beyond one workgroup are served is the kernel's own choice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qsp_kernels.h"

namespace qsp {

constexpr int ONE_LANE_M = 64;    // candidates per lane from which a workgroup serves one lane
constexpr int SHAPE_D = (int)(sizeof(ShapeDev) / sizeof(double));
// ... and what follows the shape in LDS (open loop: the store tile) stays 16-byte aligned
static_assert(sizeof(ShapeDev) % 16 == 0, "ShapeDev is staged as doubles");

// the workgroup's lane's shape into lds[0 .. SHAPE_D); the caller synchronises before reading it
__device__ __forceinline__ void stage_shape(const ShapeDev& shape, double* lds) {
    const double* sh = reinterpret_cast<const double*>(&shape);
    for (int q = threadIdx.x; q < SHAPE_D; q += blockDim.x) lds[q] = sh[q];
}

// threads of a workgroup when n items are split evenly over workgroups (or passes) of at most cap: whole waves
inline int wg_threads(long long n, int cap) {
    const long long passes = (n + cap - 1) / cap;
    const long long per = (n + passes - 1) / passes;
    return (int)((per + 63) / 64 * 64);
}

}  // namespace qsp
