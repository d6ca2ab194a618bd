// qsp_rollout.hip — batched rollout costs and the u0 cost landscape on gfx950 (FP64).
//
// The reference's own optimality probe (helper.m:356-431): a control trajectory is rolled out from x0
// with the plant model, the tracking cost against the references is summed, and debug_cost_function
// repeats that for every first move u_0 of a grid with the rest of the solver's trajectory held
// (helper.m:380-427), returning the cost surface and its grid minimiser (:430-431).
//
//   rollout_cost_kernel    one thread per (lane, candidate): cost, bound violation and end state of
//                          M caller-given control trajectories per lane (evaluate_cost_function);
//   cost_landscape_kernel  the same rollout with the candidate built in registers, u_0 = (un[i], ut[j]),
//                          u_k = U_tail[k] for k >= 1, reduced per lane to the first minimum in the
//                          linear order i n_ut + j (cost_values(:) of the meshgrid, helper.m:382,430).
//
// Both call rollout_one, so a candidate's arithmetic is the same sequence of IEEE operations in either
// kernel, at any M, B, lane index or position among the candidates: results agree bit for bit.  The
// model is the OCP's f (dynamics<false>: PusherSliderModel.m:503-603, what evalModelVariableShape
// evaluates); the stage sum is epilogue_kernel's chain (qsp_solver.hip), the Euler step euler_step
// (qsp_math.hpp: the closed loop's plant step), the RK4 step rk4_kernel's xn (qsp_sim.hip).
//
// Thread mapping (qsp_candidates.hpp): a lane's candidates are adjacent threads.  With 64 candidates or
// more a workgroup serves one lane and stages what the lane's threads share in LDS -- its shape, the
// N x 6 references, the terminal reference and (landscape) the tail of U -- and loops over candidates
// beyond its size.  With fewer, a 256-thread workgroup serves floor(256 / M) lanes and reads the
// shared data through the vector cache.  The landscape always runs one lane per workgroup: its
// reduction stays inside the workgroup (wave shifts, then one LDS slot per wave), without atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qsp_nmpc.h"
#include "qsp_math.hpp"
#include "qsp_candidates.hpp"

namespace qsp {

constexpr int RO_BLOCK = 256;        // largest workgroup

struct RollOut {
    double cost, viol, x[4];
};

// One candidate.  u_at(k, u) gives stage k's control.  cost: sum_k 0.5 tau |[x_k; u_k] - yref_k|^2_W
// + 0.5 |x_N - yref_e|^2_We; viol: the largest violation of lh <= [s_k, u_n, u_t] <= uh over
// k = 0..N-1 (0 when feasible; the s bound at stage 0 only with s0_bound, as merit_stage; a NaN
// entry compares false and leaves viol as it is -- the cost is NaN then).
template <int INTEG, class UAt>
__device__ __forceinline__ void rollout_one(const RolloutArgs& A, const ShapeDev& sh, const double* x0, const double* yref,
                                            const double* ye, UAt u_at, RollOut& o) {
    double x[4] = {x0[0], x0[1], x0[2], x0[3]};
    double cost = 0.0, viol = 0.0;
    for (int k = 0; k < A.N; ++k) {
        double u[2];
        u_at(k, u);
        const double* yr = yref + 6 * k;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { const double r = x[q] - yr[q]; s = qfma(A.W[q] * r, r, s); }
#pragma unroll
        for (int q = 0; q < 2; ++q) { const double r = u[q] - yr[4 + q]; s = qfma(A.W[4 + q] * r, r, s); }
        cost = qfma(0.5 * A.tau, s, cost);
        const double v[3] = {x[3], u[0], u[1]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j == 0 && k == 0 && !A.s0_bound) continue;
            const double vl = A.lh[j] - v[j], vh = v[j] - A.uh[j];
            if (vl > viol) viol = vl;
            if (vh > viol) viol = vh;
        }
        if (INTEG == QSP_ROLLOUT_RK4) {
            Lin L;
            rk4<false>(sh, A.Ts, x, u, L);
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = L.xn[c];
        } else {
            euler_step(sh, A.Ts, x, u[0], u[1]);
        }
    }
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const double r = x[q] - ye[q]; s = qfma(A.We[q] * r, r, s); }
    o.cost = qfma(0.5, s, cost);
    o.viol = viol;
#pragma unroll
    for (int c = 0; c < 4; ++c) o.x[c] = x[c];
}

// LDS image of one lane: [shape | yref N x 6 | yref_e 4 | tail N x 2 (landscape)]
__device__ __forceinline__ void stage_lane(const RolloutArgs& A, int lane, double* lds, bool tail) {
    stage_shape(shape_clamped(A.shapes, A.n_shapes, A.shape_id, lane), lds);
    double* yr = lds + SHAPE_D;
    const double* gy = A.yref + (size_t)lane * A.N * 6;
    for (int q = threadIdx.x; q < A.N * 6; q += blockDim.x) yr[q] = gy[q];
    double* ye = yr + A.N * 6;
    if (threadIdx.x < 4) ye[threadIdx.x] = A.yref_e[(size_t)lane * 4 + threadIdx.x];
    if (tail) {
        double* ut = ye + 4;
        const double* gu = A.U_tail + (size_t)lane * A.N * 2;
        for (int q = threadIdx.x; q < A.N * 2; q += blockDim.x) ut[q] = gu[q];
    }
    __syncthreads();
}

struct UGlobal {   // a candidate's N x 2 block; VEC: 16-byte loads (the block's base is 16-byte aligned)
    const double* u;
    bool vec;
    __device__ __forceinline__ void operator()(int k, double o[2]) const {
        if (vec) {
            const double2 v = reinterpret_cast<const double2*>(u)[k];
            o[0] = v.x;
            o[1] = v.y;
        } else {
            o[0] = u[2 * k];
            o[1] = u[2 * k + 1];
        }
    }
};

struct UGrid {     // landscape candidate: stage 0 from the grid, the rest from the lane's tail
    double u0n, u0t;
    const double* tail;
    __device__ __forceinline__ void operator()(int k, double o[2]) const {
        o[0] = k == 0 ? u0n : tail[2 * k];
        o[1] = k == 0 ? u0t : tail[2 * k + 1];
    }
};

__device__ __forceinline__ void store_rollout(const RolloutArgs& A, size_t g, const RollOut& r) {
    A.cost[g] = r.cost;
    if (A.viol) A.viol[g] = r.viol;
    if (A.x_end) {
#pragma unroll
        for (int c = 0; c < 4; ++c) A.x_end[g * 4 + c] = r.x[c];
    }
}

// ONE_LANE: blockIdx.x is the lane, the threads loop over its candidates (dynamic LDS: stage_lane's
// image).  Otherwise the workgroup serves lpb = floor(blockDim / M) lanes, thread t the candidate
// t % M of its lane t / M.
template <int INTEG, bool ONE_LANE>
__global__ void __launch_bounds__(RO_BLOCK) rollout_cost_kernel(RolloutArgs A, int lpb, int vec) {
    extern __shared__ double ro_lds[];
    if (ONE_LANE) {
        const int lane = blockIdx.x;
        stage_lane(A, lane, ro_lds, false);
        const ShapeDev& sh = *reinterpret_cast<const ShapeDev*>(ro_lds);
        const double* yr = ro_lds + SHAPE_D;
        const double* ye = yr + A.N * 6;
        const double* x0 = A.x0 + (size_t)lane * 4;
        for (int m = threadIdx.x; m < A.M; m += blockDim.x) {
            const size_t g = (size_t)lane * A.M + m;
            RollOut r;
            rollout_one<INTEG>(A, sh, x0, yr, ye, UGlobal{A.U + g * A.N * 2, vec != 0}, r);
            store_rollout(A, g, r);
        }
    } else {
        const int ll = threadIdx.x / A.M, m = threadIdx.x - ll * A.M;
        const long long lane = (long long)blockIdx.x * lpb + ll;
        if (ll >= lpb || lane >= A.B) return;
        const size_t g = (size_t)lane * A.M + m;
        RollOut r;
        rollout_one<INTEG>(A, shape_clamped(A.shapes, A.n_shapes, A.shape_id, (int)lane), A.x0 + (size_t)lane * 4,
                           A.yref + (size_t)lane * A.N * 6, A.yref_e + (size_t)lane * 4, UGlobal{A.U + g * A.N * 2, vec != 0}, r);
        store_rollout(A, g, r);
    }
}

// MATLAB's min over the surface in linear order: (c, i) with i < 0 meaning "no non-NaN entry yet".
// b replaces a when it holds an entry and a holds none, or b's is smaller, or equal at a lower index.
__device__ __forceinline__ void min_take(double& ca, int& ia, double cb, int ib) {
    const bool take = ib >= 0 && (ia < 0 || cb < ca || (cb == ca && ib < ia));
    ca = take ? cb : ca;
    ia = take ? ib : ia;
}

template <int INTEG>
__global__ void __launch_bounds__(RO_BLOCK) cost_landscape_kernel(RolloutArgs A) {
    extern __shared__ double ro_lds[];
    const int lane = blockIdx.x;
    stage_lane(A, lane, ro_lds, true);
    const ShapeDev& sh = *reinterpret_cast<const ShapeDev*>(ro_lds);
    const double* yr = ro_lds + SHAPE_D;
    const double* ye = yr + A.N * 6;
    const double* tail = ye + 4;
    double* red_c = ro_lds + SHAPE_D + A.N * 8 + 4;                 // one slot per wave
    int* red_i = reinterpret_cast<int*>(red_c + RO_BLOCK / 64);
    const double* x0 = A.x0 + (size_t)lane * 4;
    const int G = A.n_un * A.n_ut;
    double best = 0.0;
    int ibest = -1;
    for (int g = threadIdx.x; g < G; g += blockDim.x) {    // ascending g: a strict < keeps the first minimum
        const int i = g / A.n_ut, j = g - i * A.n_ut;
        RollOut r;
        rollout_one<INTEG>(A, sh, x0, yr, ye, UGrid{A.un_grid[i], A.ut_grid[j], tail}, r);
        if (A.cost) A.cost[(size_t)lane * G + g] = r.cost;
        if (r.cost == r.cost) min_take(best, ibest, r.cost, g);       // NaN never wins
    }
    // the workgroup's threads all arrive here (no early exit above): wave shifts, then the waves' slots
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double cb = __shfl_down(best, d, 64);
        const int ib = __shfl_down(ibest, d, 64);
        min_take(best, ibest, cb, ib);
    }
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { red_c[wave] = best; red_i[wave] = ibest; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) min_take(best, ibest, red_c[w], red_i[w]);
        // every entry NaN: min returns NaN at the first index (MATLAB min of an all-NaN vector)
        const int gi = ibest < 0 ? 0 : ibest;
        const int i = gi / A.n_ut, j = gi - i * A.n_ut;
        A.cost_min[lane] = ibest < 0 ? __builtin_nan("") : best;
        if (A.idx_min) A.idx_min[lane] = gi;
        A.u_min[(size_t)lane * 2] = A.un_grid[i];
        A.u_min[(size_t)lane * 2 + 1] = A.ut_grid[j];
    }
}

hipError_t launch_rollout_cost(const RolloutArgs& a, hipStream_t stream) {
    const int vec = ((uintptr_t)a.U & 15) == 0 ? 1 : 0;
    const bool rk = a.integrator == QSP_ROLLOUT_RK4;
    if (a.M >= ONE_LANE_M) {
        const size_t lds = (size_t)(SHAPE_D + a.N * 6 + 4) * sizeof(double);
        const dim3 grid((unsigned)a.B), block((unsigned)wg_threads(a.M, RO_BLOCK));
        if (rk) hipLaunchKernelGGL((rollout_cost_kernel<QSP_ROLLOUT_RK4, true>), grid, block, lds, stream, a, 1, vec);
        else hipLaunchKernelGGL((rollout_cost_kernel<QSP_ROLLOUT_EULER, true>), grid, block, lds, stream, a, 1, vec);
    } else {
        const int lpb = RO_BLOCK / a.M;
        const dim3 grid((unsigned)(((long long)a.B + lpb - 1) / lpb)), block(RO_BLOCK);
        if (rk) hipLaunchKernelGGL((rollout_cost_kernel<QSP_ROLLOUT_RK4, false>), grid, block, 0, stream, a, lpb, vec);
        else hipLaunchKernelGGL((rollout_cost_kernel<QSP_ROLLOUT_EULER, false>), grid, block, 0, stream, a, lpb, vec);
    }
    return hipGetLastError();
}

hipError_t launch_cost_landscape(const RolloutArgs& a, hipStream_t stream) {
    const size_t lds = (size_t)(SHAPE_D + a.N * 8 + 4 + RO_BLOCK / 64) * sizeof(double) + (RO_BLOCK / 64) * sizeof(int);
    const dim3 grid((unsigned)a.B), block((unsigned)wg_threads((long long)a.n_un * a.n_ut, RO_BLOCK));
    if (a.integrator == QSP_ROLLOUT_RK4)
        hipLaunchKernelGGL((cost_landscape_kernel<QSP_ROLLOUT_RK4>), grid, block, lds, stream, a);
    else
        hipLaunchKernelGGL((cost_landscape_kernel<QSP_ROLLOUT_EULER>), grid, block, lds, stream, a);
    return hipGetLastError();
}

}  // namespace qsp
