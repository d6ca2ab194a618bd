// qsp_kkt.hip — KKT residuals of NLP iterates and QP points recomputed on gfx950 (FP64): the kernels of
// qsp_eval_kkt / qsp_eval_kkt_device and qsp_qp_residuals around the stage functions of qsp_kkt.hpp.
//
// Thread mapping, both kernels: one thread per (lane, stage), consecutive threads on consecutive stages
// of a lane, so the rows of X, U, PI, LAM (and of the QP's arrays) load from consecutive addresses.  A
// 256-thread workgroup serves floor(256 / (N + 1)) whole lanes (N + 1 <= 128: at least two), so a lane's
// maxima never leave the workgroup: each thread puts its stage's row and finite flag into LDS (column-major:
// column q of thread t at q * 256 + t, conflict-free), and after one barrier the first threads of the lane
// each take one column and fold it over the lane's N + 1 rows -- a lane may span several waves (N + 1 > 64),
// which the barrier covers.  A second barrier hands the lane's flag and maxima back: thread 0 of the lane
// writes its res / parts row, every thread its own stage_res row.  A maximum is order-free, each column is
// folded by one thread in stage order, and no atomics are used: the result does not depend on B, on the
// lane's place in the batch or in its workgroup.  The threads of a workgroup's tail (no lane) only
// take part in the barriers.
//
// A lane with a non-finite value (a stage's flag unset) gets NaN in every output, stage_res rows included;
// the other lanes of its workgroup share nothing with it but the barriers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qsp_kernels.h"
#include "qsp_kkt.hpp"

namespace qsp {

constexpr int KKT_BLOCK = 256;

// The lane's fold of NCOL columns (the last one the flag: 1.0 = a non-finite stage) over its L rows, in
// place: afterwards column q's maximum stands in the lane's first row, tab[q * KKT_BLOCK + base].
template <int NCOL>
__device__ __forceinline__ void kkt_lane_fold(double* tab, const double* row, bool live, int base, int k, int L) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NCOL; ++q) tab[q * KKT_BLOCK + t] = row[q];
    __syncthreads();
    if (live) {
        for (int q = k; q < NCOL; q += L) {
            const double* col = tab + q * KKT_BLOCK + base;
            double m = 0.0;
            for (int j = 0; j < L; ++j) m = fmax(m, col[j]);
            tab[q * KKT_BLOCK + base] = m;   // only this thread reads or writes the lane's column q here
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(KKT_BLOCK) kkt_nlp_kernel(KktNlpArgs A, int lpb) {
    __shared__ double tab[(KKT_NPARTS + 1) * KKT_BLOCK];
    const SolveParams& p = A.p;
    const int N = p.N, L = N + 1;
    const int ll = threadIdx.x / L, k = threadIdx.x - ll * L;
    const long long lane = (long long)blockIdx.x * lpb + ll;
    const bool live = ll < lpb && lane < A.B;
    double row[KKT_NPARTS + 1];
#pragma unroll
    for (int q = 0; q <= KKT_NPARTS; ++q) row[q] = 0.0;
    if (live) {
        const bool fin = kkt_nlp_stage(shape_clamped(A.pt.shapes, A.pt.n_shapes, A.pt.shape_id, (int)lane), p, k,
                                       PointRows(A.pt, N, (size_t)lane, k), row);
        row[KKT_NPARTS] = fin ? 0.0 : 1.0;
    }
    const int base = threadIdx.x - k;
    kkt_lane_fold<KKT_NPARTS + 1>(tab, row, live, base, k, L);
    if (!live) return;
    const bool bad = tab[KKT_NPARTS * KKT_BLOCK + base] != 0.0;
    const double nan = __builtin_nan("");
    if (k == 0) {
        double part[KKT_NPARTS], res[4];
#pragma unroll
        for (int q = 0; q < KKT_NPARTS; ++q) part[q] = tab[q * KKT_BLOCK + base];
        kkt_res_of_parts(part, res);
#pragma unroll
        for (int q = 0; q < 4; ++q) A.res[(size_t)lane * 4 + q] = bad ? nan : res[q];
        if (A.parts) {
#pragma unroll
            for (int q = 0; q < KKT_NPARTS; ++q) A.parts[(size_t)lane * KKT_NPARTS + q] = bad ? nan : part[q];
        }
    }
    if (A.stage_res) {
        double res[4];
        kkt_res_of_parts(row, res);
        double* out = A.stage_res + ((size_t)lane * L + k) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) out[q] = bad ? nan : res[q];
    }
}

__global__ void __launch_bounds__(KKT_BLOCK) kkt_qp_kernel(KktQpArgs A, int lpb) {
    __shared__ double tab[(KKT_QP_NRES + 1) * KKT_BLOCK];
    const int N = A.N, L = N + 1;
    const int ll = threadIdx.x / L, k = threadIdx.x - ll * L;
    const long long lane = (long long)blockIdx.x * lpb + ll;
    const bool live = ll < lpb && lane < A.nb;
    double row[KKT_QP_NRES + 1];
#pragma unroll
    for (int q = 0; q <= KKT_QP_NRES; ++q) row[q] = 0.0;
    if (live) {
        const QpLaneData d(A.A, A.B, A.b, A.H, A.g, A.lo, A.hi, N, (size_t)lane);
        const PointRows r(A.pt, N, (size_t)lane, k);
        const bool fin = kkt_qp_stage(N, A.s0_bound, k, d.Ak(k), d.Bk(k), d.bk(k), d.Hk(k), d.gk(k), d.lok(k), d.hik(k), r.x0, r.x,
                                      r.u, r.x1, r.pi, r.pip, r.lam, row);
        row[KKT_QP_NRES] = fin ? 0.0 : 1.0;
    }
    const int base = threadIdx.x - k;
    kkt_lane_fold<KKT_QP_NRES + 1>(tab, row, live, base, k, L);
    if (!live || k != 0) return;
    const bool bad = tab[KKT_QP_NRES * KKT_BLOCK + base] != 0.0;
#pragma unroll
    for (int q = 0; q < KKT_QP_NRES; ++q)
        A.res[(size_t)lane * KKT_QP_NRES + q] = bad ? __builtin_nan("") : tab[q * KKT_BLOCK + base];
}

// whole lanes per workgroup; the handle's horizons keep N + 1 <= 128 (qsp_create)
static int kkt_lanes_per_block(int N) { return KKT_BLOCK / (N + 1); }

hipError_t launch_kkt_nlp(const KktNlpArgs& a, hipStream_t stream) {
    const int lpb = kkt_lanes_per_block(a.p.N);
    if (lpb < 1 || a.B < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((long long)a.B + lpb - 1) / lpb)), block(KKT_BLOCK);
    hipLaunchKernelGGL(kkt_nlp_kernel, grid, block, 0, stream, a, lpb);
    return hipGetLastError();
}

hipError_t launch_kkt_qp(const KktQpArgs& a, hipStream_t stream) {
    const int lpb = kkt_lanes_per_block(a.N);
    if (lpb < 1 || a.nb < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((long long)a.nb + lpb - 1) / lpb)), block(KKT_BLOCK);
    hipLaunchKernelGGL(kkt_qp_kernel, grid, block, 0, stream, a, lpb);
    return hipGetLastError();
}

}  // namespace qsp
