// qsp_sens.hip — solution sensitivities du_k/dx_0 on gfx950 (FP64): the kernels of qsp_eval_sens /
// qsp_eval_sens_device / qsp_get_sens and qsp_qp_sens around the functions of qsp_sens.hpp (the definition
// is in that header).
//
// sens_lin_kernel: one thread per (lane, stage k < N), the lane fastest, so that its 20 stores per stage (a,
// B, Hx, Hu) go to consecutive addresses of the workspace (SensField, qsp_kernels.h); its loads (rows of X,
// U, PI, LAM of different lanes) are whole 16 .. 48 byte rows each.  A stage with a non-finite value writes
// NaN into its Hx, which the walk's flag then sees.
//
// sens_walk_kernel: one thread per lane, one wave per workgroup.  Backward over k = N-1 .. 0 with P (10) and
// the stage's 20 values in registers; the gain K_k goes to the K output and, when dU is asked for, to wK in
// the workspace's order, from where the forward pass of the same thread reads it back (a thread reads only
// what it wrote itself: no fence).  The QP-level entry runs the same walk on the caller's arrays (lane-major:
// its loads are not coalesced; that entry is for checks, not for rates).  A lane whose flag is unset gets NaN
// in every output it was asked for and 1 in flag; nothing of a lane is read by another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qsp_kernels.h"
#include "qsp_sens.hpp"

namespace qsp {

constexpr int SENS_LIN_BLOCK = 256;
constexpr int SENS_WALK_BLOCK = 64;

__global__ void __launch_bounds__(SENS_LIN_BLOCK) sens_lin_kernel(SensNlpArgs A) {
    const SolveParams& p = A.p;
    const int N = p.N;
    const size_t B = (size_t)A.B;
    const size_t gi = (size_t)blockIdx.x * SENS_LIN_BLOCK + threadIdx.x;
    if (gi >= B * (size_t)N) return;
    const int k = (int)(gi / B);
    const size_t i = gi - (size_t)k * B;
    double a[6], Bm[8], Hx[4], Hu[2];
    const bool fin = sens_nlp_stage(shape_clamped(A.pt.shapes, A.pt.n_shapes, A.pt.shape_id, (int)i), p, A.s0_bound, A.t_floor,
                                    k, PointRows(A.pt, N, i, k), a, Bm, Hx, Hu);
    if (!fin) Hx[0] = __builtin_nan("");
    double* w = A.ws + (size_t)k * SF_COUNT * B + i;
#pragma unroll
    for (int q = 0; q < 6; ++q) w[(size_t)(SF_A + q) * B] = a[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[(size_t)(SF_B + q) * B] = Bm[q];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[(size_t)(SF_HX + q) * B] = Hx[q];
#pragma unroll
    for (int q = 0; q < 2; ++q) w[(size_t)(SF_HU + q) * B] = Hu[q];
}

// where the walk takes a lane's stage data from
struct SensSrcWs {   // sens_lin_kernel's workspace
    const double* ws;
    size_t B, i;
    double We[4];
    __device__ __forceinline__ void terminal(double He[4]) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) He[q] = We[q];
    }
    __device__ __forceinline__ void dyn(int k, double a[6], double Bm[8]) const {
        const double* w = ws + (size_t)k * SF_COUNT * B + i;
#pragma unroll
        for (int q = 0; q < 6; ++q) a[q] = w[(size_t)(SF_A + q) * B];
#pragma unroll
        for (int q = 0; q < 8; ++q) Bm[q] = w[(size_t)(SF_B + q) * B];
    }
    __device__ __forceinline__ void stage(int k, double a[6], double Bm[8], double Hx[4], double Hu[2]) const {
        dyn(k, a, Bm);
        const double* w = ws + (size_t)k * SF_COUNT * B + i;
#pragma unroll
        for (int q = 0; q < 4; ++q) Hx[q] = w[(size_t)(SF_HX + q) * B];
#pragma unroll
        for (int q = 0; q < 2; ++q) Hu[q] = w[(size_t)(SF_HU + q) * B];
    }
};
struct SensSrcQp {   // the caller's QP arrays
    QpLaneData d;
    __device__ __forceinline__ void terminal(double He[4]) const {
#pragma unroll
        for (int q = 0; q < 4; ++q) He[q] = d.Hk(d.N)[q];
    }
    __device__ __forceinline__ void dyn(int k, double a[6], double Bm[8]) const {
        QpLaneData::free_entries(d.Ak(k), a);
#pragma unroll
        for (int q = 0; q < 8; ++q) Bm[q] = d.Bk(k)[q];
    }
    __device__ __forceinline__ void stage(int k, double a[6], double Bm[8], double Hx[4], double Hu[2]) const {
        dyn(k, a, Bm);
#pragma unroll
        for (int q = 0; q < 4; ++q) Hx[q] = d.Hk(k)[q];
#pragma unroll
        for (int q = 0; q < 2; ++q) Hu[q] = d.Hk(k)[4 + q];
    }
};

template <class Src>
__device__ __forceinline__ void sens_walk(const Src& src, int N, size_t nb, size_t i, double* wK, const SensOut& o) {
    double P[10], K[8], He[4];
    src.terminal(He);
    bool fin = sens_terminal(He, P);
    const bool fwd = o.dU != nullptr;
    for (int k = N - 1; k >= 0; --k) {
        double a[6], Bm[8], Hx[4], Hu[2];
        src.stage(k, a, Bm, Hx, Hu);
        fin = sens_back_step(a, Bm, Hx, Hu, P, K) && fin;
        if (o.K) {
#pragma unroll
            for (int q = 0; q < 8; ++q) o.K[(i * (size_t)N + k) * 8 + q] = K[q];
        }
        if (fwd) {
#pragma unroll
            for (int q = 0; q < 8; ++q) wK[((size_t)k * SENS_NK + q) * nb + i] = K[q];
        }
    }
    if (fwd) {
        double Phi[16];
        sens_identity(Phi);
        for (int k = 0; k < N; ++k) {
            double a[6], Bm[8], Kk[8], dU[8];
            src.dyn(k, a, Bm);
#pragma unroll
            for (int q = 0; q < 8; ++q) Kk[q] = wK[((size_t)k * SENS_NK + q) * nb + i];
            fin = sens_fwd_step(a, Bm, Kk, Phi, dU) && fin;
#pragma unroll
            for (int q = 0; q < 8; ++q) o.dU[(i * (size_t)N + k) * 8 + q] = dU[q];
        }
    }
    const double nan = __builtin_nan("");
#pragma unroll
    for (int q = 0; q < 8; ++q) o.K0[i * 8 + q] = fin ? K[q] : nan;
    if (o.P0) {
#pragma unroll
        for (int q = 0; q < 10; ++q) o.P0[i * 10 + q] = fin ? P[q] : nan;
    }
    if (o.flag) o.flag[i] = fin ? 0 : 1;
    if (!fin) {
        for (size_t q = 0; q < (size_t)N * 8; ++q) {
            if (o.K) o.K[i * (size_t)N * 8 + q] = nan;
            if (o.dU) o.dU[i * (size_t)N * 8 + q] = nan;
        }
    }
}

__global__ void __launch_bounds__(SENS_WALK_BLOCK) sens_walk_kernel(SensNlpArgs A) {
    const size_t i = (size_t)blockIdx.x * SENS_WALK_BLOCK + threadIdx.x;
    if (i >= (size_t)A.B) return;
    SensSrcWs src;
    src.ws = A.ws;
    src.B = (size_t)A.B;
    src.i = i;
#pragma unroll
    for (int q = 0; q < 4; ++q) src.We[q] = A.p.We[q];
    sens_walk(src, A.p.N, (size_t)A.B, i, A.wK, A.out);
}

__global__ void __launch_bounds__(SENS_WALK_BLOCK) sens_walk_qp_kernel(SensQpArgs A) {
    const size_t i = (size_t)blockIdx.x * SENS_WALK_BLOCK + threadIdx.x;
    if (i >= (size_t)A.nb) return;
    const SensSrcQp src = {QpLaneData(A.A, A.B, nullptr, A.H, nullptr, nullptr, nullptr, A.N, i)};
    sens_walk(src, A.N, (size_t)A.nb, i, A.wK, A.out);
}

static bool sens_out_ok(const SensOut& o, const double* wK) { return o.K0 && (!o.dU || wK); }

hipError_t launch_sens_nlp(const SensNlpArgs& a, hipStream_t stream) {
    if (a.B < 1 || a.p.N < 1 || !a.ws || !sens_out_ok(a.out, a.wK) || !(a.t_floor > 0.0)) return hipErrorInvalidValue;
    if (!a.pt.LAM && a.pt.PI && !a.pt.yref) return hipErrorInvalidValue;
    const size_t n = (size_t)a.B * (size_t)a.p.N;
    const dim3 lgrid((unsigned)((n + SENS_LIN_BLOCK - 1) / SENS_LIN_BLOCK)), lblock(SENS_LIN_BLOCK);
    hipLaunchKernelGGL(sens_lin_kernel, lgrid, lblock, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(((size_t)a.B + SENS_WALK_BLOCK - 1) / SENS_WALK_BLOCK)), block(SENS_WALK_BLOCK);
    hipLaunchKernelGGL(sens_walk_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_sens_qp(const SensQpArgs& a, hipStream_t stream) {
    if (a.nb < 1 || a.N < 1 || !a.A || !a.B || !a.H || !sens_out_ok(a.out, a.wK)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(((size_t)a.nb + SENS_WALK_BLOCK - 1) / SENS_WALK_BLOCK)), block(SENS_WALK_BLOCK);
    hipLaunchKernelGGL(sens_walk_qp_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace qsp
