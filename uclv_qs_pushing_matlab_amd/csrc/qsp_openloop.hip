// qsp_openloop.hip — contact modes and the open-loop simulation on gfx950 (FP64).
//
//   modes_kernel      one thread per (x, u): the motion cone and the contact mode (motion_cone,
//                     qsp_math.hpp), for a list of points or for a handle's device-resident trajectories;
//   open_loop_kernel  helper.open_loop_matlab (helper.m:132-193), one thread per (lane, candidate): per
//                     step the noise, the tangential clip, the plant's delay buffer, the mode and the
//                     Euler step x + Ts f(x, u) with the OCP's f (euler_step, qsp_math.hpp: the closed
//                     loop's plant step);
//   open_loop_noise_kernel  the same with the step's noise drawn from the handle's generator (qsp_noise.hpp)
//                     instead of read from a table.
//
// A candidate's arithmetic is the same sequence of IEEE operations at any M, B, lane index, position
// among the candidates, set of requested outputs and store path: results agree bit for bit, with
// qsp_rollout_cost's Euler x_end and with the building blocks (qsp_eval_spline, qsp_eval_modes) too.
//
// Thread mapping (qsp_candidates.hpp): a lane's candidates are adjacent threads.  With 64 candidates or
// more a workgroup serves one lane and stages its shape in LDS (candidates beyond a workgroup's
// size go to further workgroups of the lane); with fewer it serves floor(threads / M) lanes and reads
// the shapes through the vector cache.
//
// The trajectory stores.  A thread writes 32 + 16 + 16 + 4 bytes per step into rows that lie
// (T + 1) 32 B apart from its neighbours': 64 lanes of a wave into 64 different rows.  Two store paths,
// selected by the template parameter K:
//   K = 1      every thread stores its own rows as it goes (16-byte stores);
//   K = 4, 8   every thread collects K steps in LDS (rows padded by 16 bytes: conflict-free 16-byte LDS
//              stores), then the workgroup writes the tile out with consecutive threads on consecutive
//              16-byte pieces of a row: K 32 contiguous bytes of X per row, K 16 of U_out and S_p.
//   K = 0      no trajectory is requested (x_end, mode_steps only): nothing is staged or stored per step.
// Which of K = 1, 4, 8 runs by default is a measurement (ol_default_tile; scripts/open_loop_rate.py,
// profiles/open_loop/open_loop_rate.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qsp_nmpc.h"
#include "qsp_math.hpp"
#include "qsp_candidates.hpp"
#include "qsp_noise.hpp"

namespace qsp {

constexpr int OL_BLOCK = 256;        // largest workgroup (K = 0, 1)
constexpr int OL_TBLOCK = 64;        // workgroup of the tiled paths: K = 8 holds 596 bytes of LDS per thread

// ------------------------------------------------------------------ modes
__global__ void modes_kernel(const ShapeDev* shapes, int n_shapes, const int32_t* sid, long long n, int per, int xper,
                             const double* x, const double* u, int32_t* mode, double* cone) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long long grp = e / per;
    const int k = (int)(e - grp * per);
    const ShapeDev& sh = shape_clamped(shapes, n_shapes, sid, (int)grp);
    const double* xe = x + ((size_t)grp * xper + k) * 4;
    const MotionCone mc = motion_cone(sh, xe[3], u[2 * e], u[2 * e + 1]);
    mode[e] = mc.mode;
    if (cone) {
        cone[3 * e] = mc.gl;
        cone[3 * e + 1] = mc.gr;
        cone[3 * e + 2] = mc.rho;
    }
}

hipError_t launch_modes(const ShapeDev* shapes, int n_shapes, const int32_t* sid, long long n, int per, int xper,
                        const double* x, const double* u, int32_t* mode, double* cone, hipStream_t stream) {
    hipLaunchKernelGGL(modes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, shapes, n_shapes, sid, n,
                       per, xper, x, u, mode, cone);
    return hipGetLastError();
}

// ------------------------------------------------------------------ open loop
// LDS tile of a workgroup of nt threads: [X nt x RX | U_out nt x RU | S_p nt x RU] doubles, [mode nt x RM] ints
template <int K>
struct Tile {
    static constexpr int RX = 4 * K + 2, RU = 2 * K + 2, RM = K + 1;
    static constexpr size_t bytes(int nt) { return (size_t)nt * ((RX + 2 * RU) * sizeof(double) + RM * sizeof(int32_t)); }
    double *X, *U, *S;
    int32_t* M;
    __device__ __forceinline__ Tile(double* base, int nt)
        : X(base), U(base + nt * RX), S(base + nt * (RX + RU)), M(reinterpret_cast<int32_t*>(base + nt * (RX + 2 * RU))) {}
};

__device__ __forceinline__ void st2(double* p, double a, double b) { *reinterpret_cast<double2*>(p) = make_double2(a, b); }

// steps [k0, k0 + kt) of the workgroup's rows gbase .. gbase + nrows - 1: consecutive threads write
// consecutive 16-byte pieces of a row (X: 2 K pieces per row; U_out, S_p: K), the modes 4 bytes each
template <int K>
__device__ __forceinline__ void flush_tile(const OpenLoopArgs& A, const Tile<K>& t, size_t gbase, int nrows, int k0, int kt) {
    const int nt = blockDim.x, T = A.T;
    if (A.X) {
        for (int q = threadIdx.x; q < nrows * 2 * K; q += nt) {
            const int r = q / (2 * K), c = q - r * 2 * K;
            if ((c >> 1) < kt)
                *reinterpret_cast<double2*>(A.X + ((gbase + r) * (size_t)(T + 1) + k0) * 4 + 2 * c) =
                    *reinterpret_cast<const double2*>(t.X + r * Tile<K>::RX + 2 * c);
        }
    }
    for (int q = threadIdx.x; q < nrows * K; q += nt) {
        const int r = q / K, c = q - r * K;
        if (c >= kt) continue;
        const size_t o = (gbase + r) * (size_t)T + k0 + c;
        if (A.U_out) *reinterpret_cast<double2*>(A.U_out + o * 2) = *reinterpret_cast<const double2*>(t.U + r * Tile<K>::RU + 2 * c);
        if (A.S_p) *reinterpret_cast<double2*>(A.S_p + o * 2) = *reinterpret_cast<const double2*>(t.S + r * Tile<K>::RU + 2 * c);
        if (A.mode) A.mode[o] = t.M[r * Tile<K>::RM + c];
    }
}

// The workgroup's rows gbase + threadIdx.x, threadIdx.x < nrows (lane: this thread's; every thread of the
// workgroup calls this, the tiled paths synchronise inside).
// GEN: the step's noise is drawn from A.gen (qsp_noise.hpp) instead of read from A.noise.
template <int K, bool GEN>
__device__ __forceinline__ void open_loop_rows(const OpenLoopArgs& A, const ShapeDev& sh, int lane, size_t gbase, int nrows,
                                               double* tile_lds) {
    const bool active = (int)threadIdx.x < nrows;
    const size_t g = gbase + threadIdx.x, BM = (size_t)A.B * A.M;
    const int T = A.T, D = A.D;
    const bool replay = A.u_steps != 1;
    const double* Ug = A.U + g * (size_t)A.u_steps * 2;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    double uc[2] = {0.0, 0.0};
    if (active) {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = A.x0[(size_t)lane * 4 + c];
        if (!replay) { uc[0] = Ug[0]; uc[1] = Ug[1]; }
    }
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    const bool want_sp = K != 0 && A.S_p != nullptr;

    // one step: logs row i through `log`, then advances x
    auto step = [&](int i, auto log) {
        if constexpr (GEN) {                                   // helper.m:155, the table's values drawn here
            double nz[4];
            sim_noise(A.gen, A.lane_scale, lane, i, nz);
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = x[c] + nz[c];
        } else if (A.noise) {                                  // helper.m:155
            const double* nz = A.noise + ((size_t)i * A.B + lane) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) x[c] = x[c] + nz[c];
        }
        double u[2] = {uc[0], uc[1]};
        if (replay) { u[0] = Ug[2 * i]; u[1] = Ug[2 * i + 1]; }
        double sp[2] = {0.0, 0.0};
        if (A.clip || want_sp) {                               // :162-166, :187
            SplineEval e;
            spline_eval(sh, mat_mod(x[3], sh.b), e);
            if (A.clip) {
                const double v = A.v_alpha / fabs(angle_rate_of(e));
                u[1] = (v < u[1]) ? v : u[1];                  // MATLAB's min(v, u_t): a NaN never wins
            }
            sp[0] = e.C[0];
            sp[1] = e.C[1];
        }
        double ua[2] = {u[0], u[1]};
        if (D > 0) {                                           // :169-177: u_buff_plant(:, end), then the push
            ua[0] = 0.0;
            ua[1] = 0.0;
            double* slot = A.ring + (size_t)(i % D) * BM + g;  // holds step i - D's clipped u_t
            if (i >= D) {
                ua[0] = replay ? Ug[2 * (i - D)] : uc[0];      // u_n is never clipped
                ua[1] = A.clip ? *slot : (replay ? Ug[2 * (i - D) + 1] : uc[1]);
            }
            if (A.clip) *slot = u[1];
        }
        const MotionCone mc = motion_cone(sh, x[3], ua[0], ua[1]);
        n0 += mc.mode == QSP_MODE_NONE;
        n1 += mc.mode == QSP_MODE_ST;
        n2 += mc.mode == QSP_MODE_SL;
        n3 += mc.mode == QSP_MODE_SR;
        log(i, u, sp, mc.mode);
        euler_step(sh, A.Ts, x, ua[0], ua[1]);
    };

    if constexpr (K == 0) {
        if (active)
            for (int i = 0; i < T; ++i) step(i, [](int, const double*, const double*, int) {});
    } else if constexpr (K == 1) {
        if (active)
            for (int i = 0; i < T; ++i)
                step(i, [&](int ii, const double* u, const double* sp, int mode) {
                    const size_t o = g * (size_t)T + ii;
                    if (A.X) {
                        double* X = A.X + (g * (size_t)(T + 1) + ii) * 4;
                        st2(X, x[0], x[1]);
                        st2(X + 2, x[2], x[3]);
                    }
                    if (A.U_out) st2(A.U_out + o * 2, u[0], u[1]);
                    if (A.S_p) st2(A.S_p + o * 2, sp[0], sp[1]);
                    if (A.mode) A.mode[o] = mode;
                });
    } else {
        const Tile<K> t(tile_lds, blockDim.x);
        double* tx = t.X + threadIdx.x * Tile<K>::RX;
        double* tu = t.U + threadIdx.x * Tile<K>::RU;
        double* ts = t.S + threadIdx.x * Tile<K>::RU;
        int32_t* tm = t.M + threadIdx.x * Tile<K>::RM;
        for (int k0 = 0; k0 < T; k0 += K) {                    // uniform over the workgroup
            const int kt = T - k0 < K ? T - k0 : K;
            if (active)
                for (int kk = 0; kk < kt; ++kk)
                    step(k0 + kk, [&](int, const double* u, const double* sp, int mode) {
                        st2(tx + 4 * kk, x[0], x[1]);
                        st2(tx + 4 * kk + 2, x[2], x[3]);
                        st2(tu + 2 * kk, u[0], u[1]);
                        st2(ts + 2 * kk, sp[0], sp[1]);
                        tm[kk] = mode;
                    });
            __syncthreads();
            flush_tile<K>(A, t, gbase, nrows, k0, kt);
            __syncthreads();                                   // the tile is rewritten by the next K steps
        }
    }
    if (!active) return;
    if (K != 0 && A.X) {
        double* X = A.X + (g * (size_t)(T + 1) + T) * 4;
#pragma unroll
        for (int c = 0; c < 4; ++c) X[c] = x[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) A.x_end[g * 4 + c] = x[c];
    if (A.mode_steps) {
        int32_t* ms = A.mode_steps + g * 4;
        ms[0] = n0; ms[1] = n1; ms[2] = n2; ms[3] = n3;
    }
}

// ONE_LANE: blockIdx.x is the lane, blockIdx.y the block of blockDim.x candidates (dynamic LDS: the shape,
// then the tile).  Otherwise the workgroup serves lpb = floor(blockDim / M) lanes, thread t the candidate
// t % M of its lane t / M; its rows are lane0 M + t, contiguous in every output.
template <int K, bool ONE_LANE>
__global__ void __launch_bounds__(OL_BLOCK) open_loop_kernel(OpenLoopArgs A, int lpb) {
    extern __shared__ __align__(16) double ol_lds[];
    if (ONE_LANE) {
        const int lane = blockIdx.x;
        // stage_shape (qsp_candidates.hpp) written out: through the call these four instantiations'
        // scalar instructions come out in another order (profiles/sim_layer/README.md)
        const double* sg = reinterpret_cast<const double*>(&shape_clamped(A.shapes, A.n_shapes, A.shape_id, lane));
        for (int q = threadIdx.x; q < SHAPE_D; q += blockDim.x) ol_lds[q] = sg[q];
        __syncthreads();
        const ShapeDev& sh = *reinterpret_cast<const ShapeDev*>(ol_lds);
        const int m0 = blockIdx.y * blockDim.x, left = A.M - m0;   // left >= 1 by the grid
        open_loop_rows<K, false>(A, sh, lane, (size_t)lane * A.M + m0, left < (int)blockDim.x ? left : (int)blockDim.x,
                                 ol_lds + SHAPE_D);
    } else {
        const long long lane0 = (long long)blockIdx.x * lpb;
        const long long nl = A.B - lane0 < lpb ? A.B - lane0 : lpb;
        const int nrows = (int)nl * A.M;
        long long lane = lane0 + (int)threadIdx.x / A.M;
        if (lane >= A.B) lane = A.B - 1;                       // an idle thread: a valid shape, no loads or stores
        open_loop_rows<K, false>(A, shape_clamped(A.shapes, A.n_shapes, A.shape_id, (int)lane), (int)lane, (size_t)lane0 * A.M,
                                 nrows, ol_lds);
    }
}

// The same workgroups with the step's noise drawn from A.gen.  A kernel of its own, not a branch in the one
// above: with the draw compiled into the kernels of a run without noise, the tiled ones went from 121 to 131
// VGPRs and from 19 to 67 spilled SGPRs, and open_loop_kernel's code must stay what it was
// (profiles/sim_noise/README.md).
template <int K, bool ONE_LANE>
__global__ void __launch_bounds__(OL_BLOCK) open_loop_noise_kernel(OpenLoopArgs A, int lpb) {
    extern __shared__ __align__(16) double ol_lds[];
    if (ONE_LANE) {
        const int lane = blockIdx.x;
        stage_shape(shape_clamped(A.shapes, A.n_shapes, A.shape_id, lane), ol_lds);
        __syncthreads();
        const int m0 = blockIdx.y * blockDim.x, left = A.M - m0;
        open_loop_rows<K, true>(A, *reinterpret_cast<const ShapeDev*>(ol_lds), lane, (size_t)lane * A.M + m0,
                                left < (int)blockDim.x ? left : (int)blockDim.x, ol_lds + SHAPE_D);
    } else {
        const long long lane0 = (long long)blockIdx.x * lpb;
        const long long nl = A.B - lane0 < lpb ? A.B - lane0 : lpb;
        long long lane = lane0 + (int)threadIdx.x / A.M;
        if (lane >= A.B) lane = A.B - 1;
        open_loop_rows<K, true>(A, shape_clamped(A.shapes, A.n_shapes, A.shape_id, (int)lane), (int)lane, (size_t)lane0 * A.M,
                                (int)nl * A.M, ol_lds);
    }
}

template <int K>
static hipError_t launch_ol(const OpenLoopArgs& a, hipStream_t stream) {
    const int cap = K >= 4 ? OL_TBLOCK : OL_BLOCK;
    if (a.M >= ONE_LANE_M) {
        const int nt = wg_threads(a.M, cap);
        const long long blocks = ((long long)a.M + nt - 1) / nt;
        if (blocks > 65535) return hipErrorInvalidValue;
        const size_t lds = sizeof(ShapeDev) + (K >= 4 ? Tile<(K >= 4 ? K : 4)>::bytes(nt) : 0);
        const auto kernel = a.gen.on ? open_loop_noise_kernel<K, true> : open_loop_kernel<K, true>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)a.B, (unsigned)blocks), dim3((unsigned)nt), lds, stream, a, 1);
    } else {
        const int lpb = cap / a.M;
        const size_t lds = K >= 4 ? Tile<(K >= 4 ? K : 4)>::bytes(cap) : 0;
        const auto kernel = a.gen.on ? open_loop_noise_kernel<K, false> : open_loop_kernel<K, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(((long long)a.B + lpb - 1) / lpb)), dim3((unsigned)cap), lds, stream, a,
                           lpb);
    }
    return hipGetLastError();
}

// The store path of a call that leaves the choice to the library: the faster one measured on one MI355X at
// 65 536 rows of 200 steps (profiles/open_loop/open_loop_rate.txt) -- several lanes per workgroup (M = 1):
// tiles of 4 steps 1.15 ms, direct 1.28 ms, tiles of 8 steps 1.30 ms; one lane per workgroup (M = 64):
// direct 0.79 ms, tiles of 4 steps 0.93 ms, of 8 steps 1.28 ms.
static int ol_default_tile(const OpenLoopArgs& a) { return a.M >= ONE_LANE_M ? 1 : 4; }

hipError_t launch_open_loop(const OpenLoopArgs& a, hipStream_t stream) {
    const bool traj = a.X || a.U_out || a.S_p || a.mode;
    // the 16-byte stores of both paths need 16-byte aligned rows (T + 1) 32 B and T 16 B apart: aligned bases
    const bool al = (((uintptr_t)a.X | (uintptr_t)a.U_out | (uintptr_t)a.S_p) & 15) == 0;
    if (traj && !al) return hipErrorInvalidValue;
    if (!traj) return launch_ol<0>(a, stream);
    const int tile = a.tile ? a.tile : ol_default_tile(a);
    if (tile == 8) return launch_ol<8>(a, stream);
    if (tile == 4) return launch_ol<4>(a, stream);
    return launch_ol<1>(a, stream);
}

}  // namespace qsp
