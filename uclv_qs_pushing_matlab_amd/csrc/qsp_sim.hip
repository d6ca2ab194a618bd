// qsp_sim.hip — what runs around the solve on gfx950 (FP64): the device closed loop's plant, reference
// generation and staging, and the building-block kernels.
//
//   closed_loop_pre_kernel, plant_kernel   helper.m:195-322 around each NMPC_controller.solve;
//   delay_sim_kernel, reproject_kernel     NMPC_controller.delay_buffer_sim and the disturbance's
//                                          re-projection on their own;
//   sim_noise_kernel                       the table of sim_noise that the loops draw with the handle's
//                                          generator (qsp_noise.hpp);
//   straight_lines_kernel                  TrajectoryGenerator.straight_line per lane;
//   waypoints_kernel                       TrajectoryGenerator.waypoints_gen / waypoint_gen_fixed_angle
//                                          per lane;
//   stage_yref_kernel                      get_y_ref: a controller step's references out of the table;
//   spline_, dynamics_, rk4_, vbound_kernel  one device function each (qsp_math.hpp), for the tests and
//                                          the oracle comparison.
//
// The plant's step is euler_step_cm (qsp_math.hpp), the one the prologue, the rollout and the open-loop
// simulation take: their chains agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qsp_nmpc.h"
#include "qsp_ipm.hpp"
#include "qsp_kernels.h"
#include "qsp_noise.hpp"

namespace qsp {

// ------------------------------------------------------- closed-loop plant
// helper.m:195-322 (closed_loop_matlab), one thread per lane, around each NMPC_controller.solve:
//   closed_loop_pre_kernel: the disturbance (:221-236), sim_noise (:240-242), the trajectory log
//     and the controller's delay prediction delay_buffer_sim (NMPC_controller.m:112-120) into the
//     solver's x0;
//   plant_kernel: the controller input buffer push (helper.m:255), the plant x(:,i+1) = x(:,i) +
//     Ts * evalModelVariableShape(x(:,i), u) with the plant's own delay buffer (:289-307), logs.

// With a plant model installed (qsp_set_plant_*) the three kernels below take lane i's shape, c and
// mu from it (plant_of): the reference simulates, predicts and re-projects with `plant`
// (helper.m:226-233, :244, :294-307) and keeps the controller's model for solve alone.

// Lane i's plant: the shape and the two constants f reads beside it
struct PlantModel {
    const ShapeDev* sh;
    LaneCM cm;
};
__device__ __forceinline__ PlantModel plant_of(const ClosedLoopArgs& a, int i) {
    const ShapeDev& sh = a.pshapes ? shape_clamped(a.pshapes, a.n_pshapes, a.psid, i)
                                   : shape_clamped(a.shapes, a.n_shapes, a.sid, i);
    return PlantModel{&sh, LaneCM{a.pc ? a.pc[i] : sh.c, a.pmu ? a.pmu[i] : sh.mu}};
}

__global__ void closed_loop_pre_kernel(ClosedLoopArgs a, int t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B) return;
    const PlantModel pm = plant_of(a, i);
    const ShapeDev& sh = *pm.sh;
    double x[4] = {a.x[(size_t)i * 4], a.x[(size_t)i * 4 + 1], a.x[(size_t)i * 4 + 2], a.x[(size_t)i * 4 + 3]};
    if (a.dist_step > 0 && t + 1 == a.dist_step) {
        disturb_contact(sh, a.dist_amp ? a.dist_amp[i] : 0.0, x);   // :224-234
    }
    if (a.noise) {
        for (int c = 0; c < 4; ++c) x[c] += a.noise[((size_t)t * a.B + i) * 4 + c];
    } else if (a.gen.on) {   // the same values, drawn here
        double nz[4];
        sim_noise(a.gen, a.lane_scale, i, t, nz);
        for (int c = 0; c < 4; ++c) x[c] = x[c] + nz[c];
    }
    for (int c = 0; c < 4; ++c) {
        a.x[(size_t)i * 4 + c] = x[c];
        if (a.Xtraj) a.Xtraj[((size_t)i * (a.n_steps + 1) + t) * 4 + c] = x[c];
    }
    delay_predict(*pm.sh, pm.cm, a.Ts, a.D, a.ubc + (size_t)i * a.D * 2, x);   // delay_buffer_sim
    for (int c = 0; c < 4; ++c) a.xs[(size_t)i * 4 + c] = x[c];
    if (a.Xsim)
        for (int c = 0; c < 4; ++c) a.Xsim[((size_t)i * a.n_steps + t) * 4 + c] = x[c];
}

// Row of lane i's reference table at the 1-based column col, clamped at both ends as get_y_ref clamps
// (NMPC_controller.m:307-313); the table as installed, without the delay prefix
__device__ __forceinline__ const double* metrics_ref(const ClosedLoopArgs& a, int i, int col) {
    col = col > a.mT ? a.mT : col;
    col = col < 1 ? 1 : col;
    return a.mtraj + ((size_t)(a.mper_lane ? i : 0) * a.mT + (size_t)(col - 1)) * 6;
}

// qsp_closed_loop_metrics' accumulators of lane i for step t (0-based): x the logged plant state (after
// disturbance and noise), xn the state after the plant step, u the commanded and ua the applied input.
// Plain products and sums in step order (no qfma), so that numpy restates them bit for bit.
__device__ __forceinline__ void metrics_step(const ClosedLoopArgs& a, const PlantModel& pm, int i, int t,
                                             const double x[4], const double xn[4], const double u[2],
                                             const double ua[2]) {
    double* m = a.metrics + (size_t)i * CL_NMETRICS;
    const double* r = metrics_ref(a, i, a.index0[i] + t);
    const double ex = x[0] - r[0], ey = x[1] - r[1], et = x[2] - r[2];
    const double e2 = ex * ex + ey * ey;
    m[0] = m[0] + e2;
    m[1] = e2 > m[1] ? e2 : m[1];
    m[2] = m[2] + et * et;
    if (t + 1 == a.n_steps) {
        const double* re = metrics_ref(a, i, a.index0[i] + a.n_steps);
        const double fx = xn[0] - re[0], fy = xn[1] - re[1];
        m[3] = fx * fx + fy * fy;
    }
    m[4] = m[4] + (u[0] * u[0] + u[1] * u[1]);
    if (a.status[i] != 0) m[5] = m[5] + 1.0;
    const int mode = motion_cone_cm(*pm.sh, pm.cm, x[3], ua[0], ua[1]).mode;
    if (mode != QSP_MODE_NONE) m[5 + mode] = m[5 + mode] + 1.0;   // 6, 7, 8: ST, SL, SR
    if (!(x[3] >= a.s_lo && x[3] <= a.s_hi)) m[9] = m[9] + 1.0;
}

__global__ void plant_kernel(ClosedLoopArgs a, int t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B) return;
    const PlantModel pm = plant_of(a, i);
    double xi[4] = {a.x[(size_t)i * 4], a.x[(size_t)i * 4 + 1], a.x[(size_t)i * 4 + 2], a.x[(size_t)i * 4 + 3]};
    const double u[2] = {a.u0[(size_t)i * 2], a.u0[(size_t)i * 2 + 1]};
    double ua[2];   // u_buff_contr takes u; the plant applies u or u_buff_plant(:, end), which then takes u
    buffers_step(a.ubc + (size_t)i * a.D * 2, a.D, a.ubp + (size_t)i * a.Dp * 2, a.Dp, u, ua);
    double xn[4] = {xi[0], xi[1], xi[2], xi[3]};   // the metrics read the state before the step too
    euler_step_cm(*pm.sh, pm.cm, a.Ts, xn, ua[0], ua[1]);
    for (int c = 0; c < 4; ++c) {
        a.x[(size_t)i * 4 + c] = xn[c];
        if (a.Xtraj && t + 1 == a.n_steps) a.Xtraj[((size_t)i * (a.n_steps + 1) + t + 1) * 4 + c] = xn[c];
    }
    if (a.Utraj) {
        a.Utraj[((size_t)i * a.n_steps + t) * 2] = u[0];
        a.Utraj[((size_t)i * a.n_steps + t) * 2 + 1] = u[1];
    }
    if (a.Straj) a.Straj[(size_t)i * a.n_steps + t] = a.status[i];
    if (a.metrics) metrics_step(a, pm, i, t, xi, xn, u, ua);
}

// NMPC_controller.delay_buffer_sim alone (qsp_delay_buffer_sim)
__global__ void delay_sim_kernel(ClosedLoopArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.B) return;
    const PlantModel pm = plant_of(a, i);
    double x[4] = {a.x[(size_t)i * 4], a.x[(size_t)i * 4 + 1], a.x[(size_t)i * 4 + 2], a.x[(size_t)i * 4 + 3]};
    delay_predict(*pm.sh, pm.cm, a.Ts, a.D, a.ubc + (size_t)i * a.D * 2, x);   // delay_buffer_sim
    for (int c = 0; c < 4; ++c) a.xs[(size_t)i * 4 + c] = x[c];
}

__global__ void reproject_kernel(const ShapeDev* shapes, int n_shapes, const int32_t* sid, int n, const double* px,
                                 const double* py, const double* s0, double* s) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    s[i] = reproject_contact(shape_clamped(shapes, n_shapes, sid, i), px[i], py[i], s0[i]);
}

// qsp_gen_sim_noise: one thread per (step, lane), four doubles each
__global__ void sim_noise_kernel(SimNoiseGen g, const double* lane_scale, int B, long long n, double* noise) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const long long t = e / B;
    double nz[4];
    sim_noise(g, lane_scale, (int)(e - t * B), (int)t, nz);
    for (int c = 0; c < 4; ++c) noise[(size_t)e * 4 + c] = nz[c];
}

hipError_t launch_sim_noise(const SimNoiseGen& g, const double* lane_scale, int B, int n_steps, double* noise,
                            hipStream_t stream) {
    const long long n = (long long)B * n_steps, blocks = (n + 255) / 256;
    if (B < 1 || n_steps < 1 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sim_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, lane_scale, B, n, noise);
    return hipGetLastError();
}

hipError_t launch_closed_loop_pre(const ClosedLoopArgs& a, int t, hipStream_t stream) {
    hipLaunchKernelGGL(closed_loop_pre_kernel, dim3((a.B + 127) / 128), dim3(128), 0, stream, a, t);
    return hipGetLastError();
}

hipError_t launch_plant(const ClosedLoopArgs& a, int t, hipStream_t stream) {
    hipLaunchKernelGGL(plant_kernel, dim3((a.B + 127) / 128), dim3(128), 0, stream, a, t);
    return hipGetLastError();
}

hipError_t launch_delay_sim(const ClosedLoopArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(delay_sim_kernel, dim3((a.B + 127) / 128), dim3(128), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_reproject(const ShapeDev* shapes, int n_shapes, const int32_t* sid, int n, const double* px,
                            const double* py, const double* s0, double* s, hipStream_t stream) {
    hipLaunchKernelGGL(reproject_kernel, dim3((n + 127) / 128), dim3(128), 0, stream, shapes, n_shapes, sid, n, px, py,
                       s0, s);
    return hipGetLastError();
}

// ------------------------------------------------- reference generation
// TrajectoryGenerator.straight_line (TrajectoryGenerator.m:39-79), one thread per
// (lane, sample): quintic time scaling s(t) = 6 tau^5 - 15 tau^4 + 10 tau^3, tau = t / tf
// (:39-42), x(t) = x0 + s(t) (xf - x0) on (x, y, theta); rows [x y theta 0 0 0] as
// main.m:165-178 builds y_ref (s_ref = 0, u_ref = 0).  auto_angle: theta follows its own
// quintic over tf / 2 and then holds its final value (:58-66).
__device__ __forceinline__ double quintic(double t, double tf) {
    const double tau = t / tf;
    return qfma(qfma(6.0, tau, -15.0), tau, 10.0) * tau * tau * tau;
}

__global__ void straight_lines_kernel(int B, int T, const double* x0, const double* xf, double t0, double tf,
                                      double Ts, int auto_angle, double* traj) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)B * T) return;
    const int i = (int)(g / T), k = (int)(g - (size_t)i * T);
    const double t = qfma((double)k, Ts, t0);
    const double* a = x0 + (size_t)i * 3;
    const double* b = xf + (size_t)i * 3;
    const double s = quintic(t, tf);
    double* out = traj + g * 6;
    out[0] = qfma(s, b[0] - a[0], a[0]);
    out[1] = qfma(s, b[1] - a[1], a[1]);
    if (auto_angle) {
        const double tfa = 0.5 * tf;
        const int ka = (int)floor((tfa - t0) / Ts + 1e-9);      // last sample of t0:Ts:tf/2
        const double ta = qfma((double)(k < ka ? k : ka), Ts, t0);
        out[2] = qfma(quintic(ta, tf), b[2] - a[2], a[2]);
    } else {
        out[2] = qfma(s, b[2] - a[2], a[2]);
    }
    out[3] = 0.0;
    out[4] = 0.0;
    out[5] = 0.0;
}

hipError_t launch_straight_lines(int B, int T, const double* x0, const double* xf, double t0, double tf, double Ts,
                                 int auto_angle, double* traj, hipStream_t stream) {
    const size_t n = (size_t)B * T;
    hipLaunchKernelGGL(straight_lines_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B, T, x0, xf,
                       t0, tf, Ts, auto_angle, traj);
    return hipGetLastError();
}

// TrajectoryGenerator.waypoints_gen (TrajectoryGenerator.m:96-143, the constant-speed polyline that
// trajectory.py restates) and waypoint_gen_fixed_angle (:81-95), one thread per (lane, sample) from the
// lane's waypoints and what qsp_gen_waypoints prepared of them: arrival times or row counts, the yaw of
// each segment, the lane's own row count T_i.  Rows [x y yaw s_ref 0 0]; a sample past the lane's last is
// the last one again.  Plain quotients, products and sums (no qfma), so that numpy restates every row bit
// for bit.
__global__ void waypoints_kernel(WaypointArgs a) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)a.B * a.T) return;
    const int i = (int)(g / a.T), Ti = a.T_lane[i];
    int j = (int)(g - (size_t)i * a.T);
    j = j < Ti ? j : Ti - 1;
    const int last = a.n_wp[i] - 2;   // the last segment
    const double* wp = a.wp + (size_t)i * a.K * 2;
    int k = 0;
    double x = wp[0], y = wp[1];      // row 0 of the linspace law
    if (a.law == QSP_WP_LAW_CONSTANT_SPEED) {
        const double* tk = a.knot + (size_t)i * a.K;
        const double t = (double)j * a.Ts;
        while (k < last && tk[k + 1] <= t) ++k;   // the last segment that has begun
        const double al = (t - tk[k]) / (tk[k + 1] - tk[k]);
        x = wp[2 * k] + al * (wp[2 * k + 2] - wp[2 * k]);
        y = wp[2 * k + 1] + al * (wp[2 * k + 3] - wp[2 * k + 1]);
    } else if (j > 0) {
        const int32_t* c = a.brk + (size_t)i * a.K;
        const int r = j - 1;                      // c[k] <= r < c[k + 1]: row m of segment k's n
        while (k < last && c[k + 1] <= r) ++k;
        const int m = r - c[k], n = c[k + 1] - c[k];
        if (m == n - 1) {                         // linspace ends on the waypoint itself
            x = wp[2 * k + 2];
            y = wp[2 * k + 3];
        } else {
            x = wp[2 * k] + (double)m * ((wp[2 * k + 2] - wp[2 * k]) / (double)(n - 1));
            y = wp[2 * k + 1] + (double)m * ((wp[2 * k + 3] - wp[2 * k + 1]) / (double)(n - 1));
        }
    }
    double* out = a.traj + g * 6;
    out[0] = x;
    out[1] = y;
    out[2] = a.yaw[(size_t)i * a.K + k];
    out[3] = a.s_ref ? a.s_ref[i] : 0.0;
    out[4] = 0.0;
    out[5] = 0.0;
}

hipError_t launch_waypoints(const WaypointArgs& a, hipStream_t stream) {
    const long long n = (long long)a.B * a.T, blocks = (n + 255) / 256;
    if (a.B < 1 || a.T < 1 || a.K < 2 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(waypoints_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// ----------------------------------------------------- building-block kernels
// sid[i] indexes the table as it is: the host entries check the ids first (check_ids, qsp_capi.hip)
__global__ void spline_kernel(const ShapeDev* shapes, const int32_t* sid, int n, const double* s,
                              double* C, double* D, double* Dd, double* kappa) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShapeDev& sh = shapes[sid[i]];
    SplineEval e;
    spline_eval(sh, s[i], e);
    for (int c = 0; c < 2; ++c) { C[2 * i + c] = e.C[c]; D[2 * i + c] = e.D[c]; Dd[2 * i + c] = e.Dd[c]; }
    kappa[i] = angle_rate_of(e);
}

__global__ void dynamics_kernel(const ShapeDev* shapes, const int32_t* sid, int n, const double* x, const double* u,
                                double* f, double* J) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShapeDev& sh = shapes[sid[i]];
    DynOut d;
    dynamics<true>(sh, x[4 * i + 2], x[4 * i + 3], u[2 * i], u[2 * i + 1], d);
    pack_dynamics(d, f + 4 * i, J + (size_t)24 * i);
}

__global__ void rk4_kernel(const ShapeDev* shapes, const int32_t* sid, int n, double h, const double* x, const double* u,
                           double* xn, double* Aout, double* Bout) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ShapeDev& sh = shapes[sid[i]];
    double xi[4] = {x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
    double ui[2] = {u[2 * i], u[2 * i + 1]};
    Lin L;
    rk4<true>(sh, h, xi, ui, L);
    pack_lin(L, xn + 4 * i, Aout + (size_t)16 * i, Bout + (size_t)8 * i);
}

__global__ void vbound_kernel(const ShapeDev* shapes, const int32_t* sid, int n, CtrlParams cp, const double* s,
                              double* vb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vb[i] = v_bound(shapes[sid[i]], cp, s[i]);
}

hipError_t launch_spline(const ShapeDev* shapes, const int32_t* sid, int n, const double* s, double* C, double* D,
                         double* Dd, double* kappa, hipStream_t stream) {
    hipLaunchKernelGGL(spline_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, shapes, sid, n, s, C, D, Dd, kappa);
    return hipGetLastError();
}
hipError_t launch_dynamics(const ShapeDev* shapes, const int32_t* sid, int n, const double* x, const double* u,
                           double* f, double* J, hipStream_t stream) {
    hipLaunchKernelGGL(dynamics_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, shapes, sid, n, x, u, f, J);
    return hipGetLastError();
}
hipError_t launch_rk4(const ShapeDev* shapes, const int32_t* sid, int n, double h, const double* x, const double* u,
                      double* xn, double* A, double* B, hipStream_t stream) {
    hipLaunchKernelGGL(rk4_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, shapes, sid, n, h, x, u, xn, A, B);
    return hipGetLastError();
}
hipError_t launch_vbound(const ShapeDev* shapes, const int32_t* sid, int n, CtrlParams cp, const double* s, double* vb,
                         hipStream_t stream) {
    hipLaunchKernelGGL(vbound_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, shapes, sid, n, cp, s, vb);
    return hipGetLastError();
}

}  // namespace qsp

// ------------------------------------------------- reference staging
// get_y_ref (NMPC_controller.m:307-313) for one controller step, one thread per lane.  Outside the
// namespace: the kernel keeps the name it had beside the C ABI.
__global__ void stage_yref_kernel(const double* traj, int T, int per_lane, const int32_t* index_time, int offset,
                                  int D, int B, int N, double* yref, double* yref_e) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    if (per_lane) traj += (size_t)i * T * 6;
    qsp::stage_yref(traj, T, D, index_time[i] + offset, N, yref + (size_t)i * N * 6, yref_e + (size_t)i * 4);
}

hipError_t qsp::launch_stage_yref(const double* traj, int T, int per_lane, const int32_t* index_time, int offset, int D,
                                  int B, int N, double* yref, double* yref_e, hipStream_t stream) {
    hipLaunchKernelGGL(stage_yref_kernel, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, stream, traj, T, per_lane,
                       index_time, offset, D, B, N, yref, yref_e);
    return hipGetLastError();
}
