// qsp_kernels.h — kernel argument blocks and launchers (internal to the .so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qsp_layout.h"
#include "qsp_point.hpp"
#include "qsp_types.h"

#define QSP_FLAG_CONTROLLER 1u  // NMPC_controller.solve prologue: s pre-wrap, cold/warm start, clip, Euler rollout
#define QSP_FLAG_SHIFT 2u       // write the warm start shifted by one stage (NMPC_controller.m:397-399)
#define QSP_FLAG_POISON 4u      // debug (QSP_DEBUG_POISON=1): QP kernels fill their LDS with NaN first
#define QSP_FLAG_RUNTIME_N 8u   // developer A/B (QSP_FIXED_HORIZON=0): never the kernels compiled for one horizon (host only)

namespace qsp {

// Layout of SolveArgs' workspace, for the kernels that index it (qsp_solver.hip) and the host that sizes and
// packs it (qsp_devbuf.hpp, qsp_capi.hip).  wlin, wnlp and wqp are SoA over (instance, stage): field f of
// stage k of instance i at f * B(N+1) + i(N+1) + k.
enum LinField : int { L_A = 0, L_B = 6, L_BB = 14, L_G = 18, L_COUNT = 24 };               // wlin
enum NlpField : int { W_PI = 0, W_LAM = 4, W_NU = 10, W_ETA = 14, W_COUNT = 20 };          // wnlp (nlp_mode 1)
enum QpField : int { Q_DX = 0, Q_DU = 4, Q_PI = 6, Q_LAM = 10, Q_COUNT = 16 };             // wqp (nlp_mode 1)
constexpr int ADJ_REC = 11;                         // wadj: doubles per stage 1..N of the adjoint record
constexpr int PACK_KEYS_MAX = 1024;                 // whist: (maxkey + 1)^2 wave-packing keys
constexpr int WHIST_PER_PART = 4 * PACK_KEYS_MAX;   // whist of one part of the SQP loop (launch_sqp)

struct SolveArgs {
    SolveParams p;
    int32_t B;
    // instance range [i0, i0 + nI) of one QP / line-search launch: launch_sqp may split the
    // batch into parts iterated on their own HIP streams (whist then points at the part's own
    // histogram); strides of the SoA workspace stay B(N+1)
    int32_t i0, nI;
    uint32_t flags;
    const ShapeDev* shapes;
    int32_t n_shapes;
    const int32_t* shape_id;   // B (nullptr: shape 0); clamped into [0, n_shapes)
    const double* x0;          // B x 4
    const double* yref;        // B x N x 6
    const double* yref_e;      // B x 4
    const double* X_in;        // B x (N+1) x 4   initial guess / warm start
    const double* U_in;        // B x N x 2
    uint8_t* warm_valid;       // B (controller mode; nullptr: always cold)
    const double* PI_in;       // B x N x 4   initial dynamics multipliers (nlp_mode 1; nullptr: zeros)
    double* u0;                // B x 2
    double* X_out;             // B x (N+1) x 4
    double* U_out;             // B x N x 2
    double* PI_out;            // B x N x 4
    int32_t* status;           // B
    int32_t* sqp_iter;         // B
    int32_t* qp_iter;          // B (sum of IPM iterations)
    int32_t* qp_capped;        // B (QPs stopped by the iteration cap; nullptr: not counted)
    int32_t* qp_stalled;       // B (QPs stopped by the stall exit; nullptr: not counted)
    double* cost;              // B
    // workspace (device, owned by the handle)
    double* wX;                // B x (N+1) x 4   SQP iterate
    double* wU;                // B x N x 2
    double* wx0;               // B x 4           x0 after the controller's s pre-wrap
    double* wlin;              // 24 x B(N+1)     stage data (A, B, defect, gradient), SoA (LinField)
    double* wnlp;              // 20 x B(N+1)     nlp_mode 1: PI(4), LAM(6), merit weights NU(4), ETA(6), SoA (NlpField)
    int32_t* wdone;            // B               nlp_mode 1: converged (KKT tolerances met)
    double* wres;              // B x 4           nlp_mode 1: the last KKT test's residuals (stat, eq, ineq, comp;
                               //                 nullptr: not recorded).  At max_iter (status 2) that is the test
                               //                 before the last QP: the final iterate is not re-tested (acados
                               //                 v0.2.1 semantics as restated; unpinned, qsp_nmpc.h)
    double* wqp;               // 16 x B(N+1)     nlp_mode 1: QP step dx(4), du(2), multipliers pi(4), lam(6), SoA
    int32_t* wperm;            // B               wave packing order of the QP kernel (nullptr: identity)
    int32_t* wnit;             // B               IPM iterations of each instance's last four QPs (8 bits each, last lowest)
    int32_t* whist;            // 4 x 1024        per parity of the SQP iteration: histogram of the wave-packing
                               //                 keys (accumulated by the QP kernel) and running scatter offsets
    double* wadj;              // B x N x 11      nlp_mode 0: adjoint record of the instance's last successful QP
                               //                 (ADJ_REC doubles per stage 1..N, instance-major)
    int32_t* wadjv;            // B               nlp_mode 0: the record is valid (a QP of this solve wrote it)
    // QP-level interface only (qsp_qp_solve): when qp_dx != nullptr the QP kernel
    // reports the QP solution instead of updating the iterate
    double* qp_dx;             // B x (N+1) x 4
    double* qp_du;             // B x N x 2
    double* qp_lam;            // B x N x 6
};

// Shape of instance i of a kernel's argument block (solver, closed loop, rollout, open loop, modes).  The
// ids are device data that the host cannot validate without a round trip, and the table may have shrunk
// since they were set, so these kernels clamp them into the table, by shape_clamp.  The four
// building-block kernels (spline_, dynamics_, rk4_, vbound_kernel) do not: they index shapes[sid[i]] with
// ids that come from the host in the same call, which the entry point has checked (check_ids).
__device__ __forceinline__ int shape_clamp(int id, int n_shapes) { return id < 0 ? 0 : (id >= n_shapes ? n_shapes - 1 : id); }
__device__ __forceinline__ const ShapeDev& shape_clamped(const ShapeDev* shapes, int n_shapes, const int32_t* sid, int i) {
    return shapes[shape_clamp(sid ? sid[i] : 0, n_shapes)];
}

// QSP_WALK_* of a handle's QP kernels (factor_walk_of, qsp_layout.h: the launchers select by it, factor_alt)
int factor_walk_kind(const SolveParams& p, int S);
int qp_fixed_horizon(const SolveParams& p, int S, uint32_t flags);   // compiled horizon of the per-iteration QP launches (0: none)
void mfw_prepare(SolveParams& p);   // SolveParams::mfw_on / mfw_is from N and mfma_walk
// Multi-stream split of the SQP loop (SqpStreams::parts = P > 1): the instances are cut into
// P parts and each part runs its own (sort, qp_step) sequence on its own stream (part 0 on
// the solve's stream, part p on aux[p-1]), so the launch tail of one part's QP overlaps the
// other parts' work.  Results are bit-identical to the single-stream loop (instances are
// independent).  Streams and events owned by the handle.
// Two parts at most: measured (scripts/parts_sweep.sh) three or four parts run slower than one
// at every batch size (down to half the rate at B = 4 096) -- with GPU_MAX_HW_QUEUES = 4 the
// extra streams share hardware queues, whose kernels then serialise across parts.
constexpr int SQP_MAX_PARTS = 2;
struct SqpStreams {
    hipStream_t aux[SQP_MAX_PARTS - 1] = {};
    hipEvent_t fork = nullptr, join[SQP_MAX_PARTS - 1] = {};
    int parts = 1;   // 1 .. SQP_MAX_PARTS
    int fused = 0;   // 1: the whole SQP loop in one launch (sqp_loop_kernel; small batches, nlp_mode 0)
};
// ev (optional): 2*sqp_iters + 3 events recorded on `stream` at every kernel boundary
// (prologue | sort, qp_step x sqp_iters | epilogue), for per-kernel timing.  With several
// parts only ev[0], ev[1] (fork), ev[2K+1] (join) and ev[2K+2] are recorded: the SQP loop is
// timed as a whole (qsp_get_kernel_times then reports K qp_step "launches" = SQP iterations).
hipError_t launch_sqp(const SolveArgs& a, int S, hipStream_t stream, hipEvent_t* ev = nullptr,
                      const SqpStreams* split = nullptr);
// cus: compute units of the handle's device (hipDeviceProp multiProcessorCount; 256 on a whole
// MI355X, fewer on a partitioned one)
int sqp_parts_auto(int B, int N, int S, int cus);
int sqp_fused_auto(int B, int N, int S, int nlp_mode, int cus);
hipError_t launch_qp(const SolveArgs& a, int S, hipStream_t stream);   // one QP step on prepared workspace
// sim_noise drawn in the kernels (qsp_noise.hpp; helper.m:240-242, :154-156): the handle's generator
// (qsp_set_sim_noise) by value.  The noise of (lane, step) is a pure function of these words.
struct SimNoiseGen {
    int32_t on;                // 0: no generator (every other field unread)
    uint32_t stream;           // Philox counter word 3
    uint32_t key0, key1;       // seed, low and high word
    uint32_t lane0;            // lane i draws as global lane lane0 + i (lane_offset + B <= 2^32)
    uint64_t step0;            // step t of a call draws at step0 + t
    double sigma[4];
};
// Device closed loop (helper.m:195-322): buffers and logs of qsp_closed_loop, one thread per lane.
struct ClosedLoopArgs {
    const ShapeDev* shapes;
    int32_t n_shapes;
    const int32_t* sid;        // B (nullptr: shape 0)
    int32_t B, n_steps;
    double Ts;
    double* x;                 // B x 4   plant state
    double* xs;                // B x 4   state handed to the solver (after the delay prediction)
    const double* noise;       // n_steps x B x 4 (sim_noise) or nullptr
    SimNoiseGen gen;           // gen.on (then noise == nullptr): the step's noise is drawn in closed_loop_pre_kernel
    const double* lane_scale;  // B, the generator's per-lane factor of sigma, or nullptr (1)
    int32_t dist_step;         // 1-based step of the disturbance (0: none)
    const double* dist_amp;    // B amplitude_dist (nullptr: 0)
    int32_t D, Dp;             // controller delay_buff_comp, plant delay_buff_plant
    double* ubc;               // B x D x 2  u_buff_contr (column 0 = newest)
    double* ubp;               // B x Dp x 2 u_buff_plant
    const double* u0;          // B x 2   the solve's u0
    const int32_t* status;     // B
    double* Xtraj;             // B x (n_steps + 1) x 4 or nullptr (a metrics run)
    double* Xsim;              // B x n_steps x 4 or nullptr
    double* Utraj;             // B x n_steps x 2 or nullptr (a metrics run)
    int32_t* Straj;            // B x n_steps or nullptr
    // The plant's own model (qsp_set_plant_*; helper.m passes `plant` beside `controller`): the Euler
    // step, the delay prediction and the disturbance re-projection read lane i's shape from this table
    // and c, mu from the overrides.  All nullable: no table -> the controller's shape (shapes / sid
    // above), no override -> the plant shape's own constant.
    const ShapeDev* pshapes;
    int32_t n_pshapes;
    const int32_t* psid;       // B ids into pshapes (nullptr: plant shape 0); clamped
    const double* pmu;         // B mu_sp of the plant or nullptr
    const double* pc;          // B c_ellipse of the plant or nullptr
    // Per-lane metrics of the run (qsp_closed_loop_metrics), accumulated by plant_kernel; with them
    // Xtraj and Utraj may be nullptr (nothing of size B x n_steps is kept)
    double* metrics;           // B x QSP_CL_NMETRICS or nullptr
    const double* mtraj;       // the reference table as installed: T x 6, or B x T x 6 (mper_lane)
    int32_t mT, mper_lane;
    const int32_t* index0;     // B, 1-based column of step 1
    double s_lo, s_hi;         // the handle's lh[0], uh[0]
};
constexpr int CL_NMETRICS = 10;   // QSP_CL_NMETRICS (include/qsp_nmpc.h), columns QSP_CLM_*
hipError_t launch_closed_loop_pre(const ClosedLoopArgs& a, int t, hipStream_t stream);
hipError_t launch_plant(const ClosedLoopArgs& a, int t, hipStream_t stream);
hipError_t launch_delay_sim(const ClosedLoopArgs& a, hipStream_t stream);   // x -> xs (delay_buffer_sim)
// the table the loops would draw with g: noise[(t * B + i) * 4 + c], t < n_steps (qsp_gen_sim_noise)
hipError_t launch_sim_noise(const SimNoiseGen& g, const double* lane_scale, int B, int n_steps, double* noise,
                            hipStream_t stream);
hipError_t launch_reproject(const ShapeDev* shapes, int n_shapes, const int32_t* sid, int n, const double* px,
                            const double* py, const double* s0, double* s, hipStream_t stream);
hipError_t launch_straight_lines(int B, int T, const double* x0, const double* xf, double t0, double tf, double Ts,
                                 int auto_angle, double* traj, hipStream_t stream);
// Waypoint paths per lane (qsp_gen_waypoints): what the host prepared, O(B K), for the fill of B x T rows.
struct WaypointArgs {
    int32_t B, T, K;           // lanes, rows of the table (max T_lane), waypoint slots per lane
    int32_t law;               // QSP_WP_LAW_*
    double Ts;
    const double* wp;          // B x K x 2
    const int32_t* n_wp;       // B waypoints in use, 2..K
    const double* knot;        // B x K   constant speed: arrival time of waypoint k (strictly increasing)
    const int32_t* brk;        // B x K   segment linspace: rows before segment k's first, after row 0
    const double* yaw;         // B x K   yaw of segment k's rows (K - 1 used)
    const double* s_ref;       // B or nullptr (0)
    const int32_t* T_lane;     // B rows of lane i, 1..T; rows T_lane..T-1 repeat row T_lane - 1
    double* traj;              // B x T x 6
};
hipError_t launch_waypoints(const WaypointArgs& a, hipStream_t stream);
// y_ref, y_ref_e of the controller step at index_time + offset, from the T x 6 (per_lane: B x T x 6) table
hipError_t launch_stage_yref(const double* traj, int T, int per_lane, const int32_t* index_time, int offset, int D,
                             int B, int N, double* yref, double* yref_e, hipStream_t stream);
hipError_t launch_spline(const ShapeDev* shapes, const int32_t* sid, int n, const double* s, double* C, double* D,
                         double* Dd, double* kappa, hipStream_t stream);
hipError_t launch_dynamics(const ShapeDev* shapes, const int32_t* sid, int n, const double* x, const double* u,
                           double* f, double* J, hipStream_t stream);
hipError_t launch_rk4(const ShapeDev* shapes, const int32_t* sid, int n, double h, const double* x, const double* u,
                      double* xn, double* A, double* B, hipStream_t stream);
hipError_t launch_vbound(const ShapeDev* shapes, const int32_t* sid, int n, CtrlParams cp, const double* s, double* vb,
                         hipStream_t stream);

// Rollout costs and the u0 cost landscape (qsp_rollout.hip; helper.m:356-431): candidate control
// trajectories rolled out from x0 with the OCP's f, one thread per (lane, candidate).
struct RolloutArgs {
    int32_t N, B;
    int32_t integrator;        // QSP_ROLLOUT_EULER / QSP_ROLLOUT_RK4
    int32_t s0_bound;          // 1: the s bound of h also counts at stage 0 (viol)
    double Ts, tau;            // step; stage-cost scaling (the handle's tau, or 1 with cost_scale = 0)
    double W[6], We[4], lh[3], uh[3];
    const ShapeDev* shapes;
    int32_t n_shapes;
    const int32_t* shape_id;   // B (nullptr: shape 0); clamped into [0, n_shapes)
    const double* x0;          // B x 4
    const double* yref;        // B x N x 6
    const double* yref_e;      // B x 4
    // rollout_cost_kernel
    int32_t M;                 // candidates per lane
    const double* U;           // B x M x N x 2
    double* cost;              // B x M; landscape: B x n_un x n_ut or nullptr
    double* viol;              // B x M or nullptr
    double* x_end;             // B x M x 4 or nullptr
    // cost_landscape_kernel
    const double* U_tail;      // B x N x 2, row 0 ignored
    int32_t n_un, n_ut;
    const double* un_grid;     // n_un
    const double* ut_grid;     // n_ut
    double* u_min;             // B x 2
    double* cost_min;          // B
    int32_t* idx_min;          // B or nullptr
};
hipError_t launch_rollout_cost(const RolloutArgs& a, hipStream_t stream);
hipError_t launch_cost_landscape(const RolloutArgs& a, hipStream_t stream);

// Contact modes and the open-loop simulation (qsp_openloop.hip; helper.m:132-193).
// modes_kernel: entry e of n belongs to group e / per (its shape: sid[group], clamped) and reads
// x[(group * xper + e % per) * 4 ..], u[e * 2 ..] -- per = xper = 1 for a list of points, per = N and
// xper = N + 1 for a handle's trajectories.
hipError_t launch_modes(const ShapeDev* shapes, int n_shapes, const int32_t* sid, long long n, int per, int xper,
                        const double* x, const double* u, int32_t* mode, double* cone, hipStream_t stream);
struct OpenLoopArgs {
    int32_t B, M, T;
    int32_t u_steps;           // 1 or T
    int32_t D;                 // plant delay columns
    int32_t clip;
    int32_t tile;              // 0: the launcher's choice; 1: direct stores; 4 / 8: steps per thread collected in LDS
    double Ts, v_alpha;
    const ShapeDev* shapes;
    int32_t n_shapes;
    const int32_t* shape_id;   // B (nullptr: shape 0); clamped into [0, n_shapes)
    const double* x0;          // B x 4
    const double* U;           // B x M x u_steps x 2
    const double* noise;       // T x B x 4 or nullptr
    double* ring;              // D x (B M): the clipped u_t of the last D steps (clip && D > 0; else unused)
    double* X;                 // B x M x (T+1) x 4 or nullptr
    double* U_out;             // B x M x T x 2 or nullptr
    double* S_p;               // B x M x T x 2 or nullptr
    int32_t* mode;             // B x M x T or nullptr
    int32_t* mode_steps;       // B x M x 4 or nullptr
    double* x_end;             // B x M x 4
    // last, so that the kernels without a generator read the block above where they always did
    SimNoiseGen gen;           // gen.on (then noise == nullptr): the step's noise is drawn in open_loop_noise_kernel
    const double* lane_scale;  // B, the generator's per-lane factor of sigma, or nullptr (1)
};
hipError_t launch_open_loop(const OpenLoopArgs& a, hipStream_t stream);

// KKT residuals recomputed from given numbers (qsp_kkt.hip, qsp_kkt.hpp): one thread per (lane, stage).  The
// inputs of an NLP point are a PointIn (qsp_point.hpp), as the sensitivities' below.
struct KktNlpArgs {
    SolveParams p;             // the handle's: N, Ts, tau, W, We, lh, uh, s0_bound are read
    int32_t B;
    PointIn pt;                // x0 nullptr: X's row 0 is the initial state; LAM nullptr: implied multipliers
    double* res;               // B x 4      stat, eq, ineq, comp
    double* parts;             // B x 7 or nullptr (KktPart)
    double* stage_res;         // B x (N+1) x 4 or nullptr
};
hipError_t launch_kkt_nlp(const KktNlpArgs& a, hipStream_t stream);
struct KktQpArgs {
    int32_t N, nb;
    int32_t s0_bound;          // 1: the stage-0 s row counts in infeas, comp and dual
    const double* A;           // nb x N x 16
    const double* B;           // nb x N x 8
    const double* b;           // nb x N x 4
    const double* H;           // nb x (6N+4)
    const double* g;           // nb x (6N+4)
    const double* lo;          // nb x N x 3
    const double* hi;          // nb x N x 3
    PointIn pt;                // the QP point dx0, dx, du, pi, lam as x0, X, U, PI, LAM (all given); the rest unset
    double* res;               // nb x 6     stat_u, stat_x, dyn, infeas, comp, dual (KktQpRes)
};
hipError_t launch_kkt_qp(const KktQpArgs& a, hipStream_t stream);

// Solution sensitivities du_k/dx_0 (qsp_sens.hip, qsp_sens.hpp).  The workspace of the NLP entry is stage- and
// field-major with the lane fastest: field f of stage k < N of lane i at (k * SF_COUNT + f) * B + i, so that
// the walk (one thread per lane) loads consecutive addresses across a wave.  wK, the gains kept for the
// forward pass, has the same order with 8 fields.
enum SensField : int { SF_A = 0, SF_B = 6, SF_HX = 14, SF_HU = 18, SF_COUNT = 20 };
constexpr int SENS_NK = 8;
struct SensOut {
    double* K0;                // B x 2 x 4
    double* K;                 // B x N x 2 x 4 or nullptr
    double* dU;                // B x N x 2 x 4 or nullptr (nullptr: no forward pass)
    double* P0;                // B x 10 or nullptr (sidx order)
    int32_t* flag;             // B or nullptr (1: the lane is non-finite, all its outputs NaN)
};
struct SensNlpArgs {
    SolveParams p;             // the handle's: N, Ts, tau, W, We, lh, uh are read
    int32_t B;
    int32_t s0_bound;          // 1: the s pair of stage 0 counts in the barrier
    double t_floor;            // > 0
    PointIn pt;                // x0 given: stands for X's row 0; LAM nullptr: the implied multipliers from PI and
                               // yref, or zero where PI is nullptr too; yref_e is not read
    double* ws;                // SF_COUNT x N x B
    double* wK;                // SENS_NK x N x B, used with out.dU only
    SensOut out;
};
hipError_t launch_sens_nlp(const SensNlpArgs& a, hipStream_t stream);   // sens_lin_kernel, then sens_walk_kernel
struct SensQpArgs {
    int32_t N, nb;
    const double* A;           // nb x N x 16, the pusher-slider structure (checked by the entry)
    const double* B;           // nb x N x 8
    const double* H;           // nb x (6N+4), barrier in it
    double* wK;                // SENS_NK x N x nb, used with out.dU only
    SensOut out;
};
hipError_t launch_sens_qp(const SensQpArgs& a, hipStream_t stream);     // sens_walk_kernel on caller data

}  // namespace qsp
