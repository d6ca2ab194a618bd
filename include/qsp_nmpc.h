/*
 * qsp_nmpc.h — C ABI of the MI355X batched pusher–slider NMPC solver.
 *
 * Drop-in boundary for the reference's solver backend: the acados MATLAB object
 * `ocp_solver = acados_ocp(ocp_model, ocp_opts)` created in
 * acados_nmpc/NMPC_controller.m:302-305 and driven through `.set/.solve/.get`
 * (NMPC_controller.m:154-157, 170, 334-348, 382-394, 403, 420; helper.m:253, 264-269).
 * One handle replaces B independent acados solver objects: every per-lane array is
 * batched along a leading dimension B.  MATLAB column-major per-lane arrays
 * (4 x (N+1), 2 x N, 4 x N) are exactly the row-major (N+1) x 4 / N x 2 / N x 4 blocks
 * used here, so they pass through unchanged.
 *
 * Conventions
 *   ownership : the caller owns host buffers; the handle owns device memory.
 *   errors    : every entry point returns QSP_OK (0) or a negative QSP_ERR_*;
 *               qsp_last_error() gives the message (thread-local).  Numerical
 *               failure is NOT an error: it is the per-lane status (as acados 'status').
 *   threading : one handle per host thread; a handle owns one HIP stream on one device.
 *   precision : FP64 throughout.
 *   versions  : qsp_version() is QSP_ABI_VERSION of the library.  Callers compiled against
 *               this header check it before anything else; qsp_options and qsp_shape carry
 *               their own size in struct_size (set by qsp_default_options / qsp_shape_from_ply,
 *               or by the caller), which qsp_create and qsp_set_shapes reject when it differs
 *               from the library's sizeof, so a stale layout fails loudly instead of being
 *               read at the wrong offsets.
 */
#ifndef QSP_NMPC_H
#define QSP_NMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSP_NX 4          /* x = [x, y, theta, s]   (PusherSliderModel.m:519) */
#define QSP_NU 2          /* u = [u_n, u_t]         (PusherSliderModel.m:520) */
#define QSP_NY 6
#define QSP_NY_E 4
#define QSP_NH 3          /* h = [s; u_n; u_t]      (NMPC_controller.m:237) */
#define QSP_MAX_CTRL 64   /* spline control points per shape */
#define QSP_ABI_VERSION 9 /* 2: struct_size fields, qp_mu_max, qsp_get_qp_stalled, QP-failure exits;
                             3: qsp_options.factor_scan; 4: qsp_get_factor_walk;
                             5: qsp_rollout_cost, qsp_rollout_cost_device, qsp_cost_landscape;
                             6: qsp_eval_modes, qsp_get_modes, qsp_open_loop, qsp_open_loop_device;
                             7: qsp_set_plant_shapes, qsp_set_plant_shape_ids, qsp_set_plant_params,
                                qsp_clear_plant, qsp_get_plant, qsp_closed_loop_metrics;
                             8: qsp_default_sim_noise, qsp_set_sim_noise, qsp_clear_sim_noise, qsp_get_sim_noise,
                                qsp_gen_sim_noise;
                             9: qsp_default_waypoint_opts, qsp_gen_waypoints (and, without a new number, the
                                query qsp_get_fixed_horizon and the KKT evaluators qsp_eval_kkt,
                                qsp_eval_kkt_device, qsp_qp_residuals with the getter qsp_get_lam, and the
                                sensitivities qsp_default_sens_opts, qsp_eval_sens, qsp_eval_sens_device,
                                qsp_get_sens, qsp_qp_sens) */

#define QSP_OK 0
#define QSP_ERR_ARG (-1)
#define QSP_ERR_HIP (-2)
#define QSP_ERR_STATE (-3)
#define QSP_ERR_IO (-4)

/* per-lane solver status (acados meaning where one exists).
 * Precedence -- non-finite wins: a lane whose returned iterate (X, U, or the x0 it was given, all
 * four components) holds a NaN or Inf has QSP_STATUS_NAN, whatever its QP did; QSP_STATUS_QP_FAIL
 * means the returned iterate is finite and a QP was infeasible or diverged (a NaN in y_ref, or a
 * finite x0 of absurd size, ends there: the iterate stays finite, the cost may not).  sqp_iter
 * counts the completed iterations either way.  Tested, not promised beyond that: with such lanes in
 * a batch the other lanes' outputs keep the bits they have without them, at 2 to 5 instances per
 * wavefront, with the factor scan, the merit kernels, the fused and the per-iteration loop, and on
 * 8192 lanes with packing and two stream parts (tests/test_gpu_bad_lanes.py). */
#define QSP_STATUS_SUCCESS 0
#define QSP_STATUS_NAN 1
#define QSP_STATUS_MAXITER 2      /* QSP_NLP_SQP_MERIT: tolerances not met within sqp_iters */
#define QSP_STATUS_QP_FAIL 4      /* acados ACADOS_QP_FAILURE: an infeasible QP (stage0_s_bound with x0's s
                                     outside [lh_s, uh_s]: the instance does not iterate) or a QP whose
                                     interior point diverged (mu >= qp_mu_max or non-finite): the SQP
                                     stops there with its last iterate */

#define QSP_NLP_SQP_RTI_FIXED 0   /* K full Gauss-Newton steps: the BASELINE metric */
#define QSP_NLP_SQP_MERIT 1       /* acados 'SQP' + 'merit_backtracking' with KKT tolerances
                                     (NMPC_controller.m:271-276); sqp_iters = max_iter */

typedef struct qsp_solver qsp_solver;

/* Solver options: NMPC_controller.m:270-300 (create_ocp_opts) + dims. */
typedef struct {
    int32_t struct_size;      /* sizeof(qsp_options) (qsp_default_options sets it)      */
    int32_t N;                /* horizon, param_scheme_N (NMPC_controller.m:281)        */
    int32_t batch;            /* number of lanes B                                      */
    int32_t nlp_mode;         /* QSP_NLP_*                                              */
    int32_t sqp_iters;        /* K (fixed-K mode)                                       */
    int32_t qp_iters;         /* max interior-point iterations per QP                   */
    int32_t stages_per_lane;  /* S in the kernel's lane layout (0 = auto)               */
    int32_t device;           /* HIP device ordinal                                     */
    int32_t cost_scale_Ts;    /* 1: stage cost scaled by Ts as acados does             */
    double Ts;                /* sample time, T = N * Ts (NMPC_controller.m:89,221)     */
    double mu0, t_min, frac, sigma_min, mu_stop;  /* interior-point parameters         */
    /* QSP_NLP_SQP_MERIT only: tol_stat/eq/ineq/comp (NMPC_controller.m:275-276) and the
     * backtracking line search (alpha *= ls_alpha_red while alpha >= ls_alpha_min,
     * Armijo constant ls_eps on the l1 merit function) */
    double tol_stat, tol_eq, tol_ineq, tol_comp;
    double ls_alpha_min, ls_alpha_red, ls_eps;
    double res_stop;          /* interior point stops when mu < mu_stop AND the bound residual < res_stop */
    /* ... AND (HPIPM's other two exit residuals, ocp_qp_ipm res_g / res_b) the stationarity and
     * equality residuals of the IPM iterate are below these (tracked exactly: each Newton step
     * scales them by 1 - alpha); qp_iters caps it (default 20: acados' qp_solver_iter_max 50 is
     * selectable; measured no change in the SQP's rounding sensitivity, 2.3x slower at B = 4 096) */
    double qp_tol_stat, qp_tol_eq;
    int32_t stage0_s_bound;   /* 1 (default): the s bound of h also applies at stage 0 (acados bgh on
                                 stages 0..N-1, NMPC_controller.m:237,251-252); 0: stages 1..N-1 */
    int32_t qp_stall_iters;   /* stall exit (generalises HPIPM's alpha_min exit): a QP whose step length
                                 stays below qp_stall_alpha for qp_stall_iters consecutive iterations is
                                 locally infeasible and stops there; its last iterate is used as at the
                                 cap (qsp_get_qp_stalled counts them); default 3 x 1e-3, 0 = off */
    double qp_stall_alpha;
    double qp_mu_max;         /* divergence exit: a QP whose complementarity mu reaches qp_mu_max (or
                                 turns non-finite) is a QP failure (status 4, the SQP stops with its last
                                 iterate) instead of overflowing to NaN; default 1e100 (mu starts at mu0 = 1:
                                 an overflow guard -- QPs whose mu grows large but finite end at the stall
                                 exit, from which the SQP recovers; measured on the bench workload) */
    int32_t factor_scan;      /* two stages per lane (S = 2: N + 1 > 32, e.g. N = 50) only.  0 (default): the
                                 Riccati factorisation walks the horizon stage by stage, as at S = 1 and in
                                 HPIPM.  1: it runs as an associative (parallel-in-time) scan of the stages'
                                 value-function elements -- configs[4] 110k -> 115k solves/s on one MI355X, but
                                 about two digits less accurate (u0 vs the extended-precision oracle: median
                                 8e-11 instead of 2e-12 after 5 SQP iterations), which the fixed-K SQP's
                                 rounding sensitivity turns into more lanes off the reference */
} qsp_options;

/* One slider shape: object_selection.m:3-42 + PusherSliderModel.m:84-132. */
typedef struct {
    int32_t n_ctrl;                     /* control points, first point repeated last   */
    int32_t struct_size;                /* sizeof(qsp_shape) (qsp_shape_from_ply sets it) */
    double ctrl[QSP_MAX_CTRL][2];       /* contour points [m]                            */
    double knots[QSP_MAX_CTRL + 4];     /* clamped cubic knot vector S (n_ctrl + 4)      */
    double b;                           /* contour length (bspline_shape.m:37)           */
    double c_ellipse;                   /* tau_max / (mu_sg m g)  (PusherSliderModel.m:55) */
    double mu_sp;                       /* pusher-slider friction                        */
    double xwidth;                      /* slider width along x (object_selection.m; the
                                           disturbance re-projection, helper.m:229)       */
} qsp_shape;

/* Device-resident I/O for qsp_solve_device (all pointers on the handle's device). */
typedef struct {
    const double* x0;        /* B x 4              'constr_x0'                 */
    const double* yref;      /* B x N x 6          'cost_y_ref' stages 0..N-1   */
    const double* yref_e;    /* B x 4              'cost_y_ref_e'               */
    const double* X_in;      /* B x (N+1) x 4      'init_x'                     */
    const double* U_in;      /* B x N x 2          'init_u'                     */
    const int32_t* shape_id; /* B (NULL: shape 0)                              */
    double* u0;              /* B x 2              get('u', 0)                  */
    double* X_out;           /* B x (N+1) x 4      get('x')                     */
    double* U_out;           /* B x N x 2          get('u')                     */
    double* PI_out;          /* B x N x 4          get('pi')                    */
    int32_t* status;         /* B                  get('status')                */
    double* cost;            /* B                  get_cost()                   */
    int32_t controller;      /* 1: NMPC_controller.solve semantics (s pre-wrap, cold/warm start,
                                tangential clip, Euler warm-start rollout, shifted X/U/PI out)    */
    int32_t pad_;
    uint8_t* warm_valid;     /* B, controller mode: 0 = cold start (set to 1 on exit); NULL = always cold */
    const double* PI_in;     /* B x N x 4  'init_pi' (NULL: zeros); read by QSP_NLP_SQP_MERIT only */
} qsp_device_io;

/* ---------------------------------------------------------------- lifecycle */
void qsp_default_options(qsp_options* opts);          /* N=20, B=1, K=50, Ts=0.05 ... */
int qsp_create(const qsp_options* opts, qsp_solver** out);   /* acados_ocp(model, opts), :304 */
int qsp_destroy(qsp_solver* s);
const char* qsp_last_error(void);
int qsp_version(void);                                 /* QSP_ABI_VERSION */
int qsp_get_layout(const qsp_solver* s, int32_t* stages_per_lane, int32_t* lanes_per_instance);
/* How the handle's QPs walk the horizon (the solver reports its own options, as acados' print does for
 * ocp_opts, NMPC_controller.m:270-300).  The choice follows N, the layout and factor_scan, and it fixes
 * the rounding order of every result: */
#define QSP_WALK_LANE 0   /* the Riccati recursion as 4x4 algebra on one lane per stage, handed lane to lane */
#define QSP_WALK_MFMA 1   /* the factorisation on the FP64 matrix cores (v_mfma_f64_4x4x4_4b_f64, one
                             instance per 16-lane block): at one stage per lane for 12 <= N <= 31, at two
                             stages per lane from N = 24 (four instances per wave or fewer).  The closed-loop forward and difference passes
                             stay lane walks (at two stages per lane: scans) */
#define QSP_WALK_SCAN 2   /* factor_scan = 1 at two stages per lane: the associative scan */
int qsp_get_factor_walk(const qsp_solver* s, int32_t* walk);
/* The horizon the handle's per-iteration QP launches are compiled for (0: they read it at run time, as every
 * launch of the fused loop and of the merit SQP does).  Today 20 at N = 20 on the matrix-core walk at one
 * stage per lane, 0 with QSP_FIXED_HORIZON=0.  Results do not depend on it. */
int qsp_get_fixed_horizon(const qsp_solver* s, int32_t* N);

/* ------------------------------------------------------------- model / OCP */
/* PLY contour -> ordered control points, knots, c_ellipse (PusherSliderModel.m:84-132, :53-55). */
int qsp_shape_from_ply(const char* ply_path, int32_t flip, double mu_sg, double mu_sp, double mass,
                       double tau_max, qsp_shape* out);
int qsp_set_shapes(qsp_solver* s, const qsp_shape* shapes, int32_t n_shapes);
int qsp_set_shape_ids(qsp_solver* s, const int32_t* shape_id /* B */);
/* 'cost_W' (stages 0..N-1, diag of blkdiag(W_x, W_u)) and 'cost_W' at stage N (W_x_e)
 * (NMPC_controller.m:153-164).  Only diagonal weights are supported. */
int qsp_set_cost_W(qsp_solver* s, const double W_diag[6], const double W_e_diag[4]);
/* 'constr_lh' / 'constr_uh' for h = [s; u_n; u_t] (NMPC_controller.m:251-252). */
int qsp_set_constr_h(qsp_solver* s, const double lh[3], const double uh[3]);
/* warm-start clip (update_tangential_velocity_bounds, NMPC_controller.m:98-100, 319-327) */
int qsp_set_ctrl_params(qsp_solver* s, double v_alpha, double d_v_bound, double t_angle0, double u_n_lb,
                        double u_t_ub);

/* ------------------------------------------------- acados-level set/solve/get */
int qsp_set_x0(qsp_solver* s, const double* x0 /* B x 4 */);                          /* 'constr_x0' */
int qsp_set_yref(qsp_solver* s, const double* yref /* B x N x 6 */, const double* yref_e /* B x 4 */);
int qsp_set_init(qsp_solver* s, const double* X /* B x (N+1) x 4 */, const double* U /* B x N x 2 */,
                 const double* PI /* B x N x 4 or NULL */);                              /* 'init_*' */
int qsp_solve(qsp_solver* s);                                                           /* .solve() */
int qsp_get_u0(qsp_solver* s, double* u0 /* B x 2 */);                                  /* get('u',0) */
/* get_x/u/pi return the last solve's trajectories; after qsp_controller_solve they are the
 * shifted warm start the controller keeps (xtraj/utraj/ptraj, NMPC_controller.m:392-399). */
int qsp_get_x(qsp_solver* s, double* X);
int qsp_get_u(qsp_solver* s, double* U);
int qsp_get_pi(qsp_solver* s, double* PI);
int qsp_get_cost(qsp_solver* s, double* cost /* B */);
int qsp_get_status(qsp_solver* s, int32_t* status /* B */);
int qsp_get_sqp_iter(qsp_solver* s, int32_t* sqp_iter /* B */);
int qsp_get_qp_iter(qsp_solver* s, int32_t* qp_iter /* B, summed over the SQP iterations */);
/* QPs of the last solve that stopped at the iteration cap qp_iters instead of meeting the stop
 * test (their last iterate is used, as HPIPM's at iter_max): B counts */
int qsp_get_qp_capped(qsp_solver* s, int32_t* capped /* B */);
/* QPs of the last solve stopped by the stall exit (qp_stall_iters steps below qp_stall_alpha;
 * their last iterate is used as at the cap): B counts */
int qsp_get_qp_stalled(qsp_solver* s, int32_t* stalled /* B */);
/* nlp_mode 1 only (else QSP_ERR_STATE): the NLP's KKT residuals of the last test each instance
 * evaluated -- acados' statistics res_stat, res_eq, res_ineq, res_comp (max norms; ocp_nlp_res of
 * the SQP with nlp_solver_tol_* at NMPC_controller.m:275-276).  For status 0 that is the test that
 * passed; for status 2 the test before the last QP (the final iterate after the max_iter-th step is
 * not re-tested); zeros for an instance that never iterated, and before the first solve.
 * Parity unpinned: the reference was run with acados v0.2.1; later acados releases re-linearise and
 * test the final iterate at max_iter, which moves both these residuals and the status 0/2 boundary
 * for an instance that converges on its last step.  No reference fixture fixes either behaviour. */
int qsp_get_residuals(qsp_solver* s, double* res /* B x 4 */);
/* acados' get('lam'), nlp_mode 1 only (else, and before any solve, QSP_ERR_STATE): the bound multipliers
 * of the last solve's final NLP iterate, per stage (s lo, s hi, u_n lo, u_n hi, u_t lo, u_t hi), stages
 * 0 .. N-1.  Never shifted: after qsp_controller_solve they pair with the unshifted iterate, not with the
 * shifted warm start that qsp_get_x/u/pi return then.  After qsp_solve_device on a caller's stream,
 * synchronise that stream first. */
int qsp_get_lam(qsp_solver* s, double* lam /* B x N x 6 */);

/* ------------------------------------------------- KKT residuals recomputed on the device
 * The optimality of ANY point, from its numbers alone, in both nlp_modes and without a previous solve: the
 * OCP's stage data are formed at (X, U) as the SQP forms them (one RK4 step with sensitivities per stage,
 * defect x+(x_k, u_k) - x_{k+1}, gradient tau W ([x_k; u_k] - yref_k), terminal W_e (x_N - yref_e)) and
 * the residuals are those of qsp_get_residuals: on a lane the merit SQP reports converged (status 0),
 * qsp_eval_kkt of qsp_get_x/u/pi/lam returns the bits of qsp_get_residuals.  Weights, bounds, tau, Ts and
 * stage0_s_bound are the handle's; shapes per lane as qsp_set_shape_ids.
 *   PI   B x N x 4, pi_k the multiplier of x_{k+1} = x+(x_k, u_k) (qsp_get_pi's);
 *   LAM  B x N x 6 as qsp_get_lam, or NULL for the IMPLIED multipliers: each bounded quantity of a stage
 *        (s_k for k >= 1, u_n, u_t) takes lam_lo = max(r, 0), lam_hi = max(-r, 0) from its stationarity r
 *        without bound multipliers (the stage-0 s pair is 0).  The stationarity of those components is
 *        then zero by construction and the optimality gap shows in res_comp; at a KKT point with strict
 *        complementarity the implied multipliers are the true ones.  This is the measure for the RTI
 *        path, which keeps no bound multipliers.
 *   x0   B x 4 or NULL.  Used as given, without the controller's s pre-wrap.  NULL: X's row 0 is taken
 *        as the initial state.
 *   yref, yref_e  NULL: the references the handle has staged (qsp_set_yref*, or the last controller
 *        step's); QSP_ERR_STATE if none ever were.
 *   res        B x 4, acados' order: res_stat = max(stat_u, stat_x, stat_term), res_eq = max(eq_dyn, eq_x0)
 *              with eq_x0 = max |x0 - X_0| (0 with x0 == NULL), res_ineq, res_comp;
 *   parts      B x QSP_KKT_NPARTS or NULL, columns QSP_KKT_*: the maxima res is formed from;
 *   stage_res  B x (N+1) x 4 or NULL: the four residuals of each stage (eq_x0 counts at stage 0), of which
 *              res is the maximum over the stages, bit for bit.
 * A lane for which any value read is not finite (X, U, PI, LAM, its references, x0 where given; or whose
 * RK4 step is not) returns NaN in every output, all rows of stage_res included; every other lane keeps
 * the bits it has without that lane.  QSP_ERR_STATE without shapes; QSP_ERR_ARG for a null required
 * pointer.  After qsp_controller_solve, qsp_get_x/u/pi are the shifted warm start: evaluate them against
 * the next step's references, not as the step's answer. */
#define QSP_KKT_NPARTS 7
#define QSP_KKT_STAT_U 0      /* stationarity in u, stages 0 .. N-1 */
#define QSP_KKT_STAT_X 1      /* stationarity in x, stages 1 .. N-1 */
#define QSP_KKT_STAT_TERM 2   /* stationarity in x_N */
#define QSP_KKT_EQ_DYN 3      /* dynamics defect */
#define QSP_KKT_EQ_X0 4       /* |x0 - X_0| */
#define QSP_KKT_INEQ 5        /* bound violation */
#define QSP_KKT_COMP 6        /* complementarity |lam * slack| */
int qsp_eval_kkt(qsp_solver* s, const double* x0 /* B x 4 or NULL */, const double* X, const double* U,
                 const double* PI, const double* LAM /* B x N x 6 or NULL */, const double* yref,
                 const double* yref_e /* NULL: the handle's staged ones */, double* res /* B x 4 */,
                 double* parts /* B x 7 or NULL */, double* stage_res /* B x (N+1) x 4 or NULL */);
/* The same on caller-owned device memory, asynchronous on hip_stream (NULL: the handle's), as
 * qsp_rollout_cost_device: x0, LAM, yref, yref_e, parts, stage_res NULL as above; shape_id NULL = the
 * handle's. */
typedef struct {
    const double* x0;        /* B x 4 or NULL */
    const double* X;         /* B x (N+1) x 4 */
    const double* U;         /* B x N x 2 */
    const double* PI;        /* B x N x 4 */
    const double* LAM;       /* B x N x 6 or NULL */
    const double* yref;      /* B x N x 6 or NULL */
    const double* yref_e;    /* B x 4 or NULL */
    const int32_t* shape_id; /* B or NULL */
    double* res;             /* B x 4 */
    double* parts;           /* B x QSP_KKT_NPARTS or NULL */
    double* stage_res;       /* B x (N+1) x 4 or NULL */
} qsp_kkt_io;
int qsp_eval_kkt_device(qsp_solver* s, const qsp_kkt_io* io, void* hip_stream);

/* ------------------------------------------------- solution sensitivities du_k/dx0 on the device
 * How the optimal inputs move when the measured state moves: the first-order sensitivities dU_k = du_k/dx0
 * (2 x 4 each, row-major) of ANY point (X, U), in both nlp_modes and without a previous solve.  The stage-0
 * block K0 = dU_0 is the feedback gain: between two solves a faster loop applies u = u0 + K0 (x - x0).
 * Definition -- the BARRIER-SMOOTHED GAUSS-NEWTON SENSITIVITY (csrc/qsp_sens.hpp):
 *   stage data  A_k, B_k from one RK4 step with sensitivities at (x_k, u_k), as qsp_eval_kkt forms them;
 *   Hessian     Hx = tau W[0..3], Hu = tau W[4..5] for k < N, W_e at N (the exact Gauss-Newton Hessian of the
 *               least-squares cost);
 *   bounds      each of the six bound sides of h = [s; u_n; u_t] at stage k adds lam / max(slack, t_floor) to
 *               that component's diagonal entry, slack = v - lh or uh - v; the stage-0 s pair only with
 *               s0_bound.  An inactive bound (lam = 0) adds nothing, an active one lam / t_floor, which pins the
 *               component; as t_floor -> 0 under strict complementarity this tends to the exact active-set
 *               sensitivity, and it is what the interior point's last factorisation holds;
 *   backward    P_N = diag(W_e), then the solver's own Riccati step for k = N-1 .. 0: the stage gains K_k
 *               (du_k = K_k dx_k) and P_0, the Hessian of the optimal value in dx0;
 *   forward     only when dU is asked for: Phi_0 = I, dU_k = K_k Phi_k, Phi_{k+1} = (A_k + B_k K_k) Phi_k.
 * It is the sensitivity of the Gauss-Newton QP at the point, not of the exact-Hessian NLP.  Parity against
 * acados' solution sensitivities is unpinned, as everywhere: no reference fixture fixes them.
 * Accuracy (measured against a dense KKT solve on data of order one, tests/test_sens_host.py): with input
 * bounds pinned alone, by weights up to 1e10, the gains hold to a few eps relative.  A pinned s carries its
 * weight d = lam / t_floor through the Riccati recursion, which cancels it twice (the limit qsp_qp_solve's
 * header describes): K0 was off by 4e-6 relative at d = 4e7 and by 0.4 at d = 7e9 in mid-horizon.  The OCP's own
 * data couple s more weakly (B = O(Ts)); where gains at an active s bound matter, raise t_floor.
 * The implied multipliers are the true ones at a KKT point; away from one the stationarity residual of an
 * interior component acts as a (spurious) barrier, so read such gains beside qsp_eval_kkt's residuals.
 *   x0   B x 4 or NULL.  Given, it stands for X's row 0 as the point of stage 0 (used as given, without the
 *        controller's s pre-wrap).
 *   PI, LAM  LAM: B x N x 6 as qsp_get_lam.  LAM == NULL with PI: the implied multipliers of qsp_eval_kkt,
 *        formed against the references the handle has staged (QSP_ERR_STATE if none ever were).  Both NULL:
 *        zero multipliers, the unconstrained LQR gains.
 *   K0   B x 2 x 4;  K  B x N x 2 x 4 or NULL (the stage gains);  dU  B x N x 2 x 4 or NULL;
 *   P0   B x 10 or NULL, the upper triangle by rows: (0,0)(0,1)(0,2)(0,3)(1,1)(1,2)(1,3)(2,2)(2,3)(3,3);
 *   flag B (int32) or NULL.
 * A lane where any value read (every row of X, U and of the multipliers given; x0; the references with implied
 * multipliers), any linearisation or any 1/det is not finite gets NaN in every output and 1 in flag; every
 * other lane gets 0 and keeps the bits it has without that lane.  A NULL optional output is not written.
 * QSP_ERR_STATE without shapes; QSP_ERR_ARG for a null required pointer (X, U, K0), an opts of another
 * struct_size, t_floor <= 0 or not finite, s0_bound outside -1, 0, 1.  opts == NULL: the defaults.  The
 * handle owns the workspace of these calls (allocated on first use): calls on one handle must not overlap. */
typedef struct {
    int32_t struct_size;     /* sizeof(qsp_sens_opts) */
    int32_t s0_bound;        /* -1 (default): the handle's stage0_s_bound; 0 / 1: that value for this call */
    double t_floor;          /* smallest slack a multiplier is divided by; default 1e-8 */
} qsp_sens_opts;
void qsp_default_sens_opts(qsp_sens_opts* o);
int qsp_eval_sens(qsp_solver* s, const qsp_sens_opts* opts, const double* x0 /* B x 4 or NULL */, const double* X,
                  const double* U, const double* PI /* or NULL */, const double* LAM /* or NULL */,
                  double* K0 /* B x 2 x 4 */, double* K /* B x N x 2 x 4 or NULL */,
                  double* dU /* B x N x 2 x 4 or NULL */, double* P0 /* B x 10 or NULL */, int32_t* flag /* B or NULL */);
/* The same on caller-owned device memory, asynchronous on hip_stream (NULL: the handle's), no copies and no
 * synchronisation; yref NULL = the handle's staged references, shape_id NULL = the handle's. */
typedef struct {
    const double* x0;        /* B x 4 or NULL */
    const double* X;         /* B x (N+1) x 4 */
    const double* U;         /* B x N x 2 */
    const double* PI;        /* B x N x 4 or NULL */
    const double* LAM;       /* B x N x 6 or NULL */
    const double* yref;      /* B x N x 6 or NULL */
    const int32_t* shape_id; /* B or NULL */
    double* K0;              /* B x 2 x 4 */
    double* K;               /* B x N x 2 x 4 or NULL */
    double* dU;              /* B x N x 2 x 4 or NULL */
    double* P0;              /* B x 10 or NULL */
    int32_t* flag;           /* B or NULL */
} qsp_sens_io;
int qsp_eval_sens_device(qsp_solver* s, const qsp_sens_opts* opts, const qsp_sens_io* io, void* hip_stream);
/* The same computation at the last solve's final, unshifted iterate (after qsp_solve the bits of
 * qsp_get_x/u): with its bound multipliers (qsp_get_lam) in nlp_mode 1, with the implied ones from qsp_get_pi
 * and the staged references in nlp_mode 0.  QSP_ERR_STATE before any solve.  After qsp_controller_solve the
 * iterate and, in nlp_mode 1, its bound multipliers are still the step's own (never shifted), so nlp_mode 1
 * answers there too; in nlp_mode 0 the epilogue keeps the dynamics multipliers only shifted by one stage
 * (pi_0 is gone), the implied multipliers cannot be formed, and the call returns QSP_ERR_STATE.  After
 * qsp_solve_device on a caller's stream, synchronise that stream first. */
int qsp_get_sens(qsp_solver* s, const qsp_sens_opts* opts, double* K0, double* K, double* dU, double* P0, int32_t* flag);
/* The linear algebra alone, on caller-given QP data of nb lanes and horizon N (any N >= 1, not the handle's):
 * A nb x N x 16, B nb x N x 8 and the diagonal Hessian H nb x (6N+4) of qsp_qp_solve's layout, with the
 * barrier terms already in H (H may differ per stage and lane).  A must have the structure qsp_qp_solve
 * asks for (the identity except a02, a03, a12, a13, a23, a33), else QSP_ERR_ARG.  Outputs, flag and lane
 * isolation as above. */
int qsp_qp_sens(qsp_solver* s, int32_t nb, int32_t N, const double* A, const double* B, const double* H, double* K0,
                double* K, double* dU, double* P0, int32_t* flag);
int qsp_get_time_tot(qsp_solver* s, double* ms);                                        /* 'time_tot' */
/* dims of the handle (outputs of a MEX/FFI layer are sized from these, never from caller input) */
int qsp_get_dims(const qsp_solver* s, int32_t* N, int32_t* B);
/* the acados field-by-field setters: set('cost_y_ref', y, k) for one stage k in 0..N-1 (B x 6),
 * set('cost_y_ref_e', y_e, N) (B x 4), set('init_x'/'init_u'/'init_pi') one at a time */
int qsp_set_yref_stage(qsp_solver* s, int32_t stage, const double* y /* B x 6 */);
int qsp_set_yref_e(qsp_solver* s, const double* y_e /* B x 4 */);
int qsp_set_init_x(qsp_solver* s, const double* X /* B x (N+1) x 4 */);
int qsp_set_init_u(qsp_solver* s, const double* U /* B x N x 2 */);
int qsp_set_init_pi(qsp_solver* s, const double* PI /* B x N x 4 */);
/* acados get('time_tot'/'time_lin'/'time_qp_sol') in seconds (helper.m:264-269): with qsp_set_timing(s, 1)
 * every solve records HIP events at its kernel boundaries and qsp_get_timings reports the last solve
 * (time_lin = the separate linearisation / packing-sort kernels, time_qp_sol = the QP kernels, which in
 * nlp_mode 0 include the fused linearisation); without it time_lin / time_qp_sol are NaN. */
int qsp_set_timing(qsp_solver* s, int32_t on);
int qsp_get_timings(qsp_solver* s, double* time_tot, double* time_lin, double* time_qp_sol);

/* --------------------------------------- NMPC_controller.solve(x0, index_time) */
/* reference table y_ref (6 x T, MATLAB column-major == T x 6 row-major), shared by all lanes
 * (set_reference_trajectory, NMPC_controller.m:425-431 with delay_buff_comp = 0) */
int qsp_set_reference_trajectory(qsp_solver* s, const double* traj /* T x 6 */, int32_t T);
/* one reference table per lane: traj B x T x 6 (scenario sweeps; same staging rule) */
int qsp_set_reference_trajectories(qsp_solver* s, const double* traj /* B x T x 6 */, int32_t T);
/* per-lane TrajectoryGenerator.straight_line generated on the device (TrajectoryGenerator.m:39-79):
 * x0, xf: B x 3 (x, y, theta); samples t0:Ts:tf; rows [x y theta 0 0 0] (main.m:165-178).
 * Installs the tables as with qsp_set_reference_trajectories; T_out (optional) = samples. */
int qsp_gen_straight_lines(qsp_solver* s, const double* x0, const double* xf, double t0, double tf,
                           int32_t auto_angle, int32_t* T_out);
/* per-lane waypoint paths generated on the device: TrajectoryGenerator.waypoints_gen
 * (TrajectoryGenerator.m:96-143) and waypoint_gen_fixed_angle (:81-95), one polyline of n_wp[i] waypoints
 * per lane.  The one deviation from the reference is trajectory.py's: MATLAB's waypointTrajectory (:121) is
 * replaced by the constant-speed polyline through the waypoints, exact for two waypoints (main.m:150-164).
 * Rows [x y yaw s_ref 0 0]; the table is B x T x 6 with T = max_i T_i, and a lane with T_i < T repeats its
 * last row up to T, which is what get_y_ref's clamp at the end reads anyway (NMPC_controller.m:307-313).
 * Time laws, with len_k = sqrt(dx*dx + dy*dy) and d_k = len_k / vel_k of segment k:
 *   QSP_WP_LAW_CONSTANT_SPEED    arrival times t_0 = 0, t_{k+1} = t_k + d_k; T_i = floor(t_end/Ts + 1e-9) + 1
 *                                samples at t = j*Ts (the colon rule of qsp_gen_straight_lines); sample j lies
 *                                on the last segment k with t_k <= t (capped at the last one) at
 *                                wp_k + a*(wp_{k+1} - wp_k), a = (t - t_k)/(t_{k+1} - t_k)
 *   QSP_WP_LAW_SEGMENT_LINSPACE  row 0 is wp_0; segment k adds n_k = floor(d_k/Ts + 1e-9) rows, the count of
 *                                (a+Ts):Ts:(a+d_k) (:88), which are linspace(wp_k, wp_{k+1}, n_k) (:90-91):
 *                                wp_k + m*((wp_{k+1} - wp_k)/(n_k - 1)), the last one (and the only one of
 *                                n_k = 1) wp_{k+1} itself; n_k = 0 adds none.  T_i = 1 + sum n_k
 * Yaw of a row: the heading h_k = atan2(dy, dx) of its segment (row 0 of the linspace law: segment 0's),
 * raw, or unwrapped along the path (y_0 = h_0, y_k = y_{k-1} + d with d = h_k - h_{k-1} reduced by
 * 2 pi rint(d / (2 pi))), or theta[i] on every row (x0(3) of :86,92).
 * QSP_ERR_ARG, with the installed table left as it is: struct_size, law or yaw out of range; K outside
 * 2..QSP_MAX_WAYPOINTS; an n_wp outside 2..K; a waypoint, theta or s_ref that is not finite; a vel that is
 * not finite and > 0; under constant speed two consecutive waypoints that are equal (or so close that the
 * arrival time does not advance); QSP_WP_YAW_FIXED without theta; a segment duration that overflows; a path
 * of more than 2^24 samples.
 * Installs the tables as with qsp_set_reference_trajectories.  All arrays are host arrays. */
#define QSP_MAX_WAYPOINTS 16
#define QSP_WP_LAW_CONSTANT_SPEED 0   /* waypoints_gen, TrajectoryGenerator.m:96-143, as trajectory.py restates it */
#define QSP_WP_LAW_SEGMENT_LINSPACE 1 /* waypoint_gen_fixed_angle, :81-95 */
#define QSP_WP_YAW_HEADING 0          /* atan2 of the segment, raw */
#define QSP_WP_YAW_HEADING_UNWRAPPED 1
#define QSP_WP_YAW_FIXED 2            /* theta[i] on every row (x0(3) of :86,92) */
typedef struct {
    int32_t struct_size;      /* sizeof(qsp_waypoint_opts) (qsp_default_waypoint_opts sets it; checked as qsp_options') */
    int32_t law;              /* QSP_WP_LAW_* */
    int32_t yaw;              /* QSP_WP_YAW_* */
    int32_t pad_;
} qsp_waypoint_opts;
void qsp_default_waypoint_opts(qsp_waypoint_opts* opts);   /* constant speed, heading */
int qsp_gen_waypoints(qsp_solver* s, const qsp_waypoint_opts* opts, int32_t K,
                      const double* wp      /* B x K x 2; lane i reads its first n_wp[i] rows */,
                      const int32_t* n_wp   /* B, 2..K; NULL: K everywhere */,
                      const double* vel     /* B x (K-1), per segment */,
                      const double* theta   /* B, QSP_WP_YAW_FIXED only, else NULL */,
                      const double* s_ref   /* B or NULL (0): column 3 of every row, traj row 4 of :92,:140 */,
                      int32_t* T_out /* or NULL */, int32_t* T_lane /* B or NULL */);
/* copy of the installed table(s): T x 6 (shared) or B x T x 6 (per lane) */
int qsp_get_reference_trajectories(qsp_solver* s, double* traj);
/* x0: B x 4, index_time: B (1-based, as MATLAB).  Warm start lives on the device and is
 * shifted after every call; u0 is available through qsp_get_u0. */
int qsp_controller_solve(qsp_solver* s, const double* x0, const int32_t* index_time);
int qsp_controller_reset(qsp_solver* s);                                                 /* clear_variables */
/* Closed-loop simulation on the device (helper.m:195-322, closed_loop_matlab): cold start of the
 * solver's warm start (X, U, PI), then for t = 0..n_steps-1: x += noise[t] (sim_noise, optional), u = solve(x, index0 + t),
 * x += Ts * f(x, u) (evalModelVariableShape + Euler, :292-307).  x0: B x 4; index0: B (1-based);
 * noise: n_steps x B x 4 or NULL (NULL with a generator installed, qsp_set_sim_noise below: drawn on the
 * device); X_traj: B x (n_steps+1) x 4; U_traj: B x n_steps x 2;
 * status_traj: B x n_steps (found_sol = status == 0) or NULL. */
int qsp_closed_loop(qsp_solver* s, const double* x0, const int32_t* index0, int32_t n_steps, const double* noise,
                    double* X_traj, double* U_traj, int32_t* status_traj);
/* closed_loop_matlab's other branches (helper.m:195-322) */
typedef struct {
    double plant_delay;        /* plant.time_delay [s]: the plant applies u delayed by ceil(delay/Ts) steps
                                  (u_buff_plant, helper.m:211-212, 289-296) */
    int32_t disturbance;       /* disturbance_: at step t_dist (1-based) y += amplitude and the contact
                                  point is re-projected onto the contour (helper.m:221-236) */
    int32_t t_dist;
    const double* amplitude;   /* B amplitude_dist per lane (NULL: 0) */
} qsp_closed_loop_opts;
/* Per step i: disturbance (i == t_dist), noise, the controller's delay prediction (delay_buffer_sim
 * with the handle's delay compensation), u = solve(x_sim, index0 + i - 1 + delay_buff_comp), the
 * controller buffer push, the (delayed) plant step.  X_traj: the plant states after disturbance and
 * noise (B x (n+1) x 4); X_sim (optional): the states handed to the solver (B x n x 4).
 * State carried between calls: the controller's input buffer u_buff_contr is the controller
 * object's (NMPC_controller.m:109), as in helper.m, where it persists across closed_loop_matlab
 * calls: it is NOT reset here (a second closed loop on the same handle starts from the buffer the
 * first one left); only qsp_set_delay_comp zeroes it.  The plant's buffer u_buff_plant is local
 * to one call (helper.m:211-212) and starts at zero.  Both closed-loop entry points behave so. */
int qsp_closed_loop_ex(qsp_solver* s, const qsp_closed_loop_opts* opts, const double* x0, const int32_t* index0,
                       int32_t n_steps, const double* noise, double* X_traj, double* X_sim, double* U_traj,
                       int32_t* status_traj);
/* A plant model of its own.  closed_loop_matlab(plant, controller, ...) simulates with the plant's model
 * and solves with the controller's (helper.m:195-322).  After qsp_create the plant is the controller's
 * model; the entries below install another one on the handle.  Lane i's plant is a shape -- the plant
 * table's entry at the lane's plant id, or without a plant table the controller's shape of the lane --
 * with its two physical constants mu_sp and c_ellipse replaced by the lane's overrides where given.
 * With a plant installed these read it:
 *   the plant's Euler step            plant.evalModelVariableShape, helper.m:292-307
 *   the delay prediction              controller.delay_buffer_sim(plant, x), helper.m:244,
 *                                     NMPC_controller.m:112-120
 *   the disturbance re-projection     plant.SP, plant.slider_params.xwidth, helper.m:221-236 (the
 *                                     plant's contour, xwidth and b)
 *   the mode counts of qsp_closed_loop_metrics
 * The prediction runs on the plant's model, not the controller's: the reference passes `plant` into
 * delay_buffer_sim, and this is the literal reading of it.  qsp_delay_buffer_sim follows the installed
 * plant too, so it stays bit-identical to the closed loop's own prediction.
 * Everything else keeps the controller's model: NMPC_controller.solve (its warm-start rollout and clip,
 * the OCP, v_bound), qsp_get_modes, the rollout and landscape entries, qsp_open_loop.
 * With nothing installed every result is bit-identical to a library without these entries. */
/* the plant's shape table: validated and converted as qsp_set_shapes; the plant ids return to 0 */
int qsp_set_plant_shapes(qsp_solver* s, const qsp_shape* shapes, int32_t n_shapes);      /* helper.m:294-307 */
/* ids into the plant table (default 0 for every lane); QSP_ERR_STATE without a plant table */
int qsp_set_plant_shape_ids(qsp_solver* s, const int32_t* shape_id /* B */);            /* helper.m:294-307 */
/* per-lane mu_sp and c_ellipse of the plant (PusherSliderModel.m:53-55, :547-548), the Monte-Carlo path:
 * one double per lane instead of one shape per lane.  Each finite and > 0 (else QSP_ERR_ARG, and what was
 * installed stays); NULL leaves that constant to the lane's plant shape (both NULL: no overrides).  Works
 * with or without a plant table. */
int qsp_set_plant_params(qsp_solver* s, const double* mu_sp /* B or NULL */,
                         const double* c_ellipse /* B or NULL */);                       /* helper.m:294-307 */
/* back to "the plant is the controller's model" (table, ids and overrides dropped) */
int qsp_clear_plant(qsp_solver* s);
/* what is installed: has_shapes = entries of the plant table (0: none); has_params = 1 (mu_sp) | 2
 * (c_ellipse).  Either pointer may be NULL. */
int qsp_get_plant(qsp_solver* s, int32_t* has_shapes, int32_t* has_params);

/* Per-lane metrics of a closed loop without its trajectories: exactly qsp_closed_loop_ex's loop (same
 * arguments, same state carried), but nothing of size B x n_steps is allocated or copied; only
 * metrics (B x QSP_CL_NMETRICS), x_end (B x 4, the state after the last plant step, X_traj's last row;
 * or NULL) and status_last (B, the last solve's status; or NULL) come back.
 * e_i = the logged plant state of step i = 1..n_steps (X_traj's row i - 1: after disturbance and noise)
 * minus the lane's reference-table row at the 1-based column index0 + i - 1, clamped at the table's
 * end as get_y_ref clamps (NMPC_controller.m:307-313); the table as installed, without the delay prefix.
 * Sums run in step order with plain products and sums (e_x * e_x + e_y * e_y, then acc + that); counts
 * are exact doubles.  The modes are those of the applied input (after the plant's delay buffer) at the
 * logged state under the plant's model (QSP_MODE_*; mode 0 is counted nowhere).
 * QSP_ERR_STATE without a reference table or shapes. */
#define QSP_CL_NMETRICS 10
#define QSP_CLM_SUM_EXY2 0    /* sum_i (e_x^2 + e_y^2)                                              */
#define QSP_CLM_MAX_EXY2 1    /* max_i (e_x^2 + e_y^2); a NaN step does not enter                   */
#define QSP_CLM_SUM_ETH2 2    /* sum_i e_theta^2                                                    */
#define QSP_CLM_END_EXY2 3    /* e_x^2 + e_y^2 of the final state against column index0 + n_steps   */
#define QSP_CLM_SUM_U2 4      /* sum_i (u_n^2 + u_t^2) of the commanded input                       */
#define QSP_CLM_N_FAILED 5    /* steps with status != 0 (found_sol false, helper.m:253-260)         */
#define QSP_CLM_N_ST 6        /* steps whose applied input is sticking ...                          */
#define QSP_CLM_N_SL 7        /* ... sliding left ...                                               */
#define QSP_CLM_N_SR 8        /* ... sliding right                                                  */
#define QSP_CLM_N_S_OUT 9     /* steps with the logged s not inside the handle's [lh[0], uh[0]]     */
int qsp_closed_loop_metrics(qsp_solver* s, const qsp_closed_loop_opts* opts, const double* x0, const int32_t* index0,
                            int32_t n_steps, const double* noise, double* metrics /* B x QSP_CL_NMETRICS */,
                            double* x_end /* B x 4 or NULL */, int32_t* status_last /* B or NULL */);
/* set_delay_comp (NMPC_controller.m:106-110): delay_buff_comp = ceil(delay / Ts) columns; the
 * reference table is read as set_reference_trajectory prepends it (:425-431) and the per-lane input
 * buffer u_buff_contr is zeroed (the only call that zeroes it).  get: the column count. */
int qsp_set_delay_comp(qsp_solver* s, double delay);
int qsp_get_delay_comp(qsp_solver* s, int32_t* cols);
/* delay_buffer_sim (NMPC_controller.m:112-120): x (B x 4) advanced by delay_buff_comp Euler steps with
 * the buffered inputs, oldest first -> x_sim (B x 4); and the buffer update the caller does after a
 * solve, u_buff_contr = [u, u_buff_contr(:, 1:end-1)] (helper.m:255), u: B x 2. */
int qsp_delay_buffer_sim(qsp_solver* s, const double* x, double* x_sim);
int qsp_delay_buffer_push(qsp_solver* s, const double* u);
/* the disturbance branch's contact re-projection alone: s = argmin |C(s) - (px, py)|^2 from s0 (per
 * lane shape ids; fminunc in helper.m:230, restated as a damped Newton iteration) */
int qsp_reproject_contact(qsp_solver* s, int32_t n, const int32_t* shape_id, const double* px, const double* py,
                          const double* s0, double* s_out);

/* ------------------------------------------------ device-resident fast path */
int qsp_solve_device(qsp_solver* s, const qsp_device_io* io, void* hip_stream);
int qsp_synchronize(qsp_solver* s);
/* The SQP loop of a solve can run in two parts, each half of the lanes iterating on its own
 * HIP stream (forked from and joined back into the solve's stream), so that the tail of one
 * half's QP launch overlaps the other half's work.  Results are bit-identical either way.
 * parts: 0 = auto (two once the batch fills the GPU's wave slots), 1, or 2.  No acados
 * counterpart (an execution choice of the batched engine).  get: the count the next solve uses.
 * Batches whose waves fit the GPU's SIMDs once (nlp_mode 0) run the whole SQP loop in one launch
 * instead (one part; environment QSP_FUSED_LOOP=0/1 at qsp_create overrides the automatic choice).
 * The Riccati factorisation runs on the FP64 matrix cores at one stage per lane for 12 <= N <= 31 and at
 * two stages per lane from N = 24 (qsp_get_factor_walk reports it); environment
 * QSP_MFMA_WALK=0 at qsp_create selects the lane walk instead, a developer A/B that rounds differently
 * (the oracle twin follows the same variable).
 * At N = 20 the per-iteration QP kernel of that variant is compiled for its horizon; environment
 * QSP_FIXED_HORIZON=0 at qsp_create launches the runtime-horizon kernel instead (developer A/B, the same
 * bits). */
int qsp_set_stream_parts(qsp_solver* s, int32_t parts);
int qsp_get_stream_parts(qsp_solver* s, int32_t* parts);
/* Per-kernel timing (acados' time_lin / time_qp split).  qsp_set_kernel_timing(s, n) pre-creates
 * HIP events for the next n solves (0 disables): every kernel boundary of each solve is then
 * recorded on the solve's stream.  qsp_get_kernel_times synchronises the recorded events and
 * returns the summed milliseconds and launch counts per kernel family in the order
 * {prologue, linearize, qp_step, epilogue}, then re-arms the pool.  With nlp_mode 0 the SQP
 * iteration's linearisation runs inside the qp_step kernel, so "linearize" is only the
 * wave-packing sort before it; with nlp_mode 1 it is the separate linearisation kernel. */
int qsp_set_kernel_timing(qsp_solver* s, int32_t max_solves);
int qsp_get_kernel_times(qsp_solver* s, double* ms /* 4 */, int32_t* launches /* 4 */);

/* ------------------------------------------- building blocks (host arrays) */
int qsp_eval_spline(qsp_solver* s, int32_t n, const int32_t* shape_id, const double* sigma,
                    double* C /* n x 2 */, double* D /* n x 2 */, double* Dd /* n x 2 */, double* kappa /* n */);
int qsp_eval_dynamics(qsp_solver* s, int32_t n, const int32_t* shape_id, const double* x, const double* u,
                      double* f /* n x 4 */, double* J /* n x 4 x 6 */);
int qsp_eval_rk4(qsp_solver* s, int32_t n, const int32_t* shape_id, double h, const double* x, const double* u,
                 double* xn /* n x 4 */, double* A /* n x 4 x 4 */, double* B /* n x 4 x 2 */);
int qsp_eval_vbound(qsp_solver* s, int32_t n, const int32_t* shape_id, const double* sval, double* vb);
/* Batched LQ-QP (interior point) with per-stage data; H and bound widths must be equal on
 * every stage (as in the OCP).  H: nb x (6N+4) diag, g: nb x (6N+4), lo/hi: nb x N x 3,
 * stage-0 s bound as the handle's stage0_s_bound.  qp_status (optional, nb): 0 the stop test
 * was met, 1 non-finite solution, 2 stopped at the iteration cap, 3 infeasible (the fixed
 * stage-0 s = dx0's outside its bounds), 4 stall exit, 5 diverged (mu >= qp_mu_max).
 * Non-finite wins: a lane whose returned dx or du holds a NaN or Inf reports 1 whatever else
 * happened to it (infeasible, diverged); 3, 5 and the other codes describe finite answers only.
 * One NaN in a lane's g, A, B, b, lo, hi or dx0 therefore gives that lane 1 and leaves every other
 * lane's answer as it is without it.
 * H is one set of weights for the whole call, not per-lane data ("equal on every stage"): the ten
 * entries that are read as weights are lane 0's stage-0 entries H[0 .. 5] and lane 0's terminal
 * entries H[6 N .. 6 N + 3]; the kernels run with these (the handle's own cost weights are not
 * consulted).  Every other entry of every lane is only compared with them, and a differing one --
 * a NaN differs, also from itself, so a NaN in the ten entries too -- fails the whole call with
 * QSP_ERR_ARG before any lane is solved.  H can therefore not make a single lane non-finite.
 * A must be the identity except a02, a03, a12, a13, a23, a33 (the pusher-slider structure).
 * Accuracy (measured against QPs with known exact solutions): with no active
 * bound or active input bounds only, a status-0 answer is within 4e-9 of the solution at data of
 * order one (the stop test's truncation, mu_stop 1e-10).  The stop test tracks its residuals as
 * r0 * prod(1 - alpha) and does not recompute them, so status 0 certifies the point only while the
 * Newton steps are accurate.  An active STATE bound puts its barrier weight sigma = lam / t ~
 * lam^2 / mu into the Riccati recursion, which cancels it twice: the u-stationarity of the returned
 * point is off by ~ 3e-5 eps sigma^2 (B and bound offsets of order one, N = 20; about linear in the
 * offsets, B's scale to the power 1 .. 2), up to the multipliers' own size.  Domain at mu_stop =
 * 1e-10: state-bound multipliers lam <~ 1e-2 at such data (du then within 1e-4, mostly truncation);
 * the OCP's own QPs (B = O(Ts), offsets <= 0.07) sit lower at the same multipliers (u-stationarity
 * of 1 024 bench lanes' QPs: median 1e-13 .. 3e-7, 99th percentile 2e-3 .. 8e-3).
 * Beyond it (lam ~ 1: du wrong by up to 1) check the returned point with qsp_qp_residuals (below) before
 * trusting status 0. */
int qsp_qp_solve(qsp_solver* s, int32_t nb, const double* A, const double* B, const double* b, const double* H,
                 const double* g, const double* lo, const double* hi, const double* dx0, double* dx, double* du,
                 double* pi, double* lam, int32_t* iters, int32_t* qp_status);
/* The KKT residuals of QP points, recomputed on the device from the numbers given: same array layouts and
 * sign conventions as qsp_qp_solve (dx: nb x (N+1) x 4, du: nb x N x 2, pi: nb x N x 4, lam: nb x N x 6).
 * None of qsp_qp_solve's restrictions applies: H may differ per stage and lane, bound widths per stage, A
 * is read as a full 4 x 4; the data are read as given.  res: nb x 6, largest absolute values per lane of
 *   0 stat_u   H_u du_k + g_u + B_k' pi_k - lam_lo + lam_hi, k < N
 *   1 stat_x   H_x dx_k + g_x + A_k' pi_k - pi_{k-1} + e_s (lam_hi - lam_lo), 0 < k < N, and the terminal
 *              H_N dx_N + g_N - pi_{N-1}
 *   2 dyn      dx_{k+1} - A_k dx_k - B_k du_k - b_k, and dx_0 - dx0
 *   3 infeas   bound violation;  4 comp  |lam * slack|;  5 dual  negative multipliers
 * The stage-0 s row counts in infeas, comp and dual with the handle's stage0_s_bound = 1 and is left out of
 * all three otherwise.  A lane with a non-finite value in any array returns NaN in its six outputs; the
 * other lanes keep their bits. */
int qsp_qp_residuals(qsp_solver* s, int32_t nb, const double* A, const double* B, const double* b, const double* H,
                     const double* g, const double* lo, const double* hi, const double* dx0, const double* dx,
                     const double* du, const double* pi, const double* lam, double* res /* nb x 6 */);

/* ------------------------------------- rollout costs and the u0 cost landscape */
/* The reference's optimality probe on the device (helper.m:356-431): control trajectories are rolled out
 * from x0 with the model, the tracking cost against the references is summed
 *     cost = sum_{k<N} 0.5 tau |[x_k; u_k] - yref_k|^2_W + 0.5 |x_N - yref_e|^2_We     (helper.m:416-423)
 * with the handle's W, W_e (qsp_set_cost_W), and the largest violation of lh <= [s_k; u_n; u_t] <= uh
 * over k = 0..N-1 is tracked (qsp_set_constr_h; the s bound at stage 0 only with stage0_s_bound).
 * Two deviations from the reference, both deliberate:
 *   model      : the probe calls the fixed-shape plant.eval_model (helper.m:362,419); the library rolls out
 *                with the OCP's own f (PusherSliderModel.m:503-603), which is what evalModelVariableShape
 *                evaluates (helper.m:294) and what the solver optimises over;
 *   references : the probe reads get_y_ref(time_index + n), n = 1..Hp (helper.m:360,417), one column
 *                later than solve stages them (index_time + k, k = 0..Hp-1, NMPC_controller.m:343-346).
 *                These entry points evaluate against the references they are given (or the handle's
 *                staged ones); which columns those are is the caller's choice (helper.py stages the
 *                probe's).
 * x0 is used as given: the s pre-wrap of NMPC_controller.m:332 is the controller's, not the probe's. */
#define QSP_ROLLOUT_EULER 0   /* x+ = x + Ts f(x, u): the probe's and the plant's step (helper.m:419-420, :307) */
#define QSP_ROLLOUT_RK4 1     /* the OCP's integrator: one RK4 step of Ts (NMPC_controller.m:272), qsp_eval_rk4's xn */
typedef struct {
    int32_t struct_size;      /* sizeof(qsp_rollout_opts) (qsp_default_rollout_opts sets it; checked as qsp_options') */
    int32_t integrator;       /* QSP_ROLLOUT_* */
    int32_t cost_scale;       /* 1: the handle's objective, stage terms x tau (Ts with cost_scale_Ts), as
                                 qsp_get_cost; 0: unscaled stage terms, as helper.m:418 */
    int32_t pad_;
} qsp_rollout_opts;
void qsp_default_rollout_opts(qsp_rollout_opts* opts);   /* Euler, cost_scale 1 */
/* evaluate_cost_function (helper.m:356-367), batched: M control trajectories per lane.
 * x0: B x 4; U: B x M x N x 2; yref: B x N x 6 and yref_e: B x 4, or NULL for the references the handle
 * has staged (qsp_set_yref*, or the last qsp_controller_solve's); shapes per lane as qsp_set_shape_ids.
 * cost: B x M; viol: B x M or NULL (0 when feasible); x_end: B x M x 4 or NULL (x_N). */
int qsp_rollout_cost(qsp_solver* s, const qsp_rollout_opts* opts, int32_t M, const double* x0, const double* U,
                     const double* yref, const double* yref_e, double* cost, double* viol, double* x_end);
/* The same on caller-owned device memory, asynchronous on hip_stream (NULL: the handle's), as
 * qsp_solve_device: yref, yref_e, shape_id NULL = the handle's; viol, x_end optional. */
typedef struct {
    const double* x0;        /* B x 4 */
    const double* U;         /* B x M x N x 2 */
    const double* yref;      /* B x N x 6 or NULL */
    const double* yref_e;    /* B x 4 or NULL */
    const int32_t* shape_id; /* B or NULL */
    double* cost;            /* B x M */
    double* viol;            /* B x M or NULL */
    double* x_end;           /* B x M x 4 or NULL */
} qsp_rollout_io;
int qsp_rollout_cost_device(qsp_solver* s, const qsp_rollout_opts* opts, int32_t M, const qsp_rollout_io* io,
                            void* hip_stream);
/* debug_cost_function (helper.m:369-431): the cost of every first move u_0 = (un_grid[i], ut_grid[j]) with
 * u_k = U_tail[k], k >= 1 (u_vect(:,1) replaced, helper.m:413), and the grid minimiser (helper.m:430-431).
 * U_tail: B x N x 2, row 0 ignored; NULL: the last solve's solution before the controller's shift, what
 * ocp_solver.get('u') returns at helper.m:376 (QSP_ERR_STATE before any solve; after qsp_solve_device on
 * a caller's stream, synchronise that stream first).
 * cost: B x n_un x n_ut row-major (cost_values(j, i) of the meshgrid, helper.m:382) or NULL: then only
 * the B x 4 numbers below leave the device.  u_min: B x 2; cost_min: B; idx_min: B or NULL, the 0-based
 * linear index i n_ut + j = MATLAB's ind_raw - 1.  min as MATLAB's: the first minimum in that order,
 * NaN never wins, an all-NaN lane gives cost_min = NaN, idx_min = 0. */
int qsp_cost_landscape(qsp_solver* s, const qsp_rollout_opts* opts, const double* x0, const double* U_tail,
                       int32_t n_un, const double* un_grid, int32_t n_ut, const double* ut_grid, const double* yref,
                       const double* yref_e, double* cost, double* u_min, double* cost_min, int32_t* idx_min);
/* The same on caller-owned device memory, asynchronous on hip_stream (NULL: the handle's); NULL
 * U_tail, yref, yref_e, shape_id, cost, idx_min as above. */
typedef struct {
    const double* x0;        /* B x 4 */
    const double* U_tail;    /* B x N x 2 or NULL */
    const double* un_grid;   /* n_un */
    const double* ut_grid;   /* n_ut */
    const double* yref;      /* B x N x 6 or NULL */
    const double* yref_e;    /* B x 4 or NULL */
    const int32_t* shape_id; /* B or NULL */
    double* cost;            /* B x n_un x n_ut or NULL */
    double* u_min;           /* B x 2 */
    double* cost_min;        /* B */
    int32_t* idx_min;        /* B or NULL */
    int32_t n_un, n_ut;
} qsp_landscape_io;
int qsp_cost_landscape_device(qsp_solver* s, const qsp_rollout_opts* opts, const qsp_landscape_io* io,
                              void* hip_stream);

/* ------------------------------------- contact modes and the open-loop simulation */
/* The contact mode of (x, u): which branch of f the input selects, in helper.convert_str2num's coding,
 * taken from the OCP model's indicators (PusherSliderModel.m:587-589)
 *     ST  gamma_r <= u_t / u_n <= gamma_l      SL  u_t / u_n > gamma_l      SR  u_t / u_n < gamma_r
 * with the motion cone's edges gamma_l, gamma_r at the contact point (:547-548).  The mode and the edges
 * are bit for bit the ones qsp_eval_dynamics blends with (J[3][5] = 1 exactly when sliding, J[3][4] =
 * -gamma_l on SL and -gamma_r on SR).  They depend on s and u only.
 * QSP_MODE_NONE: no indicator is set -- u_t / u_n is NaN (u_n = u_t = 0, as a delayed plant's input buffer
 * holds at its start) or s / an input is not finite; f is 0 then.  The one deviation from the reference:
 * the numeric eval_model_variable_shape's if-chain (PusherSliderModel.m:353-362) ends in an else and would
 * label that case "SR".  Its "NC" cannot occur for a contact point given by s.  u_n = 0 with u_t != 0 is
 * an infinite ratio: SL for u_t > 0, SR for u_t < 0, as in the reference. */
#define QSP_MODE_NONE 0
#define QSP_MODE_ST 1
#define QSP_MODE_SL 2
#define QSP_MODE_SR 3
/* building block, beside qsp_eval_dynamics: cone (optional) = gamma_l, gamma_r, u_t / u_n per point */
int qsp_eval_modes(qsp_solver* s, int32_t n, const int32_t* shape_id, const double* x /* n x 4 */,
                   const double* u /* n x 2 */, int32_t* mode /* n */, double* cone /* n x 3 or NULL */);
/* Stage k's mode at (x_k, u_k), k = 0..N-1, of exactly what qsp_get_x and qsp_get_u return (after
 * qsp_controller_solve: the shifted warm start), evaluated on the device-resident trajectories with the
 * handle's shape ids.  mode: B x N; cone: B x N x 3 or NULL. */
int qsp_get_modes(qsp_solver* s, int32_t* mode, double* cone);

/* helper.open_loop_matlab (helper.m:132-193), batched over B lanes x M input candidates per lane.
 * Per step i = 0..n_steps-1, in this order:
 *   1. x += noise[i]                      (sim_noise, :155; the logged state includes it)
 *   2. clip (:162-166)                    v = v_alpha / |angle_rate(mod(s, b))|, u_t <- (v < u_t ? v : u_t):
 *                                         MATLAB's min, a NaN never wins, a negative u_t passes through
 *   3. applied input (:169-177)           u itself without a plant delay; else the delay buffer's last
 *                                         column, after which the clipped u is pushed (the buffer starts at
 *                                         zero and is local to the call)
 *   4. mode of (x, u_applied)
 *   5. x <- x + Ts f(x, u_applied)        the OCP's f (evalModelVariableShape), qsp_closed_loop's plant step */
typedef struct {
    int32_t struct_size;      /* sizeof(qsp_open_loop_opts) (qsp_default_open_loop_opts sets it; checked) */
    int32_t n_steps;          /* T = length(0:sample_time:time_sim) */
    int32_t M;                /* input candidates per lane */
    int32_t u_steps;          /* 1: U is B x M x 2, held constant (repmat, :144); n_steps: U is B x M x T x 2 */
    int32_t clip;             /* 1 (default): step 2 */
    int32_t store_tile;       /* how the trajectories are written.  0 (default): the library's choice, the faster
                                 path measured for the call's M (steps of 4 below 64 candidates per lane, else 1);
                                 1: every thread stores its own rows; 4 or 8: that many steps are collected
                                 per thread in LDS and written out with consecutive threads on consecutive
                                 addresses.  Results are identical; a measurement knob */
    double Ts;                /* sample_time; 0: the handle's */
    double v_alpha;           /* 1.0 = 0.005 * 200 (:162) */
    double plant_delay;       /* plant.time_delay [s]: ceil(delay / Ts) buffer columns, as qsp_closed_loop_opts' */
} qsp_open_loop_opts;
void qsp_default_open_loop_opts(qsp_open_loop_opts* opts);   /* n_steps 1, M 1, u_steps 1, clip on, v_alpha 1 */
/* x0: B x 4; U: B x M x u_steps x 2; noise: n_steps x B x 4 or NULL (shared by a lane's candidates; NULL with a
 * generator installed, qsp_set_sim_noise below: drawn in the kernel);
 * shapes per lane as qsp_set_shape_ids.  Outputs, each optional except x_end:
 *   X          B x M x (n_steps + 1) x 4   the states, row n_steps the final one
 *   U_out      B x M x n_steps x 2         the commanded input after the clip (the reference's returned u)
 *   S_p        B x M x n_steps x 2         C(mod(s, b)), the contact point in the slider frame (:187)
 *   mode       B x M x n_steps             QSP_MODE_* of the applied input
 *   mode_steps B x M x 4                   steps spent in modes 0..3 (a sweep can skip the trajectories)
 *   x_end      B x M x 4 */
int qsp_open_loop(qsp_solver* s, const qsp_open_loop_opts* opts, const double* x0, const double* U,
                  const double* noise, double* X, double* U_out, double* S_p, int32_t* mode, int32_t* mode_steps,
                  double* x_end);
/* The same on caller-owned device memory, asynchronous on hip_stream (NULL: the handle's).  X, U_out and
 * S_p must be 16-byte aligned (device allocations are).  With the clip and a plant delay the delay buffer
 * is the handle's: one such call at a time per handle. */
typedef struct {
    const double* x0;        /* B x 4 */
    const double* U;         /* B x M x u_steps x 2 */
    const double* noise;     /* n_steps x B x 4 or NULL */
    const int32_t* shape_id; /* B or NULL: the handle's */
    double* X;               /* NULL or as above */
    double* U_out;
    double* S_p;
    int32_t* mode;
    int32_t* mode_steps;
    double* x_end;           /* B x M x 4 */
} qsp_open_loop_io;
int qsp_open_loop_device(qsp_solver* s, const qsp_open_loop_opts* opts, const qsp_open_loop_io* io, void* hip_stream);

/* ------------------------------------------- sim_noise generated on the device */
/* The reference's sim_noise branch (helper.m:240-242; open loop :154-156) adds four normals per lane and step,
 * x += [1e-5; 1e-5; 1e-3; 1e-4] .* randn(4, 1).  The entries above take them as a host table, noise: n_steps x B
 * x 4.  A generator installed on the handle draws them inside the kernels instead: no table is built, staged
 * or held, and the noise of (lane, step) is a pure function of the fields below, so every shard (lane_offset)
 * and every chunk (step_offset) of a run draws the numbers of the whole run.
 *   bits      Philox4x32-10 (Random123), one call per (lane, step), step = step_offset + t for the 0-based
 *             step t of the entry call:
 *                 counter = (uint32(lane_offset + lane), step low 32 bits, step high 32 bits, stream)
 *                 key     = (seed low 32 bits, seed high 32 bits)
 *   uniforms  u_j = (w_j + 0.5) * 2^-32 of the four output words w_0..w_3
 *   normals   z_0 = r cos(2 pi u_1), z_1 = r sin(2 pi u_1), r = sqrt(-2 log u_0); z_2, z_3 from (u_2, u_3)
 *             alike; |z| <= 6.76, always finite
 *   noise     x_c += (sigma[c] * lane_scale[lane]) * z_c
 * With a generator installed and noise == NULL (io->noise == NULL for qsp_open_loop_device), qsp_closed_loop,
 * qsp_closed_loop_ex, qsp_closed_loop_metrics, qsp_open_loop and qsp_open_loop_device draw the step's noise
 * where they add the table's: after the disturbance, before the log and the delay prediction; in the open
 * loop shared by a lane's M candidates.  The results are bit for bit those of the same call with the table
 * that qsp_gen_sim_noise writes.  A table passed while a generator is installed is ambiguous: QSP_ERR_ARG.
 * With nothing installed every result is bit-identical to a library without these entries. */
typedef struct {
    int32_t struct_size;       /* sizeof(qsp_sim_noise) (qsp_default_sim_noise sets it; checked) */
    uint32_t stream;           /* realisation index: counter word 3 */
    uint64_t seed;
    int64_t step_offset;       /* >= 0: step t of a call draws at step_offset + t */
    int64_t lane_offset;       /* >= 0, lane_offset + B <= 2^32: lane i draws as global lane lane_offset + i */
    double sigma[4];           /* finite, >= 0; default 1e-5, 1e-5, 1e-3, 1e-4 (helper.m:241) */
    const double* lane_scale;  /* B host doubles, finite, >= 0, copied; NULL: 1 */
} qsp_sim_noise;
void qsp_default_sim_noise(qsp_sim_noise* gen);   /* seed 0, stream 0, no offsets, the reference's sigma, no scale */
/* install (replacing what was installed); QSP_ERR_ARG leaves what was installed */
int qsp_set_sim_noise(qsp_solver* s, const qsp_sim_noise* gen);
int qsp_clear_sim_noise(qsp_solver* s);
/* what is installed: out (lane_scale NULL; the defaults when none is), installed 0 / 1, has_scale 0 / 1.  Each
 * of the three pointers may be NULL. */
int qsp_get_sim_noise(qsp_solver* s, qsp_sim_noise* out, int32_t* installed, int32_t* has_scale);
/* the table the loops draw over n_steps steps from step_offset, noise: n_steps x B x 4 (host), for inspection
 * and replay; QSP_ERR_STATE if no generator is installed */
int qsp_gen_sim_noise(qsp_solver* s, int32_t n_steps, double* noise);

#ifdef __cplusplus
}
#endif
#endif /* QSP_NMPC_H */
