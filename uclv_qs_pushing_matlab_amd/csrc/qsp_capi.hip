// qsp_capi.hip — C ABI (include/qsp_nmpc.h): handle, device buffers, set/solve/get.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/qsp_nmpc.h"
#include "qsp_devbuf.hpp"
#include "qsp_ipm.hpp"
#include "qsp_kernels.h"

using namespace qsp;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) return fail(QSP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr int STAGE_POOL = 13;   // most host arrays of one call (qsp_qp_residuals: 13)

// Every device array is a Dev<T> member (qsp_devbuf.hpp): it is freed with the handle, whichever call allocated it.
struct __attribute__((visibility("hidden"))) qsp_solver {
    qsp_options o;
    SolveParams p;
    Dims dim;                       // element counts of the handle's arrays (batch, N)
    int S = 1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int n_shapes = 0;
    Dev<ShapeDev> shapes;
    Dev<int32_t> shape_id, status, sqp_iter, qp_iter, qp_capped, qp_stalled, index_time;
    Dev<double> x0, yref, yref_e, X, U, PI, Xo, Uo, PIo, u0, cost, traj;
    Dev<uint8_t> warm_valid;
    // delay compensation (set_delay_comp, NMPC_controller.m:106-110): delay_buff_comp columns and the
    // per-lane controller input buffer u_buff_contr (B x D x 2, column 0 newest); closed-loop state:
    // the plant's buffer and state, the disturbance amplitudes, the noise table (n_steps x B x 4; not
    // allocated when the generator below draws the noise) and the
    // logs of a run with trajectories (B x n_steps: X_sim, X_traj, U_traj, status_traj)
    int32_t D = 0;
    Dev<double> ubc, ubp, cl_x, cl_amp, cl_noise, cl_xsim, cl_xtraj, cl_utraj;
    Dev<int32_t> cl_straj;
    // the plant's own model (qsp_set_plant_*): shape table, ids, per-lane mu_sp / c_ellipse; the closed
    // loop's metric accumulators (qsp_closed_loop_metrics)
    int n_pshapes = 0;
    bool has_pids = false, has_pmu = false, has_pc = false;
    Dev<ShapeDev> pshapes;
    Dev<int32_t> pshape_id;
    Dev<double> pmu, pc, cl_metrics;
    // sim_noise drawn in the kernels (qsp_set_sim_noise): the generator as installed (lane_scale NULL) and the
    // device copy of its per-lane scale
    bool sn_on = false, sn_has_scale = false;
    qsp_sim_noise sn = {};
    Dev<double> sn_scale;
    Dev<double> wX, wU, wx0, wlin, wnlp, wres, wqp, wadj;
    Dev<int32_t> wdone, wperm, wnit, whist, wadjv;
    Dev<uint8_t> pool[STAGE_POOL];  // device images of one call's host arrays (bytes), handed out by Staging
    Dev<double> ol_ring;            // qsp_open_loop's plant delay buffer (clipped u_t of the last D steps)
    Dev<double> wsens, wsensK;      // the sensitivity entries' workspace (SensField; the gains of the forward pass), on first use
    bool solved = false;            // wU holds a solve's iterate (qsp_cost_landscape with U_tail = NULL)
    int32_t T = 0;
    bool have_traj = false;
    bool have_yref = false;         // yref / yref_e hold references (a setter's or a controller step's)
    bool traj_per_lane = false;     // reference table per lane (B x T x 6) instead of shared (T x 6)
    float last_ms = 0.0f;
    bool last_controller = false;
    bool poison = false;            // QSP_DEBUG_POISON=1: NaN-filled workspace and QP-kernel LDS   // get_x/u/pi: controller mode returns the shifted warm start (utraj/xtraj/ptraj)
    std::vector<hipEvent_t> kev;   // kernel-timing pool (qsp_set_kernel_timing)
    int kev_used = 0;
    std::vector<int> kev_solves;   // event offset of each timed solve
    std::vector<int> kev_split;    // ... and whether its SQP loop ran in two parts
    bool auto_timing = false;      // qsp_set_timing: every solve times its kernels (acados time_lin / time_qp_sol)
    // two-stream SQP loop (launch_sqp): second stream, fork/join events, requested parts (0 = auto)
    SqpStreams split;
    int parts_req = 0;
    int fused_req = -1;            // QSP_FUSED_LOOP (-1: auto)
    bool nopack = false;           // QSP_PACKING=0: instances in lane order (developer A/B of the wave packing)
    bool mfw = true;               // QSP_MFMA_WALK=0: the lane walk wherever the matrix cores would factorise (developer
                                   // A/B; rounds differently: the oracle twin reads it by the same mfma_walk_default)
    bool fixed_n = true;           // QSP_FIXED_HORIZON=0: the runtime-horizon QP kernel at every N (developer A/B; same bits)
    int cus = 256;                 // compute units of the device (hipDeviceProp multiProcessorCount)

    // streams and events here, on the handle's device; the buffers free themselves after this body
    ~qsp_solver() {
        (void)hipSetDevice(o.device);
        for (hipEvent_t e : kev) (void)hipEventDestroy(e);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (split.fork) (void)hipEventDestroy(split.fork);
        for (int q = 0; q < SQP_MAX_PARTS - 1; ++q) {
            if (split.join[q]) (void)hipEventDestroy(split.join[q]);
            if (split.aux[q]) (void)hipStreamDestroy(split.aux[q]);
        }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// --------------------------------------------------------------- helpers
static const SqpStreams* sqp_split(qsp_solver* s) {
    s->split.parts = s->parts_req > 0 ? s->parts_req : sqp_parts_auto(s->o.batch, s->o.N, s->S, s->cus);
    // the whole SQP loop in one launch: auto for batches below one fill of the wave slots
    // when one part is in use; QSP_FUSED_LOOP=0/1 overrides (experiments, parity tests) where
    // the fused kernel exists (nlp_mode 0, S = 1 or 2)
    const bool can_fuse = s->o.nlp_mode == QSP_NLP_SQP_RTI_FIXED && (s->S == 1 || s->S == 2);
    s->split.fused = !can_fuse ? 0
                   : s->fused_req >= 0 ? s->fused_req
                   : (s->split.parts == 1 && sqp_fused_auto(s->o.batch, s->o.N, s->S, s->o.nlp_mode, s->cus));
    if (s->split.fused) s->split.parts = 1;
    return &s->split;
}

// events for one timed solve (nullptr when timing is off or the pool is used up); with
// qsp_set_timing the one-solve pool is reused by every solve (the last one is reported)
static hipEvent_t* take_kernel_events(qsp_solver* s) {
    const int per = 2 * s->o.sqp_iters + 3;
    if (s->auto_timing) {
        s->kev_used = 0;
        s->kev_solves.clear();
        s->kev_split.clear();
    }
    if (s->kev.empty() || s->kev_used + per > (int)s->kev.size()) return nullptr;
    s->kev_solves.push_back(s->kev_used);
    s->kev_split.push_back((sqp_split(s)->parts > 1 || s->split.fused) ? 1 : 0);
    hipEvent_t* e = s->kev.data() + s->kev_used;
    s->kev_used += per;
    return e;
}

static int kernel_times_of(qsp_solver* s, double* ms, int32_t* launches);

static void fill_params(qsp_solver* s) {
    SolveParams& p = s->p;
    params_from_options(p, s->o);   // (qsp_ipm.hpp: the fields the twin's options name alike)
    p.tau = s->o.cost_scale_Ts ? s->o.Ts : 1.0;
    p.mfma_walk = s->mfw ? 1 : 0;
    mfw_prepare(p);
}

// Binary little-endian PLY with float32 vertex properties (the reference's cad_models/*.ply).
static int read_ply_xy(const char* path, std::vector<float>& xy) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(QSP_ERR_IO, std::string("cannot open ") + path);
    std::string hdr;
    char line[512];
    int nv = -1, nprop = 0;
    bool binle = false;
    while (std::fgets(line, sizeof line, f)) {
        std::string l(line);
        if (l.rfind("format binary_little_endian", 0) == 0) binle = true;
        if (l.rfind("element vertex", 0) == 0) nv = std::atoi(l.c_str() + 14);
        if (l.rfind("property float", 0) == 0) ++nprop;
        if (l.rfind("property list", 0) == 0 && nv < 0) { std::fclose(f); return fail(QSP_ERR_IO, "unsupported PLY"); }
        if (l.rfind("end_header", 0) == 0) break;
    }
    if (!binle || nv <= 0 || nprop < 2) { std::fclose(f); return fail(QSP_ERR_IO, std::string("unsupported PLY ") + path); }
    std::vector<float> v((size_t)nv * nprop);
    if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) { std::fclose(f); return fail(QSP_ERR_IO, "short PLY"); }
    std::fclose(f);
    xy.resize((size_t)nv * 2);
    for (int i = 0; i < nv; ++i) { xy[2 * i] = v[(size_t)i * nprop]; xy[2 * i + 1] = v[(size_t)i * nprop + 1]; }
    return QSP_OK;
}

// host array -> buffer / buffer -> host array, `count` elements, on the handle's stream, synchronised
template <class T>
static int h2d(qsp_solver* s, const Dev<T>& b, const T* src, size_t count) {
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(b.upload(s->stream, src, count));
    HIPCHK(hipStreamSynchronize(s->stream));
    return QSP_OK;
}
template <class T>
static int h2d_grow(qsp_solver* s, Dev<T>& b, const T* src, size_t count) {   // ... into a buffer grown to `count` first
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(b.ensure(count));
    return h2d(s, b, src, count);
}
template <class T>
static int d2h(qsp_solver* s, T* dst, const Dev<T>& b, size_t count) {
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(b.download(s->stream, dst, count));
    HIPCHK(hipStreamSynchronize(s->stream));
    return QSP_OK;
}

// The setters and getters of one whole array: the entry's name, its null test ("<who>: null argument"),
// the handle's buffer and its count from Dims.  ctl: the buffer that holds the array after a controller
// solve (the shifted warm start), where that is another one.
using DimsCount = size_t (Dims::*)() const;
template <class T>
static int set_array(qsp_solver* s, const char* who, const T* host, Dev<T> qsp_solver::*buf, DimsCount count) {
    if (!s || !host) return fail(QSP_ERR_ARG, std::string(who) + ": null argument");
    return h2d(s, s->*buf, host, (s->dim.*count)());
}
template <class T>
static int get_array(qsp_solver* s, const char* who, T* host, Dev<T> qsp_solver::*buf, DimsCount count,
                     Dev<T> qsp_solver::*ctl = nullptr) {
    if (!s || !host) return fail(QSP_ERR_ARG, std::string(who) + ": null argument");
    return d2h(s, host, s->*(ctl && s->last_controller ? ctl : buf), (s->dim.*count)());
}

static SolveArgs make_args(qsp_solver* s) {
    SolveArgs a;
    std::memset(&a, 0, sizeof a);
    a.p = s->p;
    a.B = s->o.batch;
    a.shapes = s->shapes.data();
    a.n_shapes = s->n_shapes;
    a.shape_id = s->shape_id.data();
    a.x0 = s->x0.data();
    a.yref = s->yref.data();
    a.yref_e = s->yref_e.data();
    a.X_in = s->X.data();
    a.U_in = s->U.data();
    a.u0 = s->u0.data();
    a.X_out = s->Xo.data();
    a.U_out = s->Uo.data();
    a.PI_out = s->PIo.data();
    s->last_controller = false;
    a.status = s->status.data();
    a.sqp_iter = s->sqp_iter.data();
    a.qp_iter = s->qp_iter.data();
    a.qp_capped = s->qp_capped.data();
    a.qp_stalled = s->qp_stalled.data();
    a.cost = s->cost.data();
    a.wX = s->wX.data();
    a.wU = s->wU.data();
    a.wx0 = s->wx0.data();
    a.wlin = s->wlin.data();
    a.wnlp = s->wnlp.data();
    a.wdone = s->wdone.data();
    a.wres = s->wres.data();
    a.wqp = s->wqp.data();
    a.wperm = s->nopack ? nullptr : s->wperm.data();
    if (s->poison) a.flags |= QSP_FLAG_POISON;
    if (!s->fixed_n) a.flags |= QSP_FLAG_RUNTIME_N;
    a.wnit = s->wnit.data();
    a.whist = s->whist.data();
    a.wadj = s->wadj.data();
    a.wadjv = s->wadjv.data();
    a.PI_in = s->PI.data();   // 'init_pi' (solve) / shifted warm start (controller)
    return a;
}

static int run_timed(qsp_solver* s, const SolveArgs& a) {
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    HIPCHK(launch_sqp(a, s->S, s->stream, take_kernel_events(s), sqp_split(s)));
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    HIPCHK(hipEventSynchronize(s->ev1));
    HIPCHK(hipEventElapsedTime(&s->last_ms, s->ev0, s->ev1));
    s->solved = true;
    return QSP_OK;
}

// The device images of one call's host arrays, one object per call: the handle's grow-only pool handed
// out in call order, all copies on the handle's stream.  in() copies a host array in, out() reserves the
// image of one that finish() copies back; a null host pointer (an optional array) gives a null device
// pointer.  The first error stays in err (and in qsp_last_error) and turns every later step into a no-op,
// so a caller checks once before its launch and returns finish().
struct Staging {
    qsp_solver* s;
    int used = 0, n_out = 0, err = QSP_OK;
    struct { void* host; const void* dev; size_t bytes; } outs[STAGE_POOL];

    explicit Staging(qsp_solver* s_) : s(s_) {}
    void check(hipError_t e, const char* what) {
        if (e != hipSuccess && !err) err = fail(QSP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    void* take(size_t bytes) {
        if (!err && used == STAGE_POOL) err = fail(QSP_ERR_STATE, "staging pool exhausted: more than STAGE_POOL arrays in one call");
        if (err) return nullptr;
        Dev<uint8_t>& b = s->pool[used++];
        check(b.ensure(bytes), "staging hipMalloc");
        return err ? nullptr : b.data();
    }
    template <class T>
    T* in(const T* host, size_t count) {
        void* d = host ? take(count * sizeof(T)) : nullptr;
        if (d) check(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, s->stream), "staging copy in");
        return static_cast<T*>(d);
    }
    template <class T>
    T* out(T* host, size_t count) {
        void* d = host ? take(count * sizeof(T)) : nullptr;
        if (d) outs[n_out++] = {host, d, count * sizeof(T)};   // n_out <= used <= STAGE_POOL
        return static_cast<T*>(d);
    }
    int finish() {
        for (int q = 0; q < n_out && !err; ++q)
            check(hipMemcpyAsync(outs[q].host, outs[q].dev, outs[q].bytes, hipMemcpyDeviceToHost, s->stream), "staging copy out");
        if (!err) check(hipStreamSynchronize(s->stream), "hipStreamSynchronize");
        return err;
    }
};

// The inputs of an NLP point from an evaluator's io block (qsp_kkt_io, qsp_sens_io: x0, X, U, PI, LAM, yref,
// shape_id) into the kernels' PointIn: host arrays go through the staging pool (st.err says how that went),
// device arrays are used as they are; shape_id and the references fall back to the handle's.  refs = false:
// the call reads no references.
template <class IO>
static PointIn point_in(qsp_solver* s, Staging& st, bool host, const IO& io, const double* yref_e, bool refs) {
    const Dims& dim = s->dim;
    const auto in = [&](const double* v, size_t n) -> const double* { return host ? st.in(v, n) : v; };
    PointIn pt;
    pt.shapes = s->shapes.data();
    pt.n_shapes = s->n_shapes;
    pt.shape_id = io.shape_id ? io.shape_id : s->shape_id.data();
    pt.x0 = in(io.x0, dim.x0());
    pt.X = in(io.X, dim.X());
    pt.U = in(io.U, dim.U());
    pt.PI = in(io.PI, dim.PI());
    pt.LAM = in(io.LAM, dim.lam());
    pt.yref = refs ? in(io.yref, dim.yref()) : nullptr;
    pt.yref_e = refs ? in(yref_e, dim.yref_e()) : nullptr;
    if (refs && !pt.yref) pt.yref = s->yref.data();
    if (refs && !pt.yref_e) pt.yref_e = s->yref_e.data();
    return pt;
}

static int check_ids(qsp_solver* s, int32_t n, const int32_t* ids) {
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, "no shapes set");
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= s->n_shapes) return fail(QSP_ERR_ARG, "shape id out of range");
    return QSP_OK;
}

// y_ref staging for the controller step at index_time + offset
static hipError_t launch_controller_step(qsp_solver* s, int offset) {
    s->have_yref = true;
    return launch_stage_yref(s->traj.data(), s->T, s->traj_per_lane ? 1 : 0, s->index_time.data(), offset,
                             s->D, s->o.batch, s->o.N, s->yref.data(), s->yref_e.data(), s->stream);
}

// NMPC_controller.solve arguments: warm buffers updated in place (each instance reads its
// own stages before writing), shifted outputs
static SolveArgs controller_args(qsp_solver* s) {
    SolveArgs a = make_args(s);
    a.flags |= QSP_FLAG_CONTROLLER | QSP_FLAG_SHIFT;
    a.warm_valid = s->warm_valid.data();
    a.X_out = s->X.data();
    a.U_out = s->U.data();
    a.PI_out = s->PI.data();
    s->last_controller = true;
    return a;
}

extern "C" {

void qsp_default_options(qsp_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->N = 20;
    o->batch = 1;
    o->nlp_mode = QSP_NLP_SQP_RTI_FIXED;
    o->sqp_iters = 50;
    o->qp_iters = 20;               // acados qp_solver_iter_max is 50: measured no effect on chaos, 2.3x slower at B = 4 096
    o->stages_per_lane = 0;
    o->device = 0;
    o->cost_scale_Ts = 1;
    o->Ts = 0.05;
    o->mu0 = 1.0;
    o->t_min = 1e-2;
    o->frac = 0.995;
    o->sigma_min = 1e-2;
    o->mu_stop = 1e-10;
    o->res_stop = 1e-10;
    o->qp_tol_stat = 1e-10;
    o->qp_tol_eq = 1e-10;
    o->stage0_s_bound = 1;          // acados: bgh constraints on stages 0..N-1
    o->qp_stall_iters = 3;          // stall exit: alpha < 1e-3 three times in a row
    o->qp_stall_alpha = 1e-3;
    o->qp_mu_max = 1e100;           // divergence exit: overflow guard
    o->factor_scan = 0;             // S = 2 factorisation: the walk (the scan is faster, less accurate: DESIGN.md 4)
    o->struct_size = (int32_t)sizeof(qsp_options);
    // nlp_mode 1: NMPC_controller.m:275-276 tolerances; acados merit_backtracking defaults
    o->tol_stat = o->tol_eq = o->tol_ineq = o->tol_comp = 1e-6;
    o->ls_alpha_min = 0.05;
    o->ls_alpha_red = 0.7;
    o->ls_eps = 1e-4;
}

int qsp_version(void) { return QSP_ABI_VERSION; }

const char* qsp_last_error(void) { return g_err.c_str(); }

int qsp_create(const qsp_options* o, qsp_solver** out) {
    if (!o || !out) return fail(QSP_ERR_ARG, "qsp_create: null argument");
    if (o->struct_size != (int32_t)sizeof(qsp_options))
        return fail(QSP_ERR_ARG, "qsp_create: qsp_options.struct_size != sizeof(qsp_options) (caller built "
                                 "against another qsp_nmpc.h? check qsp_version() == QSP_ABI_VERSION)");
    if (!(o->qp_mu_max > 0.0)) return fail(QSP_ERR_ARG, "qsp_create: qp_mu_max must be > 0");
    if (o->N < 1 || o->batch < 1) return fail(QSP_ERR_ARG, "qsp_create: N and batch must be >= 1");
    if (o->nlp_mode != QSP_NLP_SQP_RTI_FIXED && o->nlp_mode != QSP_NLP_SQP_MERIT)
        return fail(QSP_ERR_ARG, "qsp_create: unsupported nlp_mode");
    if (o->nlp_mode == QSP_NLP_SQP_MERIT &&
        (o->N + 1 > 64 || o->stages_per_lane > 1 || !(o->ls_alpha_red > 0.0 && o->ls_alpha_red < 1.0) ||
         !(o->ls_alpha_min > 0.0 && o->ls_alpha_min <= 1.0)))
        return fail(QSP_ERR_ARG, "qsp_create: nlp_mode 1 needs N+1 <= 64 (one stage per lane), "
                                 "0 < ls_alpha_red < 1 and 0 < ls_alpha_min <= 1");
    if (o->sqp_iters < 1 || o->qp_iters < 1) return fail(QSP_ERR_ARG, "qsp_create: iteration counts must be >= 1");
    if (o->qp_iters > 255) return fail(QSP_ERR_ARG, "qsp_create: qp_iters must be <= 255");
    if (o->qp_stall_iters < 0) return fail(QSP_ERR_ARG, "qsp_create: qp_stall_iters must be >= 0");
    if (o->factor_scan != 0 && o->factor_scan != 1) return fail(QSP_ERR_ARG, "qsp_create: factor_scan must be 0 or 1");
    if (!(o->qp_tol_stat > 0.0) || !(o->qp_tol_eq > 0.0) || !(o->mu_stop > 0.0) || !(o->res_stop > 0.0))
        return fail(QSP_ERR_ARG, "qsp_create: QP stop tolerances must be > 0");
    if (!(o->Ts > 0.0)) return fail(QSP_ERR_ARG, "qsp_create: Ts must be > 0");
    const int S = stages_per_lane(o->N, o->nlp_mode, o->stages_per_lane);
    if (S < 1 || S > 2) return fail(QSP_ERR_ARG, "qsp_create: stages_per_lane must be 1 or 2");
    if (lanes_per_instance(o->N, S) > 64)
        return fail(QSP_ERR_ARG, "qsp_create: N+1 > 64*stages_per_lane (one instance must fit in a wavefront)");
    HIPCHK(hipSetDevice(o->device));
    qsp_solver* s = new qsp_solver();
    s->o = *o;
    s->S = S;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, o->device) == hipSuccess && prop.multiProcessorCount > 0)
            s->cus = prop.multiProcessorCount;
    }
    s->mfw = mfma_walk_default() != 0;
    fill_params(s);
    // reference defaults (main.m:82-90, NMPC_controller.m:16-26, 98-100, 251-252)
    const double W[6] = {1.0, 1.0, 1e-3, 0.0, 1e-3, 1e-3};
    const double We[4] = {2e5, 2e5, 20.0, 0.0};
    const double lh[3] = {-0.06, 0.0, -0.05}, uh[3] = {0.011, 0.03, 0.05};
    std::memcpy(s->p.W, W, sizeof W);
    std::memcpy(s->p.We, We, sizeof We);
    std::memcpy(s->p.lh, lh, sizeof lh);
    std::memcpy(s->p.uh, uh, sizeof uh);
    s->p.cp = CtrlParams{1.0, 0.0, 3.0, 0.0, 0.05};
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&s->ev0);
    if (e == hipSuccess) e = hipEventCreate(&s->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->split.fork, hipEventDisableTiming);
    for (int q = 0; q < SQP_MAX_PARTS - 1; ++q) {
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->split.aux[q], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->split.join[q], hipEventDisableTiming);
    }
    if (const char* fl = std::getenv("QSP_FUSED_LOOP")) s->fused_req = (fl[0] == '1') ? 1 : (fl[0] == '0' ? 0 : -1);
    if (const char* pk = std::getenv("QSP_PACKING")) s->nopack = pk[0] == '0';
    if (const char* fh = std::getenv("QSP_FIXED_HORIZON")) s->fixed_n = fh[0] != '0';
    const char* pz = std::getenv("QSP_DEBUG_POISON");
    s->poison = pz && pz[0] == '1';
    s->dim = Dims{(size_t)o->batch, (size_t)o->N};
    const Dims& d = s->dim;
    // POISON (debug, QSP_DEBUG_POISON=1): every byte of the buffer starts as a NaN pattern, so a kernel that
    // reads a word it never wrote shows up as NaN (tests/test_gpu_errors.py)
    enum Mark { PLAIN, POISON };
    auto al = [&](auto& b, size_t count, Mark mark = PLAIN) {
        if (e == hipSuccess) e = b.ensure(count);
        if (e == hipSuccess && mark == POISON && s->poison) e = b.fill(s->stream, 0xff, count);
    };
    auto zero = [&](auto& b, size_t count) { if (e == hipSuccess) e = b.fill(s->stream, 0, count); };
    al(s->shape_id, d.lane());
    al(s->x0, d.x0());
    al(s->yref, d.yref(), POISON);
    al(s->yref_e, d.yref_e(), POISON);
    for (auto* b : {&s->X, &s->Xo, &s->wX}) al(*b, d.X(), POISON);
    for (auto* b : {&s->U, &s->Uo, &s->wU}) al(*b, d.U(), POISON);
    for (auto* b : {&s->PI, &s->PIo}) al(*b, d.PI(), POISON);
    al(s->u0, d.u0(), POISON);
    for (auto* b : {&s->status, &s->sqp_iter, &s->qp_iter, &s->qp_capped, &s->qp_stalled}) al(*b, d.lane());
    al(s->cost, d.lane(), POISON);
    al(s->warm_valid, d.lane());
    al(s->wx0, d.x0(), POISON);
    for (auto* b : {&s->wperm, &s->wnit, &s->wdone}) al(*b, d.lane(), POISON);
    al(s->whist, Dims::hist());   // per part of the SQP loop
    if (o->nlp_mode == QSP_NLP_SQP_MERIT) {
        // stage data in HBM only for the line search (defect and gradient at the iterate); the
        // fixed-K path linearises inside the QP kernel, and qsp_qp_solve stages its own
        al(s->wlin, d.lin(), POISON);
        al(s->wnlp, d.nlp(), POISON);
        al(s->wqp, d.qp(), POISON);
        al(s->wres, d.res(), POISON);
    } else {
        // fixed-K path: the adjoint record of each instance's last successful QP; the dynamics
        // multipliers are computed from it once per solve (epilogue_kernel)
        al(s->wadj, d.adj(), POISON);
        al(s->wadjv, d.lane(), POISON);
    }
    // what a caller legitimately relies on being zero, poisoned or not: the ids, the initial guess and warm state
    zero(s->shape_id, d.lane());
    zero(s->warm_valid, d.lane());
    zero(s->X, d.X());
    zero(s->U, d.U());
    zero(s->PI, d.PI());
    // qsp_get_residuals before the first solve returns zeros (header contract)
    if (s->wres.data()) zero(s->wres, d.res());
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) {
        std::string m = std::string("qsp_create: ") + hipGetErrorString(e);
        delete s;
        return fail(QSP_ERR_HIP, m);
    }
    *out = s;
    return QSP_OK;
}

int qsp_destroy(qsp_solver* s) {
    delete s;   // ~qsp_solver selects the handle's device
    return QSP_OK;
}

int qsp_get_layout(const qsp_solver* s, int32_t* S, int32_t* L) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_get_layout: null handle");
    if (S) *S = s->S;
    if (L) *L = lanes_per_instance(s->o.N, s->S);
    return QSP_OK;
}

int qsp_get_factor_walk(const qsp_solver* s, int32_t* walk) {
    if (!s || !walk) return fail(QSP_ERR_ARG, "qsp_get_factor_walk: null argument");
    *walk = factor_walk_kind(s->p, s->S);
    return QSP_OK;
}

int qsp_get_fixed_horizon(const qsp_solver* s, int32_t* N) {
    if (!s || !N) return fail(QSP_ERR_ARG, "qsp_get_fixed_horizon: null argument");
    *N = qp_fixed_horizon(s->p, s->S, s->fixed_n ? 0u : QSP_FLAG_RUNTIME_N);
    return QSP_OK;
}

// ------------------------------------------------------------------ shapes
int qsp_shape_from_ply(const char* path, int32_t flip, double mu_sg, double mu_sp, double mass, double tau_max,
                       qsp_shape* out) {
    if (!path || !out) return fail(QSP_ERR_ARG, "qsp_shape_from_ply: null argument");
    std::vector<float> P;
    int r = read_ply_xy(path, P);
    if (r != QSP_OK) return r;
    const int n0 = (int)(P.size() / 2);
    if (n0 + 1 > QSP_MAX_CTRL) return fail(QSP_ERR_ARG, "qsp_shape_from_ply: too many points");
    // sortCadPoints (PusherSliderModel.m:84-111): start at the first min-x point, then
    // greedy nearest neighbour in float32 with first-index ties; consumed points -> Inf.
    std::vector<float> xs(P);
    const float inf = INFINITY;
    int ind = 0;
    for (int i = 1; i < n0; ++i) if (xs[2 * i] < xs[2 * ind]) ind = i;
    float tx = xs[2 * ind], ty = xs[2 * ind + 1];
    xs[2 * ind] = xs[2 * ind + 1] = inf;
    std::vector<double> srt((size_t)(n0 + 1) * 2);
    srt[0] = tx; srt[1] = ty;
    for (int i = 1; i < n0; ++i) {
        int best = -1;
        float bd = 0.0f;
        for (int q = 0; q < n0; ++q) {
            const float dx = xs[2 * q] - tx, dy = xs[2 * q + 1] - ty;
            const float d = std::sqrt(dx * dx + dy * dy);
            if (best < 0 || d < bd) { best = q; bd = d; }
        }
        tx = xs[2 * best]; ty = xs[2 * best + 1];
        srt[2 * i] = tx; srt[2 * i + 1] = ty;
        xs[2 * best] = xs[2 * best + 1] = inf;
    }
    const double sc = 1.0 / 1000.0;   // scale_factor (PusherSliderModel.m:72,105)
    for (int i = 0; i < n0; ++i) { srt[2 * i] *= sc; srt[2 * i + 1] *= sc; }
    srt[2 * n0] = srt[0]; srt[2 * n0 + 1] = srt[1];   // close the loop (:106)
    const int n = n0 + 1;
    if (flip) {   // flipud for montana / pulirapid (:107-109)
        for (int i = 0; i < n / 2; ++i)
            for (int c = 0; c < 2; ++c) std::swap(srt[2 * i + c], srt[2 * (n - 1 - i) + c]);
    }
    std::memset(out, 0, sizeof(*out));
    out->n_ctrl = n;
    out->struct_size = (int32_t)sizeof(qsp_shape);
    for (int i = 0; i < n; ++i) { out->ctrl[i][0] = srt[2 * i]; out->ctrl[i][1] = srt[2 * i + 1]; }
    // knots (getSpline :117-123): p = 3, m = n - 2, S = [0 0 0 linspace(0,b,m) b b b]
    double b = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
        const double dx = out->ctrl[i + 1][0] - out->ctrl[i][0], dy = out->ctrl[i + 1][1] - out->ctrl[i][1];
        b += std::sqrt(dx * dx + dy * dy);
    }
    const int m = n - 2;
    for (int i = 0; i < 3; ++i) out->knots[i] = 0.0;
    const double step = b / (double)(m - 1);
    for (int i = 0; i < m; ++i) out->knots[3 + i] = (i == m - 1) ? b : (double)i * step;
    for (int i = 0; i < 3; ++i) out->knots[3 + m + i] = b;
    out->b = b;
    out->c_ellipse = tau_max / (mu_sg * mass * 9.81);   // :53,55 with helper.g = 9.81
    out->mu_sp = mu_sp;
    return QSP_OK;
}

// qsp_shape table -> device ShapeDev table in the handle's `table` (qsp_set_shapes, qsp_set_plant_shapes)
static int upload_shapes(qsp_solver* s, const char* who, const qsp_shape* shapes, int32_t n,
                         Dev<ShapeDev> qsp_solver::*table) {
    const std::string w(who);
    if (!s || !shapes || n < 1) return fail(QSP_ERR_ARG, w + ": bad argument");
    std::vector<ShapeDev> h((size_t)n);
    for (int q = 0; q < n; ++q) {
        const qsp_shape& in = shapes[q];
        if (in.struct_size != (int32_t)sizeof(qsp_shape))
            return fail(QSP_ERR_ARG, w + ": qsp_shape.struct_size != sizeof(qsp_shape) (stale layout?)");
        if (in.n_ctrl < 5 || in.n_ctrl > QSP_MAX_CTRL) return fail(QSP_ERR_ARG, w + ": n_ctrl out of range");
        shape_entry(h[q], in.n_ctrl, &in.ctrl[0][0], in.knots, in.b, in.c_ellipse, in.mu_sp, in.xwidth);
    }
    return h2d_grow(s, s->*table, h.data(), h.size());
}

int qsp_set_shapes(qsp_solver* s, const qsp_shape* shapes, int32_t n) {
    const int r = upload_shapes(s, "qsp_set_shapes", shapes, n, &qsp_solver::shapes);
    if (r) return r;
    s->n_shapes = n;
    return QSP_OK;
}

int qsp_set_shape_ids(qsp_solver* s, const int32_t* ids) {
    if (!s || !ids) return fail(QSP_ERR_ARG, "qsp_set_shape_ids: null argument");
    for (int i = 0; i < s->o.batch; ++i)
        if (ids[i] < 0 || ids[i] >= s->n_shapes) return fail(QSP_ERR_ARG, "qsp_set_shape_ids: id out of range");
    return h2d(s, s->shape_id, ids, s->dim.lane());
}

// ------------------------------------------------- the plant's own model
int qsp_set_plant_shapes(qsp_solver* s, const qsp_shape* shapes, int32_t n) {
    const int r = upload_shapes(s, "qsp_set_plant_shapes", shapes, n, &qsp_solver::pshapes);
    if (r) return r;
    s->n_pshapes = n;
    s->has_pids = false;   // every lane back to plant shape 0
    return QSP_OK;
}

int qsp_set_plant_shape_ids(qsp_solver* s, const int32_t* ids) {
    if (!s || !ids) return fail(QSP_ERR_ARG, "qsp_set_plant_shape_ids: null argument");
    if (s->n_pshapes < 1) return fail(QSP_ERR_STATE, "qsp_set_plant_shape_ids: no plant shapes set");
    const size_t B = s->dim.lane();
    for (size_t i = 0; i < B; ++i)
        if (ids[i] < 0 || ids[i] >= s->n_pshapes) return fail(QSP_ERR_ARG, "qsp_set_plant_shape_ids: id out of range");
    const int r = h2d_grow(s, s->pshape_id, ids, B);
    if (r) return r;
    s->has_pids = true;
    return QSP_OK;
}

int qsp_set_plant_params(qsp_solver* s, const double* mu_sp, const double* c_ellipse) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_set_plant_params: null handle");
    const size_t B = s->dim.lane();
    for (const double* v : {mu_sp, c_ellipse})
        for (size_t i = 0; v && i < B; ++i)
            if (!(std::isfinite(v[i]) && v[i] > 0.0))
                return fail(QSP_ERR_ARG, "qsp_set_plant_params: mu_sp and c_ellipse must be finite and > 0");
    int r;
    if (mu_sp && (r = h2d_grow(s, s->pmu, mu_sp, B))) return r;
    if (c_ellipse && (r = h2d_grow(s, s->pc, c_ellipse, B))) return r;
    s->has_pmu = mu_sp != nullptr;
    s->has_pc = c_ellipse != nullptr;
    return QSP_OK;
}

int qsp_clear_plant(qsp_solver* s) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_clear_plant: null handle");
    s->n_pshapes = 0;
    s->has_pids = s->has_pmu = s->has_pc = false;
    return QSP_OK;
}

int qsp_get_plant(qsp_solver* s, int32_t* has_shapes, int32_t* has_params) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_get_plant: null handle");
    if (has_shapes) *has_shapes = s->n_pshapes;
    if (has_params) *has_params = (s->has_pmu ? 1 : 0) | (s->has_pc ? 2 : 0);
    return QSP_OK;
}

int qsp_set_cost_W(qsp_solver* s, const double W[6], const double We[4]) {
    if (!s || !W || !We) return fail(QSP_ERR_ARG, "qsp_set_cost_W: null argument");
    for (int i = 0; i < 6; ++i) if (!(W[i] >= 0.0)) return fail(QSP_ERR_ARG, "qsp_set_cost_W: W must be >= 0");
    for (int i = 0; i < 4; ++i) if (!(We[i] >= 0.0)) return fail(QSP_ERR_ARG, "qsp_set_cost_W: W_e must be >= 0");
    if (!(W[4] > 0.0 && W[5] > 0.0)) return fail(QSP_ERR_ARG, "qsp_set_cost_W: control weights must be > 0");
    std::memcpy(s->p.W, W, sizeof(double) * 6);
    std::memcpy(s->p.We, We, sizeof(double) * 4);
    return QSP_OK;
}

int qsp_set_constr_h(qsp_solver* s, const double lh[3], const double uh[3]) {
    if (!s || !lh || !uh) return fail(QSP_ERR_ARG, "qsp_set_constr_h: null argument");
    for (int i = 0; i < 3; ++i) if (!(lh[i] < uh[i])) return fail(QSP_ERR_ARG, "qsp_set_constr_h: need lh < uh");
    std::memcpy(s->p.lh, lh, sizeof(double) * 3);
    std::memcpy(s->p.uh, uh, sizeof(double) * 3);
    return QSP_OK;
}

int qsp_set_ctrl_params(qsp_solver* s, double v_alpha, double d_v, double t_angle0, double u_n_lb, double u_t_ub) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_set_ctrl_params: null handle");
    s->p.cp = CtrlParams{v_alpha, d_v, t_angle0, u_n_lb, u_t_ub};
    return QSP_OK;
}

// --------------------------------------------------------- acados level
int qsp_set_x0(qsp_solver* s, const double* x0) { return set_array(s, "qsp_set_x0", x0, &qsp_solver::x0, &Dims::x0); }

int qsp_set_yref(qsp_solver* s, const double* yref, const double* yref_e) {
    if (!s || !yref || !yref_e) return fail(QSP_ERR_ARG, "qsp_set_yref: null argument");
    int r = h2d(s, s->yref, yref, s->dim.yref());
    if (!r) r = h2d(s, s->yref_e, yref_e, s->dim.yref_e());
    if (!r) s->have_yref = true;
    return r;
}

int qsp_set_init(qsp_solver* s, const double* X, const double* U, const double* PI) {
    if (!s || !X || !U) return fail(QSP_ERR_ARG, "qsp_set_init: null argument");
    int r = h2d(s, s->X, X, s->dim.X());
    if (!r) r = h2d(s, s->U, U, s->dim.U());
    if (!r && PI) r = h2d(s, s->PI, PI, s->dim.PI());
    return r;
}

int qsp_solve(qsp_solver* s) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_solve: null handle");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, "qsp_solve: no shapes set");
    HIPCHK(hipSetDevice(s->o.device));
    SolveArgs a = make_args(s);
    return run_timed(s, a);
}

int qsp_get_u0(qsp_solver* s, double* u0) { return get_array(s, "qsp_get_u0", u0, &qsp_solver::u0, &Dims::u0); }
// X, U, PI: after a controller solve the shifted warm start
int qsp_get_x(qsp_solver* s, double* X) { return get_array(s, "qsp_get_x", X, &qsp_solver::Xo, &Dims::X, &qsp_solver::X); }
int qsp_get_u(qsp_solver* s, double* U) { return get_array(s, "qsp_get_u", U, &qsp_solver::Uo, &Dims::U, &qsp_solver::U); }
int qsp_get_pi(qsp_solver* s, double* PI) { return get_array(s, "qsp_get_pi", PI, &qsp_solver::PIo, &Dims::PI, &qsp_solver::PI); }
int qsp_get_cost(qsp_solver* s, double* c) { return get_array(s, "qsp_get_cost", c, &qsp_solver::cost, &Dims::lane); }
int qsp_get_status(qsp_solver* s, int32_t* st) { return get_array(s, "qsp_get_status", st, &qsp_solver::status, &Dims::lane); }
int qsp_get_sqp_iter(qsp_solver* s, int32_t* it) { return get_array(s, "qsp_get_sqp_iter", it, &qsp_solver::sqp_iter, &Dims::lane); }
int qsp_get_qp_iter(qsp_solver* s, int32_t* it) { return get_array(s, "qsp_get_qp_iter", it, &qsp_solver::qp_iter, &Dims::lane); }
int qsp_get_qp_capped(qsp_solver* s, int32_t* c) { return get_array(s, "qsp_get_qp_capped", c, &qsp_solver::qp_capped, &Dims::lane); }
int qsp_get_qp_stalled(qsp_solver* s, int32_t* c) { return get_array(s, "qsp_get_qp_stalled", c, &qsp_solver::qp_stalled, &Dims::lane); }
int qsp_get_residuals(qsp_solver* s, double* res) {
    if (!s || !res) return fail(QSP_ERR_ARG, "qsp_get_residuals: null argument");
    if (s->o.nlp_mode != QSP_NLP_SQP_MERIT || !s->wres.data())
        return fail(QSP_ERR_STATE, "qsp_get_residuals: nlp_mode 1 (SQP) only");
    return get_array(s, "qsp_get_residuals", res, &qsp_solver::wres, &Dims::res);
}
int qsp_get_time_tot(qsp_solver* s, double* ms) {
    if (!s || !ms) return fail(QSP_ERR_ARG, "qsp_get_time_tot: null argument");
    *ms = (double)s->last_ms;
    return QSP_OK;
}

int qsp_get_dims(const qsp_solver* s, int32_t* N, int32_t* B) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_get_dims: null handle");
    if (N) *N = s->o.N;
    if (B) *B = s->o.batch;
    return QSP_OK;
}

int qsp_set_yref_stage(qsp_solver* s, int32_t k, const double* y) {
    if (!s || !y) return fail(QSP_ERR_ARG, "qsp_set_yref_stage: null argument");
    if (k < 0 || k >= s->o.N) return fail(QSP_ERR_ARG, "qsp_set_yref_stage: stage out of range 0..N-1");
    HIPCHK(hipSetDevice(s->o.device));
    // column k of every lane's N x 6 block: a strided copy (B rows of 6 doubles)
    const size_t row = 6 * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(s->yref.data() + (size_t)k * 6, s->dim.N * row, y, row, row, s->dim.B,
                            hipMemcpyHostToDevice, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    s->have_yref = true;
    return QSP_OK;
}

int qsp_set_yref_e(qsp_solver* s, const double* y_e) {
    const int r = set_array(s, "qsp_set_yref_e", y_e, &qsp_solver::yref_e, &Dims::yref_e);
    if (!r) s->have_yref = true;
    return r;
}

int qsp_set_init_x(qsp_solver* s, const double* X) { return set_array(s, "qsp_set_init_x", X, &qsp_solver::X, &Dims::X); }
int qsp_set_init_u(qsp_solver* s, const double* U) { return set_array(s, "qsp_set_init_u", U, &qsp_solver::U, &Dims::U); }
int qsp_set_init_pi(qsp_solver* s, const double* PI) { return set_array(s, "qsp_set_init_pi", PI, &qsp_solver::PI, &Dims::PI); }

int qsp_set_timing(qsp_solver* s, int32_t on) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_set_timing: null handle");
    int r = qsp_set_kernel_timing(s, on ? 1 : 0);
    if (r) return r;
    s->auto_timing = on != 0;
    return QSP_OK;
}

int qsp_get_timings(qsp_solver* s, double* time_tot, double* time_lin, double* time_qp_sol) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_get_timings: null handle");
    if (time_tot) *time_tot = s->last_ms * 1e-3;
    double lin = NAN, qp = NAN;
    if (s->auto_timing && !s->kev_solves.empty()) {
        double ms[4];
        int32_t n[4];
        HIPCHK(hipSetDevice(s->o.device));
        const int r = kernel_times_of(s, ms, n);   // the last solve's events stay readable
        if (r) return r;
        lin = ms[1] * 1e-3;
        qp = ms[2] * 1e-3;
    }
    if (time_lin) *time_lin = lin;
    if (time_qp_sol) *time_qp_sol = qp;
    return QSP_OK;
}

// ------------------------------------------------------ controller level
// the reference table of T rows, shared (T x 6) or one per lane (B x T x 6)
static int set_traj(qsp_solver* s, const char* who, const double* traj, int32_t T, bool per_lane) {
    if (!s || !traj || T < 1) return fail(QSP_ERR_ARG, std::string(who) + ": bad argument");
    const int r = h2d_grow(s, s->traj, traj, per_lane ? s->dim.traj_lanes(T) : Dims::traj(T));
    if (r) return r;
    s->T = T;
    s->have_traj = true;
    s->traj_per_lane = per_lane;
    return QSP_OK;
}

int qsp_set_reference_trajectory(qsp_solver* s, const double* traj, int32_t T) {
    return set_traj(s, "qsp_set_reference_trajectory", traj, T, false);
}

int qsp_set_reference_trajectories(qsp_solver* s, const double* traj, int32_t T) {
    return set_traj(s, "qsp_set_reference_trajectories", traj, T, true);
}

int qsp_gen_straight_lines(qsp_solver* s, const double* x0, const double* xf, double t0, double tf,
                           int32_t auto_angle, int32_t* T_out) {
    if (!s || !x0 || !xf || !(tf > t0) || t0 < 0.0) return fail(QSP_ERR_ARG, "qsp_gen_straight_lines: bad argument");
    const size_t B = s->o.batch;
    // MATLAB t0:Ts:tf
    const int32_t T = (int32_t)std::floor((tf - t0) / s->o.Ts + 1e-9) + 1;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const double* d0 = st.in(x0, B * 3);
    const double* d1 = st.in(xf, B * 3);
    if (st.err) return st.err;
    HIPCHK(s->traj.ensure(s->dim.traj_lanes(T)));
    HIPCHK(launch_straight_lines((int)B, T, d0, d1, t0, tf, s->o.Ts, auto_angle, s->traj.data(), s->stream));
    if (st.finish()) return st.err;
    s->T = T;
    s->have_traj = true;
    s->traj_per_lane = true;
    if (T_out) *T_out = T;
    return QSP_OK;
}

void qsp_default_waypoint_opts(qsp_waypoint_opts* o) {
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(qsp_waypoint_opts);
    o->law = QSP_WP_LAW_CONSTANT_SPEED;
    o->yaw = QSP_WP_YAW_HEADING;
}

// TrajectoryGenerator.waypoints_gen / waypoint_gen_fixed_angle per lane.  Everything that is O(B K) happens
// here, validation first, in plain IEEE operations (the library is built with -ffp-contract=off): segment
// durations, arrival times or row counts, the yaw of each segment, the lanes' row counts.  waypoints_kernel
// fills the B x T rows from that.
int qsp_gen_waypoints(qsp_solver* s, const qsp_waypoint_opts* o, int32_t K, const double* wp, const int32_t* n_wp,
                      const double* vel, const double* theta, const double* s_ref, int32_t* T_out, int32_t* T_lane) {
    const std::string w("qsp_gen_waypoints");
    if (!s || !o || !wp || !vel) return fail(QSP_ERR_ARG, w + ": null argument");
    if (o->struct_size != (int32_t)sizeof(qsp_waypoint_opts))
        return fail(QSP_ERR_ARG, w + ": qsp_waypoint_opts.struct_size != sizeof(qsp_waypoint_opts) (stale layout?)");
    if (o->law != QSP_WP_LAW_CONSTANT_SPEED && o->law != QSP_WP_LAW_SEGMENT_LINSPACE)
        return fail(QSP_ERR_ARG, w + ": unknown law");
    if (o->yaw < QSP_WP_YAW_HEADING || o->yaw > QSP_WP_YAW_FIXED) return fail(QSP_ERR_ARG, w + ": unknown yaw");
    if (K < 2 || K > QSP_MAX_WAYPOINTS) return fail(QSP_ERR_ARG, w + ": K outside 2..QSP_MAX_WAYPOINTS");
    if (o->yaw == QSP_WP_YAW_FIXED && !theta) return fail(QSP_ERR_ARG, w + ": QSP_WP_YAW_FIXED needs theta");
    const size_t B = s->o.batch, Ks = (size_t)K;
    const double Ts = s->o.Ts, two_pi = 2.0 * M_PI;
    const double max_rows = 16777216.0;   // 2^24 samples per lane: every count below is an exact int32
    std::vector<int32_t> nw(B), brk(B * Ks, 0), Tl(B);
    std::vector<double> knot(B * Ks, 0.0), yaw(B * Ks, 0.0);
    int32_t T = 1;
    for (size_t i = 0; i < B; ++i) {
        const int32_t n = n_wp ? n_wp[i] : K;
        if (n < 2 || n > K) return fail(QSP_ERR_ARG, w + ": n_wp outside 2..K");
        nw[i] = n;
        const double* p = wp + i * Ks * 2;
        for (int32_t k = 0; k < 2 * n; ++k)
            if (!std::isfinite(p[k])) return fail(QSP_ERR_ARG, w + ": waypoint not finite");
        if (o->yaw == QSP_WP_YAW_FIXED && !std::isfinite(theta[i])) return fail(QSP_ERR_ARG, w + ": theta not finite");
        if (s_ref && !std::isfinite(s_ref[i])) return fail(QSP_ERR_ARG, w + ": s_ref not finite");
        double* tk = knot.data() + i * Ks;
        double* yk = yaw.data() + i * Ks;
        int32_t* ck = brk.data() + i * Ks;
        double h_prev = 0.0;
        for (int32_t k = 0; k + 1 < n; ++k) {
            const double v = vel[i * (Ks - 1) + k];
            if (!(std::isfinite(v) && v > 0.0)) return fail(QSP_ERR_ARG, w + ": vel must be finite and > 0");
            const double dx = p[2 * k + 2] - p[2 * k], dy = p[2 * k + 3] - p[2 * k + 1];
            const double d = std::sqrt(dx * dx + dy * dy) / v;
            if (!std::isfinite(d)) return fail(QSP_ERR_ARG, w + ": segment duration not finite");
            if (o->law == QSP_WP_LAW_CONSTANT_SPEED) {
                if (dx == 0.0 && dy == 0.0)
                    return fail(QSP_ERR_ARG, w + ": two consecutive waypoints are equal (constant speed)");
                tk[k + 1] = tk[k] + d;
                if (!(tk[k + 1] > tk[k]))
                    return fail(QSP_ERR_ARG, w + ": a segment too short for its arrival time to advance");
                if (!(tk[k + 1] / Ts < max_rows)) return fail(QSP_ERR_ARG, w + ": more than 2^24 samples");
            } else {
                const double rows = std::floor(d / Ts + 1e-9);   // the count of (a+Ts):Ts:(a+d)
                if (!(rows + (double)ck[k] < max_rows)) return fail(QSP_ERR_ARG, w + ": more than 2^24 samples");
                ck[k + 1] = ck[k] + (int32_t)rows;
            }
            const double h = std::atan2(dy, dx);
            if (o->yaw == QSP_WP_YAW_FIXED) {
                yk[k] = theta[i];
            } else if (o->yaw == QSP_WP_YAW_HEADING || k == 0) {
                yk[k] = h;
            } else {
                double dl = h - h_prev;
                dl -= two_pi * std::rint(dl / two_pi);
                yk[k] = yk[k - 1] + dl;
            }
            h_prev = h;
        }
        // MATLAB 0:Ts:t_end, as qsp_gen_straight_lines counts; the linspace law: row 0 and every segment's rows
        Tl[i] = o->law == QSP_WP_LAW_CONSTANT_SPEED ? (int32_t)std::floor(tk[n - 1] / Ts + 1e-9) + 1 : 1 + ck[n - 1];
        T = Tl[i] > T ? Tl[i] : T;
    }
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    WaypointArgs a;
    std::memset(&a, 0, sizeof a);
    a.B = (int32_t)B;
    a.T = T;
    a.K = K;
    a.law = o->law;
    a.Ts = Ts;
    a.wp = st.in(wp, B * Ks * 2);
    a.n_wp = st.in(nw.data(), B);
    a.knot = st.in(knot.data(), B * Ks);
    a.brk = st.in(brk.data(), B * Ks);
    a.yaw = st.in(yaw.data(), B * Ks);
    a.s_ref = st.in(s_ref, B);
    a.T_lane = st.in(Tl.data(), B);
    if (st.err) return st.err;
    const hipError_t grown = s->traj.ensure(s->dim.traj_lanes(T));
    if (grown != hipSuccess) s->have_traj = false;   // a failed growth has freed the table that was installed
    HIPCHK(grown);
    a.traj = s->traj.data();
    HIPCHK(launch_waypoints(a, s->stream));
    if (st.finish()) return st.err;
    s->T = T;
    s->have_traj = true;
    s->traj_per_lane = true;
    if (T_out) *T_out = T;
    if (T_lane) std::memcpy(T_lane, Tl.data(), B * sizeof(int32_t));
    return QSP_OK;
}

int qsp_get_reference_trajectories(qsp_solver* s, double* traj) {
    if (!s || !traj) return fail(QSP_ERR_ARG, "qsp_get_reference_trajectories: null argument");
    if (!s->have_traj) return fail(QSP_ERR_STATE, "qsp_get_reference_trajectories: no reference trajectory");
    return d2h(s, traj, s->traj, s->traj_per_lane ? s->dim.traj_lanes(s->T) : Dims::traj(s->T));
}

int qsp_controller_reset(qsp_solver* s) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_controller_reset: null handle");
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(s->warm_valid.fill(s->stream, 0, s->dim.lane()));
    HIPCHK(hipStreamSynchronize(s->stream));
    return QSP_OK;
}

int qsp_controller_solve(qsp_solver* s, const double* x0, const int32_t* index_time) {
    if (!s || !x0 || !index_time) return fail(QSP_ERR_ARG, "qsp_controller_solve: null argument");
    if (!s->have_traj) return fail(QSP_ERR_STATE, "qsp_controller_solve: no reference trajectory");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, "qsp_controller_solve: no shapes set");
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(s->index_time.ensure(s->dim.lane()));
    HIPCHK(s->x0.upload(s->stream, x0, s->dim.x0()));
    HIPCHK(s->index_time.upload(s->stream, index_time, s->dim.lane()));
    HIPCHK(launch_controller_step(s, 0));
    return run_timed(s, controller_args(s));
}

// ------------------------------------------------------- delay compensation
int qsp_set_delay_comp(qsp_solver* s, double delay) {
    if (!s || !(delay >= 0.0)) return fail(QSP_ERR_ARG, "qsp_set_delay_comp: delay must be >= 0");
    const double cols = std::ceil(delay / s->o.Ts);   // delay_buff_comp = ceil(delay / sample_time) (:108)
    if (cols > 4096.0) return fail(QSP_ERR_ARG, "qsp_set_delay_comp: more than 4096 delay samples");
    HIPCHK(hipSetDevice(s->o.device));
    s->D = (int32_t)cols;
    const size_t n = s->dim.delay(s->D > 0 ? s->D : 1);
    HIPCHK(s->ubc.ensure(n));
    HIPCHK(s->ubc.fill(s->stream, 0, n));   // u_buff_contr = zeros (:109)
    HIPCHK(hipStreamSynchronize(s->stream));
    return QSP_OK;
}

int qsp_get_delay_comp(qsp_solver* s, int32_t* cols) {
    if (!s || !cols) return fail(QSP_ERR_ARG, "qsp_get_delay_comp: null argument");
    *cols = s->D;
    return QSP_OK;
}

static ClosedLoopArgs cl_args(qsp_solver* s) {
    ClosedLoopArgs a;
    std::memset(&a, 0, sizeof a);
    a.shapes = s->shapes.data();
    a.n_shapes = s->n_shapes;
    a.sid = s->shape_id.data();
    a.B = s->o.batch;
    a.Ts = s->o.Ts;
    a.D = s->D;
    a.ubc = s->ubc.data();
    // the plant's own model, where one is installed (else nullptr: the controller's)
    if (s->n_pshapes > 0) {
        a.pshapes = s->pshapes.data();
        a.n_pshapes = s->n_pshapes;
        a.psid = s->has_pids ? s->pshape_id.data() : nullptr;
    }
    a.pmu = s->has_pmu ? s->pmu.data() : nullptr;
    a.pc = s->has_pc ? s->pc.data() : nullptr;
    return a;
}

// The installed generator as the kernels take it (gen.on = 0 without one), and its per-lane scale
static SimNoiseGen noise_gen(const qsp_solver* s) {
    SimNoiseGen g;
    std::memset(&g, 0, sizeof g);
    if (!s->sn_on) return g;
    g.on = 1;
    g.stream = s->sn.stream;
    g.key0 = (uint32_t)s->sn.seed;
    g.key1 = (uint32_t)(s->sn.seed >> 32);
    g.lane0 = (uint32_t)s->sn.lane_offset;
    g.step0 = (uint64_t)s->sn.step_offset;
    std::memcpy(g.sigma, s->sn.sigma, sizeof g.sigma);
    return g;
}
static const double* noise_scale(const qsp_solver* s) { return s->sn_on && s->sn_has_scale ? s->sn_scale.data() : nullptr; }
static const char* const NOISE_TWICE = ": a noise table while a sim_noise generator is installed is ambiguous "
                                       "(pass noise = NULL, or qsp_clear_sim_noise first)";

int qsp_delay_buffer_sim(qsp_solver* s, const double* x, double* x_sim) {
    if (!s || !x || !x_sim) return fail(QSP_ERR_ARG, "qsp_delay_buffer_sim: null argument");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, "qsp_delay_buffer_sim: no shapes set");
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    ClosedLoopArgs a = cl_args(s);
    a.x = st.in(x, s->dim.x0());
    a.xs = st.out(x_sim, s->dim.x0());
    if (st.err) return st.err;
    HIPCHK(launch_delay_sim(a, s->stream));
    return st.finish();
}

int qsp_delay_buffer_push(qsp_solver* s, const double* u) {
    if (!s || !u) return fail(QSP_ERR_ARG, "qsp_delay_buffer_push: null argument");
    if (s->D == 0) return QSP_OK;
    const size_t B = s->o.batch, D = (size_t)s->D;
    std::vector<double> h(s->dim.delay(D));
    int r = d2h(s, h.data(), s->ubc, h.size());
    if (r) return r;
    for (size_t i = 0; i < B; ++i) {   // u_buff_contr = [u, u_buff_contr(:, 1:end-1)]  (helper.m:255)
        double* b = h.data() + i * D * 2;
        std::memmove(b + 2, b, (D - 1) * 2 * sizeof(double));
        b[0] = u[2 * i];
        b[1] = u[2 * i + 1];
    }
    return h2d(s, s->ubc, h.data(), h.size());
}

static_assert(CL_NMETRICS == QSP_CL_NMETRICS, "metric columns of the kernel and of the header");

// closed_loop_matlab's loop (helper.m:195-322) on the stream, for both front ends: with trajectories
// (qsp_closed_loop_ex: B x n_steps logs in s->cl_xtraj, cl_utraj, cl_straj and cl_xsim) or with the per-lane metric
// accumulators alone (qsp_closed_loop_metrics: s->cl_metrics, nothing of size B x n_steps).  The
// final plant state is left in s->cl_x, the last status in s->status; the caller copies out and
// synchronises.
static int closed_loop_run(qsp_solver* s, const char* who, const qsp_closed_loop_opts* o, const double* x0,
                           const int32_t* index0, int32_t n_steps, const double* noise, bool want_traj,
                           bool want_xsim, bool want_metrics) {
    const std::string w(who);
    if (noise && s->sn_on) return fail(QSP_ERR_ARG, w + NOISE_TWICE);
    if (!s->have_traj) return fail(QSP_ERR_STATE, w + ": no reference trajectory");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, w + ": no shapes set");
    const double plant_delay = o ? o->plant_delay : 0.0;
    if (!(plant_delay >= 0.0) || std::ceil(plant_delay / s->o.Ts) > 4096.0)
        return fail(QSP_ERR_ARG, w + ": plant_delay must be in [0, 4096 Ts]");
    if (o && o->disturbance && o->t_dist < 1) return fail(QSP_ERR_ARG, w + ": t_dist must be >= 1");
    const Dims& d = s->dim;
    const size_t T = (size_t)n_steps;
    const int Dp = (int)std::ceil(plant_delay / s->o.Ts);   // delay_buff_plant (helper.m:211)
    HIPCHK(hipSetDevice(s->o.device));
    if (want_traj) {
        HIPCHK(s->cl_xtraj.ensure(d.cl_X(T)));
        HIPCHK(s->cl_utraj.ensure(d.cl_U(T)));
        HIPCHK(s->cl_straj.ensure(d.cl_status(T)));
    }
    if (want_xsim) HIPCHK(s->cl_xsim.ensure(d.cl_Xsim(T)));
    if (want_metrics) HIPCHK(s->cl_metrics.ensure(d.metrics()));
    if (noise) HIPCHK(s->cl_noise.ensure(d.cl_noise(T)));
    HIPCHK(s->cl_x.ensure(d.x0()));
    HIPCHK(s->ubp.ensure(d.delay(Dp > 0 ? Dp : 1)));
    if (s->D > 0) HIPCHK(s->ubc.ensure(d.delay(s->D)));
    HIPCHK(s->index_time.ensure(d.lane()));
    HIPCHK(s->cl_x.upload(s->stream, x0, d.x0()));
    HIPCHK(s->index_time.upload(s->stream, index0, d.lane()));
    if (noise) HIPCHK(s->cl_noise.upload(s->stream, noise, d.cl_noise(T)));
    const bool dist = o && o->disturbance;
    if (dist && o->amplitude) {
        HIPCHK(s->cl_amp.ensure(d.lane()));
        HIPCHK(s->cl_amp.upload(s->stream, o->amplitude, d.lane()));
    }
    // initial_condition_update -> clear_variables: the first solve is a cold start (main.m:79);
    // the plant's buffer starts at zero (closed_loop_matlab's u_buff_plant, helper.m:211-212); the
    // controller's u_buff_contr is left as it is: the reference zeroes it only in set_delay_comp
    // (NMPC_controller.m:106-110; qsp_set_delay_comp), so a second run continues from the first's
    HIPCHK(s->warm_valid.fill(s->stream, 0, d.lane()));
    if (Dp > 0) HIPCHK(s->ubp.fill(s->stream, 0, d.delay(Dp)));
    if (want_metrics) HIPCHK(s->cl_metrics.fill(s->stream, 0, d.metrics()));
    ClosedLoopArgs c = cl_args(s);
    c.n_steps = n_steps;
    c.x = s->cl_x.data();
    c.xs = s->x0.data();                 // the solver's x0 (constr_x0)
    c.noise = noise ? s->cl_noise.data() : nullptr;
    c.gen = noise_gen(s);                // drawn in closed_loop_pre_kernel: cl_noise is not touched
    c.lane_scale = noise_scale(s);
    c.dist_step = dist ? o->t_dist : 0;
    c.dist_amp = (dist && o->amplitude) ? s->cl_amp.data() : nullptr;
    c.Dp = Dp;
    c.ubp = s->ubp.data();
    c.u0 = s->u0.data();
    c.status = s->status.data();
    c.Xtraj = want_traj ? s->cl_xtraj.data() : nullptr;
    c.Xsim = want_xsim ? s->cl_xsim.data() : nullptr;
    c.Utraj = want_traj ? s->cl_utraj.data() : nullptr;
    c.Straj = want_traj ? s->cl_straj.data() : nullptr;
    if (want_metrics) {
        c.metrics = s->cl_metrics.data();
        c.mtraj = s->traj.data();
        c.mT = s->T;
        c.mper_lane = s->traj_per_lane ? 1 : 0;
        c.index0 = s->index_time.data();
        c.s_lo = s->p.lh[0];
        c.s_hi = s->p.uh[0];
    }
    HIPCHK(hipEventRecord(s->ev0, s->stream));
    const SolveArgs a = controller_args(s);
    for (int32_t t = 0; t < n_steps; ++t) {
        HIPCHK(launch_closed_loop_pre(c, t, s->stream));                       // disturbance, noise, delay_buffer_sim
        HIPCHK(launch_controller_step(s, t + s->D));                           // y_ref for index0 + t + D
        HIPCHK(launch_sqp(a, s->S, s->stream, take_kernel_events(s), sqp_split(s)));   // NMPC_controller.solve
        HIPCHK(launch_plant(c, t, s->stream));                                 // buffers, plant step, logs, metrics
    }
    HIPCHK(hipEventRecord(s->ev1, s->stream));
    return QSP_OK;
}

static int closed_loop_done(qsp_solver* s) {
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipEventElapsedTime(&s->last_ms, s->ev0, s->ev1));
    s->solved = true;
    return QSP_OK;
}

int qsp_closed_loop_ex(qsp_solver* s, const qsp_closed_loop_opts* o, const double* x0, const int32_t* index0,
                       int32_t n_steps, const double* noise, double* X_traj, double* X_sim, double* U_traj,
                       int32_t* status_traj) {
    if (!s || !x0 || !index0 || !X_traj || !U_traj || n_steps < 1)
        return fail(QSP_ERR_ARG, "qsp_closed_loop: bad argument");
    const int r = closed_loop_run(s, "qsp_closed_loop", o, x0, index0, n_steps, noise, true, X_sim != nullptr, false);
    if (r) return r;
    const size_t T = (size_t)n_steps;
    HIPCHK(s->cl_xtraj.download(s->stream, X_traj, s->dim.cl_X(T)));
    HIPCHK(s->cl_utraj.download(s->stream, U_traj, s->dim.cl_U(T)));
    if (X_sim) HIPCHK(s->cl_xsim.download(s->stream, X_sim, s->dim.cl_Xsim(T)));
    if (status_traj) HIPCHK(s->cl_straj.download(s->stream, status_traj, s->dim.cl_status(T)));
    return closed_loop_done(s);
}

int qsp_closed_loop_metrics(qsp_solver* s, const qsp_closed_loop_opts* o, const double* x0, const int32_t* index0,
                            int32_t n_steps, const double* noise, double* metrics, double* x_end,
                            int32_t* status_last) {
    if (!s || !x0 || !index0 || !metrics || n_steps < 1)
        return fail(QSP_ERR_ARG, "qsp_closed_loop_metrics: bad argument");
    const int r = closed_loop_run(s, "qsp_closed_loop_metrics", o, x0, index0, n_steps, noise, false, false, true);
    if (r) return r;
    HIPCHK(s->cl_metrics.download(s->stream, metrics, s->dim.metrics()));
    if (x_end) HIPCHK(s->cl_x.download(s->stream, x_end, s->dim.x0()));
    if (status_last) HIPCHK(s->status.download(s->stream, status_last, s->dim.lane()));
    return closed_loop_done(s);
}

int qsp_closed_loop(qsp_solver* s, const double* x0, const int32_t* index0, int32_t n_steps, const double* noise,
                    double* X_traj, double* U_traj, int32_t* status_traj) {
    return qsp_closed_loop_ex(s, nullptr, x0, index0, n_steps, noise, X_traj, nullptr, U_traj, status_traj);
}

int qsp_reproject_contact(qsp_solver* s, int32_t n, const int32_t* sid, const double* px, const double* py,
                          const double* s0, double* s_out) {
    if (!s || n < 1 || !sid || !px || !py || !s0 || !s_out) return fail(QSP_ERR_ARG, "qsp_reproject_contact: bad argument");
    int r = check_ids(s, n, sid);
    if (r) return r;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const int32_t* d_sid = st.in(sid, n);
    const double *d_px = st.in(px, n), *d_py = st.in(py, n), *d_s0 = st.in(s0, n);
    double* d_s = st.out(s_out, n);
    if (st.err) return st.err;
    HIPCHK(launch_reproject(s->shapes.data(), s->n_shapes, d_sid, n, d_px, d_py, d_s0, d_s, s->stream));
    return st.finish();
}

// ------------------------------------------------------ device fast path
int qsp_solve_device(qsp_solver* s, const qsp_device_io* io, void* stream) {
    if (!s || !io) return fail(QSP_ERR_ARG, "qsp_solve_device: null argument");
    if (!io->x0 || !io->yref || !io->yref_e || !io->X_in || !io->U_in || !io->u0 || !io->X_out || !io->U_out ||
        !io->PI_out || !io->status || !io->cost)
        return fail(QSP_ERR_ARG, "qsp_solve_device: missing device pointer");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, "qsp_solve_device: no shapes set");
    HIPCHK(hipSetDevice(s->o.device));
    SolveArgs a = make_args(s);
    a.x0 = io->x0;
    a.yref = io->yref;
    a.yref_e = io->yref_e;
    a.X_in = io->X_in;
    a.U_in = io->U_in;
    a.PI_in = io->PI_in;
    a.shape_id = io->shape_id ? io->shape_id : s->shape_id.data();
    a.u0 = io->u0;
    a.X_out = io->X_out;
    a.U_out = io->U_out;
    a.PI_out = io->PI_out;
    a.status = io->status;
    a.cost = io->cost;
    if (io->controller) {
        a.flags |= QSP_FLAG_CONTROLLER | QSP_FLAG_SHIFT;
        a.warm_valid = io->warm_valid;
    }
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    HIPCHK(launch_sqp(a, s->S, st, take_kernel_events(s), sqp_split(s)));
    s->solved = true;
    return QSP_OK;
}

int qsp_set_stream_parts(qsp_solver* s, int32_t parts) {
    if (!s || parts < 0 || parts > SQP_MAX_PARTS)
        return fail(QSP_ERR_ARG, "qsp_set_stream_parts: parts must be 0 (auto), 1 or 2");
    s->parts_req = parts;
    return QSP_OK;
}

int qsp_get_stream_parts(qsp_solver* s, int32_t* parts) {
    if (!s || !parts) return fail(QSP_ERR_ARG, "qsp_get_stream_parts: null argument");
    *parts = sqp_split(s)->parts;
    return QSP_OK;
}

int qsp_set_kernel_timing(qsp_solver* s, int32_t max_solves) {
    if (!s || max_solves < 0) return fail(QSP_ERR_ARG, "qsp_set_kernel_timing: bad argument");
    HIPCHK(hipSetDevice(s->o.device));
    for (hipEvent_t e : s->kev) HIPCHK(hipEventDestroy(e));
    s->kev.clear();
    s->kev_solves.clear();
    s->kev_split.clear();
    s->kev_used = 0;
    const size_t n = (size_t)max_solves * (2 * s->o.sqp_iters + 3);
    for (size_t i = 0; i < n; ++i) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        s->kev.push_back(e);
    }
    return QSP_OK;
}

// summed kernel times of the recorded solves (events kept: the pool is re-armed by the caller)
static int kernel_times_of(qsp_solver* s, double* ms, int32_t* launches) {
    for (int k = 0; k < 4; ++k) { ms[k] = 0.0; launches[k] = 0; }
    const int K = s->o.sqp_iters;
    for (size_t j = 0; j < s->kev_solves.size(); ++j) {
        hipEvent_t* e = s->kev.data() + s->kev_solves[j];
        HIPCHK(hipEventSynchronize(e[2 * K + 2]));
        float t;
        HIPCHK(hipEventElapsedTime(&t, e[0], e[1])); ms[0] += t; launches[0] += 1;
        if (s->kev_split[j]) {
            // two-stream loop: timed as a whole, one "launch" per SQP iteration (sorts included)
            HIPCHK(hipEventElapsedTime(&t, e[1], e[2 * K + 1])); ms[2] += t; launches[2] += K;
        } else
        for (int it = 0; it < K; ++it) {
            HIPCHK(hipEventElapsedTime(&t, e[1 + 2 * it], e[2 + 2 * it])); ms[1] += t; launches[1] += 1;
            HIPCHK(hipEventElapsedTime(&t, e[2 + 2 * it], e[3 + 2 * it])); ms[2] += t; launches[2] += 1;
        }
        HIPCHK(hipEventElapsedTime(&t, e[2 * K + 1], e[2 * K + 2])); ms[3] += t; launches[3] += 1;
    }
    return QSP_OK;
}

int qsp_get_kernel_times(qsp_solver* s, double* ms, int32_t* launches) {
    if (!s || !ms || !launches) return fail(QSP_ERR_ARG, "qsp_get_kernel_times: null argument");
    HIPCHK(hipSetDevice(s->o.device));
    const int r = kernel_times_of(s, ms, launches);
    if (r) return r;
    s->kev_solves.clear();
    s->kev_split.clear();
    s->kev_used = 0;
    return QSP_OK;
}

int qsp_synchronize(qsp_solver* s) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_synchronize: null handle");
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(hipStreamSynchronize(s->stream));
    return QSP_OK;
}

// ------------------------------------------------------- building blocks
int qsp_eval_spline(qsp_solver* s, int32_t n, const int32_t* sid, const double* sig, double* C, double* D, double* Dd,
                    double* kappa) {
    if (!s || !sid || !sig || !C || !D || !Dd || !kappa || n < 1) return fail(QSP_ERR_ARG, "qsp_eval_spline: bad argument");
    int r = check_ids(s, n, sid);
    if (r) return r;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const int32_t* d_sid = st.in(sid, n);
    const double* d_sig = st.in(sig, n);
    double *dC = st.out(C, (size_t)2 * n), *dD = st.out(D, (size_t)2 * n), *dDd = st.out(Dd, (size_t)2 * n);
    double* dk = st.out(kappa, n);
    if (st.err) return st.err;
    HIPCHK(launch_spline(s->shapes.data(), d_sid, n, d_sig, dC, dD, dDd, dk, s->stream));
    return st.finish();
}

int qsp_eval_dynamics(qsp_solver* s, int32_t n, const int32_t* sid, const double* x, const double* u, double* f,
                      double* J) {
    if (!s || !sid || !x || !u || !f || !J || n < 1) return fail(QSP_ERR_ARG, "qsp_eval_dynamics: bad argument");
    int r = check_ids(s, n, sid);
    if (r) return r;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const int32_t* d_sid = st.in(sid, n);
    const double *dx = st.in(x, (size_t)4 * n), *du = st.in(u, (size_t)2 * n);
    double *df = st.out(f, (size_t)4 * n), *dJ = st.out(J, (size_t)24 * n);
    if (st.err) return st.err;
    HIPCHK(launch_dynamics(s->shapes.data(), d_sid, n, dx, du, df, dJ, s->stream));
    return st.finish();
}

int qsp_eval_rk4(qsp_solver* s, int32_t n, const int32_t* sid, double h, const double* x, const double* u, double* xn,
                 double* A, double* B) {
    if (!s || !sid || !x || !u || !xn || !A || !B || n < 1) return fail(QSP_ERR_ARG, "qsp_eval_rk4: bad argument");
    int r = check_ids(s, n, sid);
    if (r) return r;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const int32_t* d_sid = st.in(sid, n);
    const double *dx = st.in(x, (size_t)4 * n), *du = st.in(u, (size_t)2 * n);
    double *dxn = st.out(xn, (size_t)4 * n), *dA = st.out(A, (size_t)16 * n), *dB = st.out(B, (size_t)8 * n);
    if (st.err) return st.err;
    HIPCHK(launch_rk4(s->shapes.data(), d_sid, n, h, dx, du, dxn, dA, dB, s->stream));
    return st.finish();
}

int qsp_eval_vbound(qsp_solver* s, int32_t n, const int32_t* sid, const double* sv, double* vb) {
    if (!s || !sid || !sv || !vb || n < 1) return fail(QSP_ERR_ARG, "qsp_eval_vbound: bad argument");
    int r = check_ids(s, n, sid);
    if (r) return r;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const int32_t* d_sid = st.in(sid, n);
    const double* ds = st.in(sv, n);
    double* dvb = st.out(vb, n);
    if (st.err) return st.err;
    HIPCHK(launch_vbound(s->shapes.data(), d_sid, n, s->p.cp, ds, dvb, s->stream));
    return st.finish();
}

int qsp_qp_solve(qsp_solver* s, int32_t nb, const double* A, const double* B, const double* b, const double* H,
                 const double* g, const double* lo, const double* hi, const double* dx0, double* dx, double* du,
                 double* pi, double* lam, int32_t* iters, int32_t* qp_status) {
    if (!s || nb < 1 || !A || !B || !b || !H || !g || !lo || !hi || !dx0 || !dx || !du || !pi || !lam || !iters)
        return fail(QSP_ERR_ARG, "qsp_qp_solve: bad argument");
    const int N = s->o.N;
    SolveParams p = s->p;
    qp_level_params(p, H, lo, hi);   // bounds in step space lo = lh - v, hi = uh - v with lh = 0, uh = width, v = -lo
    const Dims qd{(size_t)nb, (size_t)N};   // the QPs' own batch
    const size_t tot = qd.stages();
    std::vector<double> lin(qd.lin(), 0.0), X(qd.X()), U(qd.U()), x0(qd.x0());
    for (int l = 0; l < nb; ++l) {   // each lane checked, then packed
        const QpLaneData q(A, B, b, H, g, lo, hi, N, (size_t)l);
        for (int k = 0; k < N; ++k) {
            for (int i = 0; i < 6; ++i)
                if (q.Hk(k)[i] != p.W[i]) return fail(QSP_ERR_ARG, "qsp_qp_solve: stage Hessian must be equal on every stage");
            for (int j = 0; j < 3; ++j) {
                const double w = q.hik(k)[j] - q.lok(k)[j];
                if (std::fabs(w - p.uh[j]) > 1e-12 * (1.0 + std::fabs(w)))
                    return fail(QSP_ERR_ARG, "qsp_qp_solve: bound widths must be equal on every stage");
            }
            if (!QpLaneData::has_structure(q.Ak(k))) return fail(QSP_ERR_ARG, "qsp_qp_solve: A lacks the pusher-slider structure");
        }
        for (int i = 0; i < 4; ++i)
            if (q.Hk(N)[i] != p.We[i]) return fail(QSP_ERR_ARG, "qsp_qp_solve: terminal Hessian must be equal on every lane");
        // pack the workspace on the host: stage data SoA, v = -lo through X/U, x0 - X_0 = dx0
        for (int k = 0; k <= N; ++k) {
            const size_t gi = (size_t)l * (N + 1) + k;
            if (k < N) {
                double av[6];
                QpLaneData::free_entries(q.Ak(k), av);
                for (int f = 0; f < 6; ++f) lin[(L_A + f) * tot + gi] = av[f];
                for (int f = 0; f < 8; ++f) lin[(L_B + f) * tot + gi] = q.Bk(k)[f];
                for (int f = 0; f < 4; ++f) lin[(L_BB + f) * tot + gi] = q.bk(k)[f];
            }
            for (int f = 0; f < (k < N ? 6 : 4); ++f) lin[(L_G + f) * tot + gi] = q.gk(k)[f];
        }
        // dx0 = wx0 - X_0 with X_0 = (0, 0, 0, -lo_s(0))  ->  wx0 = dx0 + X_0
        qp_level_iterate(N, q.lo, dx0 + (size_t)l * 4, X.data() + (size_t)l * (N + 1) * 4, U.data() + (size_t)l * N * 2,
                         x0.data() + (size_t)l * 4);
    }
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    std::vector<int32_t> qst((size_t)nb);
    SolveArgs a;
    std::memset(&a, 0, sizeof a);
    a.p = p;
    a.B = nb;
    a.wlin = st.in(lin.data(), lin.size());
    a.wX = st.in(X.data(), X.size());
    a.wU = st.in(U.data(), U.size());
    a.wx0 = st.in(x0.data(), x0.size());
    a.qp_dx = st.out(dx, qd.X());
    a.qp_du = st.out(du, qd.U());
    a.PI_out = st.out(pi, qd.PI());
    a.qp_lam = st.out(lam, qd.lam());
    a.qp_iter = st.out(iters, qd.lane());
    a.qp_capped = st.out(qst.data(), qd.lane());
    if (st.err) return st.err;
    HIPCHK(launch_qp(a, s->S, s->stream));
    if (st.finish()) return st.err;
    if (qp_status) {
        for (int l = 0; l < nb; ++l)
            qp_status[l] = qp_level_status(p, dx + (size_t)l * (N + 1) * 4, du + (size_t)l * N * 2,
                                           lo + (size_t)l * N * QpLaneData::NBOUND, hi + (size_t)l * N * QpLaneData::NBOUND,
                                           dx0 + (size_t)l * 4, qst[l]);
    }
    return QSP_OK;
}

// Each host entry and its _device twin run one function: the checks, io onto the kernel's argument block,
// the launch.  host: io holds host arrays, which go through the staging pool and are copied back before
// the return, on the handle's stream; else device arrays, used as they are, asynchronous on `stream`.
static const char* missing(bool host) { return host ? ": null argument" : ": missing device pointer"; }
static hipStream_t stream_of(qsp_solver* s, bool host, void* stream) {
    return (host || !stream) ? s->stream : (hipStream_t)stream;
}

// ------------------------------------- KKT residuals recomputed from given numbers
static int eval_kkt_run(qsp_solver* s, const char* who, bool host, const qsp_kkt_io* io, void* stream) {
    const std::string w(who);
    if (!s || !io || !io->X || !io->U || !io->PI || !io->res) return fail(QSP_ERR_ARG, w + missing(host));
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, w + ": no shapes set");
    if ((!io->yref || !io->yref_e) && !s->have_yref)
        return fail(QSP_ERR_STATE, w + ": no references given and none staged on the handle");
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const Dims& dim = s->dim;
    KktNlpArgs a;
    std::memset(&a, 0, sizeof a);
    a.p = s->p;
    a.B = s->o.batch;
    a.pt = point_in(s, st, host, *io, io->yref_e, true);
    a.res = host ? st.out(io->res, dim.res()) : io->res;
    a.parts = host ? st.out(io->parts, dim.kkt_parts()) : io->parts;
    a.stage_res = host ? st.out(io->stage_res, dim.kkt_stage_res()) : io->stage_res;
    if (st.err) return st.err;
    HIPCHK(launch_kkt_nlp(a, stream_of(s, host, stream)));
    return host ? st.finish() : QSP_OK;
}

int qsp_eval_kkt(qsp_solver* s, const double* x0, const double* X, const double* U, const double* PI, const double* LAM,
                 const double* yref, const double* yref_e, double* res, double* parts, double* stage_res) {
    const qsp_kkt_io io = {x0, X, U, PI, LAM, yref, yref_e, nullptr, res, parts, stage_res};
    return eval_kkt_run(s, "qsp_eval_kkt", true, &io, nullptr);
}

int qsp_eval_kkt_device(qsp_solver* s, const qsp_kkt_io* io, void* stream) {
    return eval_kkt_run(s, "qsp_eval_kkt_device", false, io, stream);
}

int qsp_get_lam(qsp_solver* s, double* lam) {
    if (!s || !lam) return fail(QSP_ERR_ARG, "qsp_get_lam: null argument");
    if (s->o.nlp_mode != QSP_NLP_SQP_MERIT || !s->wnlp.data()) return fail(QSP_ERR_STATE, "qsp_get_lam: nlp_mode 1 (SQP) only");
    if (!s->solved) return fail(QSP_ERR_STATE, "qsp_get_lam: no solve yet");
    // the iterate's multipliers live in the SQP's workspace, field-major over (instance, stage 0..N)
    const size_t B = s->dim.B, N = s->dim.N, tot = s->dim.stages();
    std::vector<double> w(6 * tot);
    HIPCHK(hipSetDevice(s->o.device));
    HIPCHK(hipMemcpyAsync(w.data(), s->wnlp.data() + W_LAM * tot, w.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    for (size_t i = 0; i < B; ++i)
        for (size_t k = 0; k < N; ++k)
            for (size_t q = 0; q < 6; ++q) lam[(i * N + k) * 6 + q] = w[q * tot + i * (N + 1) + k];
    return QSP_OK;
}

int qsp_qp_residuals(qsp_solver* s, int32_t nb, const double* A, const double* B, const double* b, const double* H,
                     const double* g, const double* lo, const double* hi, const double* dx0, const double* dx,
                     const double* du, const double* pi, const double* lam, double* res) {
    if (!s || nb < 1 || !A || !B || !b || !H || !g || !lo || !hi || !dx0 || !dx || !du || !pi || !lam || !res)
        return fail(QSP_ERR_ARG, "qsp_qp_residuals: bad argument");
    HIPCHK(hipSetDevice(s->o.device));
    const Dims qd{(size_t)nb, (size_t)s->o.N};   // the QPs' own batch
    Staging st(s);
    KktQpArgs a;
    std::memset(&a, 0, sizeof a);
    a.N = s->o.N;
    a.nb = nb;
    a.s0_bound = s->p.s0_bound;
    a.A = st.in(A, qd.qp_A());
    a.B = st.in(B, qd.qp_B());
    a.b = st.in(b, qd.PI());
    a.H = st.in(H, qd.qp_Hg());
    a.g = st.in(g, qd.qp_Hg());
    a.lo = st.in(lo, qd.qp_bound());
    a.hi = st.in(hi, qd.qp_bound());
    a.pt.x0 = st.in(dx0, qd.x0());
    a.pt.X = st.in(dx, qd.X());
    a.pt.U = st.in(du, qd.U());
    a.pt.PI = st.in(pi, qd.PI());
    a.pt.LAM = st.in(lam, qd.lam());
    a.res = st.out(res, qd.qp_res());
    if (st.err) return st.err;
    HIPCHK(launch_kkt_qp(a, s->stream));
    return st.finish();
}

// ------------------------------------- solution sensitivities du_k/dx0
void qsp_default_sens_opts(qsp_sens_opts* o) {
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(qsp_sens_opts);
    o->s0_bound = -1;
    o->t_floor = 1e-8;
}

// opts (NULL: the defaults) checked and resolved against the handle
static int sens_opts(qsp_solver* s, const qsp_sens_opts* opts, const std::string& w, int32_t& s0_bound, double& t_floor) {
    qsp_sens_opts o;
    qsp_default_sens_opts(&o);
    if (opts) {
        if (opts->struct_size != (int32_t)sizeof(qsp_sens_opts))
            return fail(QSP_ERR_ARG, w + ": qsp_sens_opts.struct_size != sizeof(qsp_sens_opts) (stale layout?)");
        o = *opts;
    }
    if (!(std::isfinite(o.t_floor) && o.t_floor > 0.0)) return fail(QSP_ERR_ARG, w + ": t_floor must be finite and > 0");
    if (o.s0_bound < -1 || o.s0_bound > 1) return fail(QSP_ERR_ARG, w + ": s0_bound must be -1, 0 or 1");
    s0_bound = o.s0_bound < 0 ? s->p.s0_bound : o.s0_bound;
    t_floor = o.t_floor;
    return QSP_OK;
}

// the gains' workspace of a call of dims d that asks for dU
static hipError_t sens_gain_buffer(qsp_solver* s, const double* dU, const Dims& d, double** wK) {
    *wK = nullptr;
    if (!dU) return hipSuccess;
    const hipError_t e = s->wsensK.ensure(d.sens_wK());
    *wK = s->wsensK.data();
    return e;
}

// the outputs of a call of dims d: host arrays through the staging pool, device arrays as they are
static SensOut sens_out(Staging& st, bool host, const Dims& d, double* K0, double* K, double* dU, double* P0, int32_t* flag) {
    if (!host) return {K0, K, dU, P0, flag};
    return {st.out(K0, d.sens_K0()), st.out(K, d.sens_gains()), st.out(dU, d.sens_gains()), st.out(P0, d.sens_P0()),
            st.out(flag, d.lane())};
}

// host entry and _device twin, as eval_kkt_run
static int eval_sens_run(qsp_solver* s, const char* who, bool host, const qsp_sens_opts* opts, const qsp_sens_io* io,
                         void* stream) {
    const std::string w(who);
    if (!s || !io || !io->X || !io->U || !io->K0) return fail(QSP_ERR_ARG, w + missing(host));
    SensNlpArgs a;
    std::memset(&a, 0, sizeof a);
    int r = sens_opts(s, opts, w, a.s0_bound, a.t_floor);
    if (r) return r;
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, w + ": no shapes set");
    const bool implied = !io->LAM && io->PI;
    if (implied && !io->yref && !s->have_yref)
        return fail(QSP_ERR_STATE, w + ": implied multipliers need references, and none are staged on the handle");
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const Dims& dim = s->dim;
    a.pt = point_in(s, st, host, *io, nullptr, implied);
    a.out = sens_out(st, host, dim, io->K0, io->K, io->dU, io->P0, io->flag);
    if (st.err) return st.err;
    HIPCHK(s->wsens.ensure(dim.sens_ws()));
    HIPCHK(sens_gain_buffer(s, a.out.dU, dim, &a.wK));
    a.p = s->p;
    a.B = s->o.batch;
    a.ws = s->wsens.data();
    HIPCHK(launch_sens_nlp(a, stream_of(s, host, stream)));
    return host ? st.finish() : QSP_OK;
}

int qsp_eval_sens(qsp_solver* s, const qsp_sens_opts* opts, const double* x0, const double* X, const double* U,
                  const double* PI, const double* LAM, double* K0, double* K, double* dU, double* P0, int32_t* flag) {
    const qsp_sens_io io = {x0, X, U, PI, LAM, nullptr, nullptr, K0, K, dU, P0, flag};
    return eval_sens_run(s, "qsp_eval_sens", true, opts, &io, nullptr);
}

int qsp_eval_sens_device(qsp_solver* s, const qsp_sens_opts* opts, const qsp_sens_io* io, void* stream) {
    return eval_sens_run(s, "qsp_eval_sens_device", false, opts, io, stream);
}

int qsp_get_sens(qsp_solver* s, const qsp_sens_opts* opts, double* K0, double* K, double* dU, double* P0, int32_t* flag) {
    if (!s || !K0) return fail(QSP_ERR_ARG, "qsp_get_sens: null argument");
    if (!s->solved) return fail(QSP_ERR_STATE, "qsp_get_sens: no solve yet");
    const bool merit = s->o.nlp_mode == QSP_NLP_SQP_MERIT && s->wnlp.data();
    if (s->last_controller && !merit)
        return fail(QSP_ERR_STATE, "qsp_get_sens: after qsp_controller_solve in nlp_mode 0 the handle keeps only the "
                                   "shifted dynamics multipliers");
    // The unshifted final iterate, through the host entry (a getter, not a hot path): X and U from the SQP's
    // workspace, which the epilogue reads and leaves (after qsp_solve the bits of qsp_get_x/u); the
    // bound multipliers are the merit SQP's (qsp_get_lam: never shifted; with them PI is not read), or the
    // implied ones from qsp_get_pi in nlp_mode 0.
    const Dims& dim = s->dim;
    std::vector<double> X(dim.X()), U(dim.U()), PI, LAM;
    int r = d2h(s, X.data(), s->wX, dim.X());
    if (!r) r = d2h(s, U.data(), s->wU, dim.U());
    if (!r && merit) {
        LAM.resize(dim.lam());
        r = qsp_get_lam(s, LAM.data());
    } else if (!r) {
        PI.resize(dim.PI());
        r = qsp_get_pi(s, PI.data());
    }
    if (r) return r;
    const qsp_sens_io io = {nullptr, X.data(), U.data(), PI.empty() ? nullptr : PI.data(),
                            LAM.empty() ? nullptr : LAM.data(), nullptr, nullptr, K0, K, dU, P0, flag};
    return eval_sens_run(s, "qsp_get_sens", true, opts, &io, nullptr);
}

int qsp_qp_sens(qsp_solver* s, int32_t nb, int32_t N, const double* A, const double* B, const double* H, double* K0,
                double* K, double* dU, double* P0, int32_t* flag) {
    if (!s || nb < 1 || N < 1 || !A || !B || !H || !K0) return fail(QSP_ERR_ARG, "qsp_qp_sens: bad argument");
    for (size_t q = 0; q < (size_t)nb * N; ++q)
        if (!QpLaneData::has_structure(A + q * QpLaneData::NA))
            return fail(QSP_ERR_ARG, "qsp_qp_sens: A lacks the pusher-slider structure");
    HIPCHK(hipSetDevice(s->o.device));
    const Dims qd{(size_t)nb, (size_t)N};   // the QPs' own batch
    Staging st(s);
    SensQpArgs a;
    std::memset(&a, 0, sizeof a);
    a.N = N;
    a.nb = nb;
    a.A = st.in(A, qd.qp_A());
    a.B = st.in(B, qd.qp_B());
    a.H = st.in(H, qd.qp_Hg());
    a.out = sens_out(st, true, qd, K0, K, dU, P0, flag);
    if (st.err) return st.err;
    HIPCHK(sens_gain_buffer(s, a.out.dU, qd, &a.wK));
    HIPCHK(launch_sens_qp(a, s->stream));
    return st.finish();
}

// ------------------------------------- rollout costs and the u0 cost landscape
void qsp_default_rollout_opts(qsp_rollout_opts* o) {
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(qsp_rollout_opts);
    o->integrator = QSP_ROLLOUT_EULER;
    o->cost_scale = 1;
}

// the options' checks and the handle's cost, bounds and shapes into a kernel argument block
static int rollout_args(qsp_solver* s, const qsp_rollout_opts* o, const char* who, RolloutArgs& a) {
    const std::string w(who);
    if (!s || !o) return fail(QSP_ERR_ARG, w + ": null argument");
    if (o->struct_size != (int32_t)sizeof(qsp_rollout_opts))
        return fail(QSP_ERR_ARG, w + ": qsp_rollout_opts.struct_size != sizeof(qsp_rollout_opts) (stale layout?)");
    if (o->integrator != QSP_ROLLOUT_EULER && o->integrator != QSP_ROLLOUT_RK4)
        return fail(QSP_ERR_ARG, w + ": unknown integrator");
    if (o->cost_scale != 0 && o->cost_scale != 1) return fail(QSP_ERR_ARG, w + ": cost_scale must be 0 or 1");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, w + ": no shapes set");
    std::memset(&a, 0, sizeof a);
    a.N = s->o.N;
    a.B = s->o.batch;
    a.integrator = o->integrator;
    a.s0_bound = s->p.s0_bound;
    a.Ts = s->p.Ts;
    a.tau = o->cost_scale ? s->p.tau : 1.0;
    std::memcpy(a.W, s->p.W, sizeof a.W);
    std::memcpy(a.We, s->p.We, sizeof a.We);
    std::memcpy(a.lh, s->p.lh, sizeof a.lh);
    std::memcpy(a.uh, s->p.uh, sizeof a.uh);
    a.shapes = s->shapes.data();
    a.n_shapes = s->n_shapes;
    a.shape_id = s->shape_id.data();
    a.yref = s->yref.data();
    a.yref_e = s->yref_e.data();
    return QSP_OK;
}

// host entry and _device twin, as eval_kkt_run
static int rollout_cost_run(qsp_solver* s, const qsp_rollout_opts* opts, const char* who, bool host, int32_t M,
                            const qsp_rollout_io* io, void* stream) {
    RolloutArgs a;
    const int r = rollout_args(s, opts, who, a);
    if (r) return r;
    const std::string w(who);
    if (!io || !io->x0 || !io->U || !io->cost) return fail(QSP_ERR_ARG, w + missing(host));
    if (M < 1) return fail(QSP_ERR_ARG, w + ": M must be >= 1");
    HIPCHK(hipSetDevice(s->o.device));
    qsp_rollout_io d = *io;
    Staging st(s);
    if (host) {
        const size_t N = s->dim.N, BM = s->dim.B * (size_t)M;
        d.x0 = st.in(io->x0, s->dim.x0());
        d.U = st.in(io->U, BM * N * 2);
        d.yref = st.in(io->yref, s->dim.yref());
        d.yref_e = st.in(io->yref_e, s->dim.yref_e());
        d.cost = st.out(io->cost, BM);
        d.viol = st.out(io->viol, BM);
        d.x_end = st.out(io->x_end, BM * 4);
        if (st.err) return st.err;
    }
    a.M = M;
    a.x0 = d.x0;
    a.U = d.U;
    if (d.yref) a.yref = d.yref;
    if (d.yref_e) a.yref_e = d.yref_e;
    if (d.shape_id) a.shape_id = d.shape_id;
    a.cost = d.cost;
    a.viol = d.viol;
    a.x_end = d.x_end;
    HIPCHK(launch_rollout_cost(a, stream_of(s, host, stream)));
    return host ? st.finish() : QSP_OK;
}

int qsp_rollout_cost(qsp_solver* s, const qsp_rollout_opts* opts, int32_t M, const double* x0, const double* U,
                     const double* yref, const double* yref_e, double* cost, double* viol, double* x_end) {
    const qsp_rollout_io io = {x0, U, yref, yref_e, nullptr, cost, viol, x_end};
    return rollout_cost_run(s, opts, "qsp_rollout_cost", true, M, &io, nullptr);
}

int qsp_rollout_cost_device(qsp_solver* s, const qsp_rollout_opts* opts, int32_t M, const qsp_rollout_io* io,
                            void* stream) {
    return rollout_cost_run(s, opts, "qsp_rollout_cost_device", false, M, io, stream);
}

static int cost_landscape_run(qsp_solver* s, const qsp_rollout_opts* opts, const char* who, bool host,
                              const qsp_landscape_io* io, void* stream) {
    RolloutArgs a;
    const int r = rollout_args(s, opts, who, a);
    if (r) return r;
    const std::string w(who);
    if (!io || !io->x0 || !io->un_grid || !io->ut_grid || !io->u_min || !io->cost_min)
        return fail(QSP_ERR_ARG, w + missing(host));
    if (io->n_un < 1 || io->n_ut < 1) return fail(QSP_ERR_ARG, w + ": empty grid");
    if ((long long)io->n_un * io->n_ut > (1ll << 30)) return fail(QSP_ERR_ARG, w + ": more than 2^30 grid points");
    if (!io->U_tail && !s->solved)
        return fail(QSP_ERR_STATE, w + ": U_tail = NULL needs a solve (the last solution's tail)");
    HIPCHK(hipSetDevice(s->o.device));
    qsp_landscape_io d = *io;
    Staging st(s);
    if (host) {
        const size_t B = s->dim.B, G = (size_t)io->n_un * io->n_ut;
        d.x0 = st.in(io->x0, s->dim.x0());
        d.U_tail = st.in(io->U_tail, s->dim.U());
        d.un_grid = st.in(io->un_grid, (size_t)io->n_un);
        d.ut_grid = st.in(io->ut_grid, (size_t)io->n_ut);
        d.yref = st.in(io->yref, s->dim.yref());
        d.yref_e = st.in(io->yref_e, s->dim.yref_e());
        d.cost = st.out(io->cost, B * G);
        d.u_min = st.out(io->u_min, s->dim.u0());
        d.cost_min = st.out(io->cost_min, B);
        d.idx_min = st.out(io->idx_min, B);
        if (st.err) return st.err;
    }
    a.x0 = d.x0;
    a.U_tail = d.U_tail ? d.U_tail : s->wU.data();   // the iterate epilogue_kernel reads
    if (d.yref) a.yref = d.yref;
    if (d.yref_e) a.yref_e = d.yref_e;
    if (d.shape_id) a.shape_id = d.shape_id;
    a.n_un = d.n_un;
    a.n_ut = d.n_ut;
    a.un_grid = d.un_grid;
    a.ut_grid = d.ut_grid;
    a.cost = d.cost;
    a.u_min = d.u_min;
    a.cost_min = d.cost_min;
    a.idx_min = d.idx_min;
    HIPCHK(launch_cost_landscape(a, stream_of(s, host, stream)));
    return host ? st.finish() : QSP_OK;
}

int qsp_cost_landscape(qsp_solver* s, const qsp_rollout_opts* opts, const double* x0, const double* U_tail,
                       int32_t n_un, const double* un_grid, int32_t n_ut, const double* ut_grid, const double* yref,
                       const double* yref_e, double* cost, double* u_min, double* cost_min, int32_t* idx_min) {
    const qsp_landscape_io io = {x0, U_tail, un_grid, ut_grid, yref, yref_e, nullptr, cost, u_min, cost_min, idx_min,
                                 n_un, n_ut};
    return cost_landscape_run(s, opts, "qsp_cost_landscape", true, &io, nullptr);
}

int qsp_cost_landscape_device(qsp_solver* s, const qsp_rollout_opts* opts, const qsp_landscape_io* io, void* stream) {
    return cost_landscape_run(s, opts, "qsp_cost_landscape_device", false, io, stream);
}

// ------------------------------------- contact modes and the open-loop simulation
int qsp_eval_modes(qsp_solver* s, int32_t n, const int32_t* sid, const double* x, const double* u, int32_t* mode,
                   double* cone) {
    if (!s || !sid || !x || !u || !mode || n < 1) return fail(QSP_ERR_ARG, "qsp_eval_modes: bad argument");
    const int r = check_ids(s, n, sid);
    if (r) return r;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    const int32_t* d_sid = st.in(sid, n);
    const double *dx = st.in(x, (size_t)4 * n), *du = st.in(u, (size_t)2 * n);
    int32_t* d_mode = st.out(mode, n);
    double* d_cone = st.out(cone, (size_t)3 * n);
    if (st.err) return st.err;
    HIPCHK(launch_modes(s->shapes.data(), s->n_shapes, d_sid, n, 1, 1, dx, du, d_mode, d_cone, s->stream));
    return st.finish();
}

int qsp_get_modes(qsp_solver* s, int32_t* mode, double* cone) {
    if (!s || !mode) return fail(QSP_ERR_ARG, "qsp_get_modes: null argument");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, "qsp_get_modes: no shapes set");
    const size_t n = (size_t)s->o.batch * s->o.N;
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    int32_t* d_mode = st.out(mode, n);
    double* d_cone = st.out(cone, 3 * n);
    if (st.err) return st.err;
    // the buffers qsp_get_x / qsp_get_u copy out
    const Dev<double>& X = s->last_controller ? s->X : s->Xo;
    const Dev<double>& U = s->last_controller ? s->U : s->Uo;
    HIPCHK(launch_modes(s->shapes.data(), s->n_shapes, s->shape_id.data(), (long long)n, s->o.N, s->o.N + 1,
                        X.data(), U.data(), d_mode, d_cone, s->stream));
    return st.finish();
}

void qsp_default_open_loop_opts(qsp_open_loop_opts* o) {
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(qsp_open_loop_opts);
    o->n_steps = 1;
    o->M = 1;
    o->u_steps = 1;
    o->clip = 1;
    o->v_alpha = 1.0;   // 0.005 * 200 (helper.m:162)
}

// the options' checks and the handle's shapes into a kernel argument block; the delay ring when one is needed
static int open_loop_args(qsp_solver* s, const qsp_open_loop_opts* o, const char* who, OpenLoopArgs& a) {
    const std::string w(who);
    if (!s || !o) return fail(QSP_ERR_ARG, w + ": null argument");
    if (o->struct_size != (int32_t)sizeof(qsp_open_loop_opts))
        return fail(QSP_ERR_ARG, w + ": qsp_open_loop_opts.struct_size != sizeof(qsp_open_loop_opts) (stale layout?)");
    if (o->n_steps < 1) return fail(QSP_ERR_ARG, w + ": n_steps must be >= 1");
    if (o->M < 1) return fail(QSP_ERR_ARG, w + ": M must be >= 1");
    if (o->u_steps != 1 && o->u_steps != o->n_steps) return fail(QSP_ERR_ARG, w + ": u_steps must be 1 or n_steps");
    if (o->clip != 0 && o->clip != 1) return fail(QSP_ERR_ARG, w + ": clip must be 0 or 1");
    if (o->store_tile != 0 && o->store_tile != 1 && o->store_tile != 4 && o->store_tile != 8)
        return fail(QSP_ERR_ARG, w + ": store_tile must be 0, 1, 4 or 8");
    const double Ts = o->Ts == 0.0 ? s->o.Ts : o->Ts;
    if (!(Ts > 0.0)) return fail(QSP_ERR_ARG, w + ": Ts must be > 0 (0: the handle's)");
    if (!(o->plant_delay >= 0.0) || std::ceil(o->plant_delay / Ts) > 4096.0)
        return fail(QSP_ERR_ARG, w + ": plant_delay must be in [0, 4096 Ts]");
    if (s->n_shapes < 1) return fail(QSP_ERR_STATE, w + ": no shapes set");
    if ((long long)s->o.batch * o->M > (1ll << 31) - 1) return fail(QSP_ERR_ARG, w + ": more than 2^31 - 1 rows (B M)");
    std::memset(&a, 0, sizeof a);
    a.B = s->o.batch;
    a.M = o->M;
    a.T = o->n_steps;
    a.u_steps = o->u_steps;
    a.D = (int)std::ceil(o->plant_delay / Ts);   // delay_buff_plant (helper.m:147)
    a.clip = o->clip;
    a.tile = o->store_tile;
    a.Ts = Ts;
    a.v_alpha = o->v_alpha;
    a.shapes = s->shapes.data();
    a.n_shapes = s->n_shapes;
    a.shape_id = s->shape_id.data();
    HIPCHK(hipSetDevice(s->o.device));
    if (a.clip && a.D > 0) {
        HIPCHK(s->ol_ring.ensure(s->dim.ring(a.D, a.M)));
        a.ring = s->ol_ring.data();
    }
    return QSP_OK;
}

static int open_loop_run(qsp_solver* s, const qsp_open_loop_opts* opts, const char* who, bool host,
                         const qsp_open_loop_io* io, void* stream) {
    OpenLoopArgs a;
    const int r = open_loop_args(s, opts, who, a);
    if (r) return r;
    const std::string w(who);
    if (!io || !io->x0 || !io->U || !io->x_end) return fail(QSP_ERR_ARG, w + missing(host));
    if (io->noise && s->sn_on) return fail(QSP_ERR_ARG, w + NOISE_TWICE);
    qsp_open_loop_io d = *io;
    Staging st(s);
    if (host) {
        const size_t B = a.B, T = a.T, BM = B * (size_t)a.M;
        d.x0 = st.in(io->x0, B * 4);
        d.U = st.in(io->U, BM * a.u_steps * 2);
        d.noise = st.in(io->noise, T * B * 4);
        d.X = st.out(io->X, BM * (T + 1) * 4);
        d.U_out = st.out(io->U_out, BM * T * 2);
        d.S_p = st.out(io->S_p, BM * T * 2);
        d.mode = st.out(io->mode, BM * T);
        d.mode_steps = st.out(io->mode_steps, BM * 4);
        d.x_end = st.out(io->x_end, BM * 4);
        if (st.err) return st.err;
    }
    if ((((uintptr_t)d.X | (uintptr_t)d.U_out | (uintptr_t)d.S_p) & 15) != 0)
        return fail(QSP_ERR_ARG, w + ": X, U_out and S_p must be 16-byte aligned");
    a.x0 = d.x0;
    a.U = d.U;
    a.noise = d.noise;
    a.gen = noise_gen(s);
    a.lane_scale = noise_scale(s);
    if (d.shape_id) a.shape_id = d.shape_id;
    a.X = d.X;
    a.U_out = d.U_out;
    a.S_p = d.S_p;
    a.mode = d.mode;
    a.mode_steps = d.mode_steps;
    a.x_end = d.x_end;
    HIPCHK(launch_open_loop(a, stream_of(s, host, stream)));
    return host ? st.finish() : QSP_OK;
}

int qsp_open_loop(qsp_solver* s, const qsp_open_loop_opts* opts, const double* x0, const double* U, const double* noise,
                  double* X, double* U_out, double* S_p, int32_t* mode, int32_t* mode_steps, double* x_end) {
    const qsp_open_loop_io io = {x0, U, noise, nullptr, X, U_out, S_p, mode, mode_steps, x_end};
    return open_loop_run(s, opts, "qsp_open_loop", true, &io, nullptr);
}

int qsp_open_loop_device(qsp_solver* s, const qsp_open_loop_opts* opts, const qsp_open_loop_io* io, void* stream) {
    return open_loop_run(s, opts, "qsp_open_loop_device", false, io, stream);
}

// ------------------------------------------- sim_noise generated on the device
void qsp_default_sim_noise(qsp_sim_noise* g) {
    std::memset(g, 0, sizeof(*g));
    g->struct_size = (int32_t)sizeof(qsp_sim_noise);
    const double sigma[4] = {1e-5, 1e-5, 1e-3, 1e-4};   // helper.m:241
    std::memcpy(g->sigma, sigma, sizeof sigma);
}

int qsp_set_sim_noise(qsp_solver* s, const qsp_sim_noise* g) {
    if (!s || !g) return fail(QSP_ERR_ARG, "qsp_set_sim_noise: null argument");
    if (g->struct_size != (int32_t)sizeof(qsp_sim_noise))
        return fail(QSP_ERR_ARG, "qsp_set_sim_noise: qsp_sim_noise.struct_size != sizeof(qsp_sim_noise) (stale layout?)");
    for (int c = 0; c < 4; ++c)
        if (!(std::isfinite(g->sigma[c]) && g->sigma[c] >= 0.0))
            return fail(QSP_ERR_ARG, "qsp_set_sim_noise: sigma must be finite and >= 0");
    const size_t B = s->dim.lane();
    if (g->step_offset < 0 || g->lane_offset < 0 || g->lane_offset > (1ll << 32) - (long long)B)
        return fail(QSP_ERR_ARG, "qsp_set_sim_noise: need step_offset >= 0, lane_offset >= 0 and lane_offset + B <= 2^32");
    for (size_t i = 0; g->lane_scale && i < B; ++i)
        if (!(std::isfinite(g->lane_scale[i]) && g->lane_scale[i] >= 0.0))
            return fail(QSP_ERR_ARG, "qsp_set_sim_noise: lane_scale must be finite and >= 0");
    // a failed copy (QSP_ERR_HIP) leaves the generator installed before, without a scale
    if (g->lane_scale) {
        s->sn_has_scale = false;
        const int r = h2d_grow(s, s->sn_scale, g->lane_scale, B);
        if (r) return r;
    }
    s->sn = *g;
    s->sn.lane_scale = nullptr;
    s->sn_has_scale = g->lane_scale != nullptr;
    s->sn_on = true;
    return QSP_OK;
}

int qsp_clear_sim_noise(qsp_solver* s) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_clear_sim_noise: null handle");
    s->sn_on = s->sn_has_scale = false;
    return QSP_OK;
}

int qsp_get_sim_noise(qsp_solver* s, qsp_sim_noise* out, int32_t* installed, int32_t* has_scale) {
    if (!s) return fail(QSP_ERR_ARG, "qsp_get_sim_noise: null handle");
    if (out) {
        if (s->sn_on) *out = s->sn;
        else qsp_default_sim_noise(out);
    }
    if (installed) *installed = s->sn_on ? 1 : 0;
    if (has_scale) *has_scale = s->sn_on && s->sn_has_scale ? 1 : 0;
    return QSP_OK;
}

int qsp_gen_sim_noise(qsp_solver* s, int32_t n_steps, double* noise) {
    if (!s || !noise || n_steps < 1) return fail(QSP_ERR_ARG, "qsp_gen_sim_noise: bad argument");
    if (!s->sn_on) return fail(QSP_ERR_STATE, "qsp_gen_sim_noise: no sim_noise generator installed (qsp_set_sim_noise)");
    HIPCHK(hipSetDevice(s->o.device));
    Staging st(s);
    double* d = st.out(noise, s->dim.cl_noise((size_t)n_steps));
    if (st.err) return st.err;
    HIPCHK(launch_sim_noise(noise_gen(s), noise_scale(s), s->o.batch, n_steps, d, s->stream));
    return st.finish();
}

}  // extern "C"
