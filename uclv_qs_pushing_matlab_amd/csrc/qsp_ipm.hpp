// qsp_ipm.hpp — the per-stage arithmetic of the interior point and of the SQP around it: the bound
// pairs of a slot (barrier terms, predictor and corrector directions, step), the IPM iteration's
// exit test, the KKT residuals, merit weights and multiplier update of the merit SQP; and the per-lane
// code around a solve: the reference staging, the controller's prologue with its initial guess and
// stage-0 feasibility rule, the epilogue's cost, status rule and warm-start shift, the parameters from
// the options and the QP-level entry's mapping and status.  As qsp_riccati.hpp: straight-line
// functions of one lane's own data, compiled by hipcc into the kernels and by a plain C++ compiler
// into the CPU twin (oracle/qsp_twin.cpp), which restates only the orchestration around them
// (the qualifier macro: qsp_fp.hpp).
//
// A slot's IPM fields live in LDS on the device and in a plain struct in the twin, so the functions
// that touch them take a *view* V of a lane's slots and the slot ls: a type whose members t(ls, q),
// lm(ls, q), rt(ls, q) (q = 0..5: [2j] lower, [2j+1] upper bound of component j), v(ls, j),
// va(ls, j), vn(ls, j) (j = 0..2: s, u_n, u_t), hg(ls, i), du(ls, i) return double&.  Stage<S>
// (qsp_solver.hip) is the kernels' view and tw_view the twin's; every access is written where the
// kernels had it, so the order of the LDS reads and writes is the source's.  The view is the lane's,
// not the slot's, and bnd_act reads s0_bound itself: a per-slot view object, or the flag passed by
// value, changes the code the compiler emits for the kernels (profiles/ipm_shared/README.md, which
// also lists the blocks that stay written out on both sides, each with the measurement that kept it
// there: registers, the headline A/B for the start point, or an instruction count).
#pragma once
#include "qsp_math.hpp"

namespace qsp {

// ------------------------------------------------------------------ the IPM's slots
// Is bound side j (0 = s, 1 = u_n, 2 = u_t) of stage k part of the QP?  Stages 0..N-1; the s
// bound at stage 0 only with stage0_s_bound (s_0 is fixed by x0 there: the pair is a
// constant slack that enters the complementarity measure, NMPC_controller.m:237,251-252).
QSP_FN bool bnd_act(const SolveParams& p, int N, int k, int j) { return (k < N) && (j > 0 || k >= 1 || p.s0_bound != 0); }

// bounds of the QP step of a slot: lo = lh - v, hi = uh - v, v = (s, u_n, u_t)
template <class V>
QSP_FN void bnd_lohi(const SolveParams& p, const V& st, int ls, double lo[3], double hi[3]) {
    const double v0 = st.v(ls, 0), v1 = st.v(ls, 1), v2 = st.v(ls, 2);
    lo[0] = p.lh[0] - v0; hi[0] = p.uh[0] - v0;
    lo[1] = p.lh[1] - v1; hi[1] = p.uh[1] - v1;
    lo[2] = p.lh[2] - v2; hi[2] = p.uh[2] - v2;
}

enum QpExit : int { QP_EXIT_CONV = 0, QP_EXIT_CAP = 1, QP_EXIT_STALL = 2, QP_EXIT_DIVERGED = 3 };

// The iteration's exit test: divergence first (mu non-finite or past qp_mu_max: a NaN mu would pass
// the stop test), then the stop test, then the stall exit (locally infeasible QP: the step length
// stays tiny while mu grows).
QSP_FN void ipm_exit_test(const SolveParams& p, double mu, double rscale, double rs_stop, int stall, bool skip,
                          bool& div, bool& conv, bool& stalled) {
    div = !skip && !(mu < p.qp_mu_max);
    conv = !div && (skip || (!(mu >= p.mu_stop) && !(rscale >= rs_stop)));
    stalled = !conv && !div && p.qp_stall_iters > 0 && stall >= p.qp_stall_iters;
}
QSP_FN int ipm_exit_code(bool conv, bool div, bool stalled) {
    return conv ? QP_EXIT_CONV : (div ? QP_EXIT_DIVERGED : (stalled ? QP_EXIT_STALL : QP_EXIT_CAP));
}

// Barrier terms of bound pair j of slot k (predictor): hg[j] Hessian addition, hg[3 + j] gradient
// addition.  They depend on t, lm, rt and the iterate only, not on mu.  The corrector changes
// only the gradient (corrector_terms).
template <class V>
QSP_FN void barrier_term(const SolveParams& p, int N, const V& st, int ls, int k, int j, double hg[6]) {
    const double v = st.v(ls, j);
    const double lo = p.lh[j] - v, hi = p.uh[j] - v;   // bnd_lohi's
    const bool act = bnd_act(p, N, k, j);
    const double ll = st.lm(ls, 2 * j), lh = st.lm(ls, 2 * j + 1);
    const double sl = ll * st.rt(ls, 2 * j), sh = lh * st.rt(ls, 2 * j + 1);
    const double gadd = qfma(-sh, hi, -sl * lo) + (lh - ll);
    hg[j] = act ? sl + sh : 0.0;
    hg[3 + j] = act ? gadd : 0.0;
}

// The step length is the largest alpha with t + alpha dt >= 0 and l + alpha dl >= 0,
// tracked as a ratio num/den without dividing (den > 0): a candidate t/(-dt) replaces
// num/den when t * den < num * (-dt).

// Affine (predictor) slack/multiplier directions of slot k from its bounded QP solution
// components (va), unmasked, kept by the caller for the rest of the IPM iteration:
// at/al[2j] lower, [2j+1] upper bound of component j.  Also folds the masked directions
// into the step-length ratio num/den.
template <class V>
QSP_FN void affine_dirs(const SolveParams& p, int N, const V& st, int ls, int k, double at[6], double al[6], double& num,
                        double& den) {
    double lo[3], hi[3];
    bnd_lohi(p, st, ls, lo, hi);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool act = bnd_act(p, N, k, j);
        const double tl = st.t(ls, 2 * j), th = st.t(ls, 2 * j + 1);
        const double ll = st.lm(ls, 2 * j), lh = st.lm(ls, 2 * j + 1);
        const double sl = ll * st.rt(ls, 2 * j), sh = lh * st.rt(ls, 2 * j + 1);
        const double v = st.va(ls, j);
        at[2 * j] = v - lo[j] - tl;
        at[2 * j + 1] = hi[j] - v - th;
        al[2 * j] = qfma(-sl, at[2 * j], -ll);
        al[2 * j + 1] = qfma(-sh, at[2 * j + 1], -lh);
        const double dtl = act ? at[2 * j] : 0.0, dth = act ? at[2 * j + 1] : 0.0;
        const double dll = act ? al[2 * j] : 0.0, dlh = act ? al[2 * j + 1] : 0.0;
        if (dtl < 0.0 && tl * den < num * -dtl) { num = tl; den = -dtl; }
        if (dth < 0.0 && th * den < num * -dth) { num = th; den = -dth; }
        if (dll < 0.0 && ll * den < num * -dll) { num = ll; den = -dll; }
        if (dlh < 0.0 && lh * den < num * -dlh) { num = lh; den = -dlh; }
    }
}

// Complementarity after the affine step aa (Mehrotra's mu_aff), from the cached directions.
template <class V>
QSP_FN double affine_mu_part(const SolveParams& p, int N, const V& st, int ls, int k, const double at[6], const double al[6],
                             double aa, double part) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool act = bnd_act(p, N, k, j);
        const double tl = st.t(ls, 2 * j), th = st.t(ls, 2 * j + 1);
        const double ll = st.lm(ls, 2 * j), lh = st.lm(ls, 2 * j + 1);
        const double dtl = act ? at[2 * j] : 0.0, dth = act ? at[2 * j + 1] : 0.0;
        const double dll = act ? al[2 * j] : 0.0, dlh = act ? al[2 * j + 1] : 0.0;
        part = qfma(qfma(aa, dtl, tl), qfma(aa, dll, ll), part);
        part = qfma(qfma(aa, dth, th), qfma(aa, dlh, lh), part);
    }
    return part;
}

// Corrector barrier gradient change of slot k from the cached affine directions (the
// Hessian is the predictor's): hg[3+j] = c_h / t_h - c_l / t_l, c = sigma mu - dt_aff dl_aff.
template <class V>
QSP_FN void corrector_terms(const SolveParams& p, int N, const V& st, int ls, int k, const double at[6], const double al[6],
                            double smu) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool act = bnd_act(p, N, k, j);
        const double cl = qfma(-at[2 * j], al[2 * j], smu), ch = qfma(-at[2 * j + 1], al[2 * j + 1], smu);
        st.hg(ls, 3 + j) = act ? qfma(ch, st.rt(ls, 2 * j + 1), -(cl * st.rt(ls, 2 * j))) : 0.0;
    }
}

// Corrector directions of slot k (masked) from its bounded QP solution components (vn) and
// the cached affine directions; folded into the ratio num/den and kept for the update.
template <class V>
QSP_FN void corrector_dirs(const SolveParams& p, int N, const V& st, int ls, int k, const double at[6], const double al[6],
                           double smu, double dt[6], double dl[6], double& num, double& den) {
    double lo[3], hi[3];
    bnd_lohi(p, st, ls, lo, hi);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool act = bnd_act(p, N, k, j);
        const double tl = st.t(ls, 2 * j), th = st.t(ls, 2 * j + 1);
        const double ll = st.lm(ls, 2 * j), lh = st.lm(ls, 2 * j + 1);
        const double rtl = st.rt(ls, 2 * j), rth = st.rt(ls, 2 * j + 1);
        const double sl = ll * rtl, sh = lh * rth;
        const double v = st.vn(ls, j);
        double dtl = v - lo[j] - tl, dth = hi[j] - v - th;
        double dll = qfma(-sl, dtl, -ll), dlh = qfma(-sh, dth, -lh);
        dll = qfma(qfma(-at[2 * j], al[2 * j], smu), rtl, dll);
        dlh = qfma(qfma(-at[2 * j + 1], al[2 * j + 1], smu), rth, dlh);
        dtl = act ? dtl : 0.0; dth = act ? dth : 0.0;
        dll = act ? dll : 0.0; dlh = act ? dlh : 0.0;
        if (dtl < 0.0 && tl * den < num * -dtl) { num = tl; den = -dtl; }
        if (dth < 0.0 && th * den < num * -dth) { num = th; den = -dth; }
        if (dll < 0.0 && ll * den < num * -dll) { num = ll; den = -dll; }
        if (dlh < 0.0 && lh * den < num * -dlh) { num = lh; den = -dlh; }
        dt[2 * j] = dtl; dt[2 * j + 1] = dth;
        dl[2 * j] = dll; dl[2 * j + 1] = dlh;
    }
}

// Step of a slot: t += alpha dt (and its reciprocal), l += alpha dl.
template <class V>
QSP_FN void apply_step(const V& st, int ls, const double dt[6], const double dl[6], double alpha) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double tn = qfma(alpha, dt[q], st.t(ls, q));
        st.t(ls, q) = tn;
        st.rt(ls, q) = rcp(tn);
        st.lm(ls, q) = qfma(alpha, dl[q], st.lm(ls, q));
    }
}

// the damped control step of a slot: du += alpha (vn - du)
template <class V>
QSP_FN void damp_du(const V& st, int ls, double alpha) {
    st.du(ls, 0) = qfma(alpha, st.vn(ls, 1) - st.du(ls, 0), st.du(ls, 0));
    st.du(ls, 1) = qfma(alpha, st.vn(ls, 2) - st.du(ls, 1), st.du(ls, 1));
}

// ------------------------------------------------------------------ the SQP's stages
// KKT residuals of stage k of the NLP iterate (nlp_mode 1) folded into the running maxima: ru, rx
// the stationarity in u and x, rt the terminal stage's, re the defect, ri the bound violation, rc
// the complementarity.  PIk, LAMk: the stage's multipliers (zero at k = N), PIp = pi_{k-1}.  Each
// maximum is only ever folded into itself (x = fmax(x, .)), never read for another: the kernel hands
// one variable in for ru, rx and rt (its single stationarity maximum), and an edit must keep that legal.
QSP_FN void kkt_stage(const SolveParams& p, int k, const double a[6], const double B[8], const double g[6],
                      const double bb[4], const double v[3], const double PIk[4], const double PIp[4],
                      const double LAMk[6], double& ru, double& rx, double& rt, double& re, double& ri, double& rc) {
    if (k < p.N) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double r = (g[4 + i] + qfma(B[6 + i], PIk[3], qfma(B[4 + i], PIk[2], qfma(B[2 + i], PIk[1], B[i] * PIk[0])))) +
                             (LAMk[2 * (1 + i) + 1] - LAMk[2 * (1 + i)]);
            ru = fmax(ru, fabs(r));
        }
        if (k >= 1) {
            const double at[4] = {PIk[0], PIk[1], qfma(a[2], PIk[1], a[0] * PIk[0]) + PIk[2],
                                  qfma(a[5], PIk[3], qfma(a[4], PIk[2], qfma(a[3], PIk[1], a[1] * PIk[0])))};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double r = g[i] - PIp[i] + at[i];
                if (i == 3) r += LAMk[1] - LAMk[0];
                rx = fmax(rx, fabs(r));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) re = fmax(re, fabs(bb[i]));
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j == 0 && k == 0 && !p.s0_bound) continue;
            const double sl = v[j] - p.lh[j], sh_ = p.uh[j] - v[j];
            ri = fmax(ri, fmax(-sl, -sh_));
            rc = fmax(rc, fmax(fabs(LAMk[2 * j] * sl), fabs(LAMk[2 * j + 1] * sh_)));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) rt = fmax(rt, fabs(g[i] - PIp[i]));
    }
}

// merit weight update: w <- max(|m|, (w + |m|) / 2) with a = |m| of the QP's multiplier
QSP_FN double merit_weight(double w, double a) {
    const double wq = 0.5 * (w + a);
    return a > wq ? a : wq;
}

// damped update old + alpha (new - old) of the NLP's multipliers
QSP_FN double damp_update(double alpha, double nw, double old) { return qfma(alpha, nw - old, old); }

// ------------------------------------------------------------------ prologue
// The controller's state guess from its input guess (NMPC_controller.m:357-380): an Euler rollout
// from x0, each stage's u_t clipped to v_bound at the rolled-out contact (u_n scaled with it).
QSP_FN void guess_rollout(const ShapeDev& sh, const SolveParams& p, const double x0[4], double* U, double* X) {
    const int N = p.N;
    double xc[4] = {x0[0], x0[1], x0[2], x0[3]};
    for (int k = 0; k <= N; ++k) {
        for (int c = 0; c < 4; ++c) X[4 * k + c] = xc[c];
        if (k == N) break;
        const double vb = v_bound(sh, p.cp, xc[3]);
        const double ut_old = U[2 * k + 1];
        if (fabs(ut_old) > vb) {
            const double sgn = ut_old > 0.0 ? 1.0 : -1.0;
            U[2 * k + 1] = sgn * vb;
            U[2 * k] = U[2 * k + 1] * U[2 * k] / ut_old;
        }
        euler_step(sh, p.Ts, xc, U[2 * k], U[2 * k + 1]);
    }
}

// With the stage-0 s bound in the QP (stage0_s_bound), s_0 = x0's s is a fixed quantity of every
// QP: outside [lh_s, uh_s] every QP of the solve is infeasible, and the instance does not iterate.
QSP_FN bool s0_infeasible(const SolveParams& p, double s0) { return p.s0_bound && !(s0 >= p.lh[0] && s0 <= p.uh[0]); }

// get_y_ref (NMPC_controller.m:307-313) for one controller step of one lane: stage k takes column
// index_time + k (1-based) of the lane's table (T x 6) as set_reference_trajectory (:425-431) builds it --
// D = delay_buff_comp zero columns prepended, their u_t-reference row copied from the first real column --
// clamped to the last column; the terminal reference is the last stage's (:348)
QSP_FN void stage_yref(const double* traj, int T, int D, int index_time, int N, double* yref, double* ye) {
    for (int k = 0; k < N; ++k) {
        int idx = index_time + k;
        if (idx > T + D) idx = T + D;
        if (idx < 1) idx = 1;
        double* out = yref + 6 * k;
        if (idx <= D) {
            for (int c = 0; c < 5; ++c) out[c] = 0.0;
            out[5] = traj[5];
        } else {
            for (int c = 0; c < 6; ++c) out[c] = traj[(size_t)(idx - D - 1) * 6 + c];
        }
    }
    for (int c = 0; c < 4; ++c) ye[c] = yref[6 * (N - 1) + c];
}

// NMPC_controller.solve's prologue (NMPC_controller.m:332-380): x0's contact wrapped into [-b, b), the
// input guess (cold: u_n at its lower bound, u_t = 0; else the warm start Uw), the state guess rolled out
QSP_FN void controller_guess(const ShapeDev& sh, const SolveParams& p, bool cold, const double* Uw, double x0[4],
                             double* U, double* X) {
    x0[3] = wrap_contact(sh, x0[3]);
    for (int k = 0; k < p.N; ++k) {
        U[2 * k] = cold ? p.cp.u_n_lb : Uw[2 * k];
        U[2 * k + 1] = cold ? 0.0 : Uw[2 * k + 1];
    }
    guess_rollout(sh, p, x0, U, X);
}

// ------------------------------------------------------------------ epilogue
// 0.5 tau sum_k |y_k - yref_k|^2_W + 0.5 |x_N - ye|^2_We of the returned iterate
QSP_FN double solve_cost(const SolveParams& p, const double* X, const double* U, const double* yref, const double* ye) {
    const int N = p.N;
    double cost = 0.0;
    for (int k = 0; k < N; ++k) {
        double s = 0.0;
        for (int q = 0; q < 4; ++q) { const double r = X[4 * k + q] - yref[6 * k + q]; s = qfma(p.W[q] * r, r, s); }
        for (int q = 0; q < 2; ++q) { const double r = U[2 * k + q] - yref[6 * k + 4 + q]; s = qfma(p.W[4 + q] * r, r, s); }
        cost = qfma(0.5 * p.tau, s, cost);
    }
    double s = 0.0;
    for (int q = 0; q < 4; ++q) { const double r = X[4 * N + q] - ye[q]; s = qfma(p.We[q] * r, r, s); }
    return qfma(0.5, s, cost);
}

// Is any word of the returned iterate (X, U, and the x0 it was given) not finite?
QSP_FN bool iterate_nonfinite(int N, const double* X, const double* U, const double x0[4]) {
    bool bad = false;
    for (int q = 0; q < 4 * (N + 1); ++q) bad |= !isfinite(X[q]);
    for (int q = 0; q < 2 * N; ++q) bad |= !isfinite(U[q]);
    for (int q = 0; q < 4; ++q) bad |= !isfinite(x0[q]);
    return bad;
}

// A lane's status (QSP_STATUS_*, qsp_nmpc.h) from its iterate and the SQP's record fr: 0 ran to the end,
// 1 converged, 2 non-finite QP solution, 3 infeasible stage-0 bound, 4 diverged QP (sqp_iter was written
// when it stopped; an instance that never stopped counts all of them).  Non-finite wins: a non-finite
// iterate is QSP_STATUS_NAN (1) whatever its QP did; a failed QP is QSP_STATUS_QP_FAIL (4) only on a
// finite iterate; the merit SQP that ran to the end is QSP_STATUS_MAXITER (2).
enum SolveStatus : int { ST_SUCCESS = 0, ST_NAN = 1, ST_MAXITER = 2, ST_QP_FAIL = 4 };   // = QSP_STATUS_* (qsp_solver.hip asserts it)
QSP_FN int solve_status(const SolveParams& p, bool bad, int fr, int& sqp_iter) {
    if (fr == 0) sqp_iter = p.sqp_iters;
    if (bad || fr == 2) return ST_NAN;
    if (fr == 3 || fr == 4) return ST_QP_FAIL;
    return (p.nlp_mode == 1 && fr != 1) ? ST_MAXITER : ST_SUCCESS;
}

// out row k (W doubles) = in row min(k + sh, n - 1): the warm start's shift (NMPC_controller.m:397-399,
// sh = 1, the last row repeated) or a plain copy (sh = 0).  in's word (row, q) lies at row * rs + q * cs.
template <int W>
QSP_FN void shift_rows(int n, int sh, const double* in, size_t rs, size_t cs, double* out) {
    for (int k = 0; k < n; ++k) {
        const int src = (k + sh < n) ? k + sh : n - 1;
        for (int q = 0; q < W; ++q) out[W * k + q] = in[src * rs + q * cs];
    }
}

// ------------------------------------------------------------------ options and the QP level (host)
// The parameters that the library's options (qsp_options) and the twin's (or_opts) name alike.  The
// caller sets what differs: tau, W, We, lh, uh, cp, mfma_walk.
template <class O>
QSP_HD_FN void params_from_options(SolveParams& p, const O& o) {
    p.N = o.N;
    p.nlp_mode = o.nlp_mode;
    p.sqp_iters = o.sqp_iters;
    p.qp_iters = o.qp_iters;
    p.Ts = o.Ts;
    p.mu0 = o.mu0; p.t_min = o.t_min; p.frac = o.frac; p.sigma_min = o.sigma_min; p.mu_stop = o.mu_stop;
    p.res_stop = o.res_stop; p.qp_tol_stat = o.qp_tol_stat; p.qp_tol_eq = o.qp_tol_eq;
    p.s0_bound = o.stage0_s_bound ? 1 : 0;
    p.factor_scan = o.factor_scan ? 1 : 0;
    p.qp_stall_iters = o.qp_stall_iters; p.qp_stall_alpha = o.qp_stall_alpha; p.qp_mu_max = o.qp_mu_max;
    p.tol_stat = o.tol_stat; p.tol_eq = o.tol_eq; p.tol_ineq = o.tol_ineq; p.tol_comp = o.tol_comp;
    p.ls_alpha_min = o.ls_alpha_min; p.ls_alpha_red = o.ls_alpha_red; p.ls_eps = o.ls_eps;
}

// The QP-level entry on the kernels' parameters: a QP min sum 0.5 z'Hz + g'z, lo <= (ds, du) <= hi is the
// SQP's QP at tau = 1, W = the stage Hessian, We = the terminal one (H: 6 N + 4 diagonal entries), lh = 0,
// uh = hi - lo of the first stage (lo, hi: N x 3), around an iterate whose bounded components are v = -lo
QSP_HD_FN void qp_level_params(SolveParams& p, const double* H, const double* lo, const double* hi) {
    p.tau = 1.0;
    for (int i = 0; i < 6; ++i) p.W[i] = H[i];
    for (int i = 0; i < 4; ++i) p.We[i] = H[6 * p.N + i];
    for (int j = 0; j < 3; ++j) { p.lh[j] = 0.0; p.uh[j] = hi[j] - lo[j]; }
}
// ... that iterate: X (N + 1 x 4) zero but for s_k = -lo_s(k), k < N; U = -lo_u; x0 = dx0 + X_0
QSP_HD_FN void qp_level_iterate(int N, const double* lo, const double dx0[4], double* X, double* U, double x0[4]) {
    for (int q = 0; q < 4 * (N + 1); ++q) X[q] = 0.0;
    for (int k = 0; k < N; ++k) {
        X[4 * k + 3] = -lo[3 * k];
        U[2 * k] = -lo[3 * k + 1];
        U[2 * k + 1] = -lo[3 * k + 2];
    }
    for (int q = 0; q < 4; ++q) x0[q] = dx0[q];
    x0[3] += X[3];
}
// the exit's qp_status: 0 stop test met, 2 cap, 4 stall (min step), 5 diverged
QSP_FN int qp_exit_status(int exit) {
    return exit == QP_EXIT_CONV ? 0 : (exit == QP_EXIT_CAP ? 2 : (exit == QP_EXIT_STALL ? 4 : 5));
}
// ... and the entry's: 1 for a non-finite solution (dx: N + 1 x 4, du: N x 2); else 3 for an infeasible QP
// (the stage-0 s is fixed, dx_0 = dx0: outside its bounds with s0_bound); else the exit's
QSP_HD_FN int qp_level_status(const SolveParams& p, const double* dx, const double* du, const double* lo,
                              const double* hi, const double dx0[4], int exit_status) {
    bool fin = true;
    for (int q = 0; q < (p.N + 1) * 4; ++q) fin = fin && __builtin_isfinite(dx[q]);   // (host and device alike)
    for (int q = 0; q < p.N * 2; ++q) fin = fin && __builtin_isfinite(du[q]);
    const bool infeas = p.s0_bound && (dx0[3] < lo[0] || dx0[3] > hi[0]);
    return !fin ? 1 : (infeas ? 3 : exit_status);
}

}  // namespace qsp
