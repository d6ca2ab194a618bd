// qsp_ipm.hpp — the per-stage arithmetic of the interior point and of the SQP around it: the bound
// pairs of a slot (barrier terms, predictor and corrector directions, step), the IPM iteration's
// exit test, the KKT residuals, merit weights and multiplier update of the merit SQP, the
// controller's initial guess and its stage-0 feasibility rule.  As qsp_riccati.hpp: straight-line
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

}  // namespace qsp
