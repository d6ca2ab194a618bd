// qsp_kkt.hpp — KKT residuals recomputed from given numbers: one stage of an NLP iterate (X, U, PI, LAM
// against the OCP: qsp_eval_kkt) and one stage of a QP point (dx, du, pi, lam against caller-given QP
// data: qsp_qp_residuals).  Lane-local straight-line functions like the other arithmetic headers
// (qsp_fp.hpp): hipcc compiles them into qsp_kkt.hip, a plain C++ compiler into a host program
// (tests/stubs/kkt_main.cpp), as qsp_noise.hpp.
//
// kkt_nlp_stage takes the point's stage (x, u, one RK4 step with sensitivities) and the implied multipliers
// from qsp_point.hpp, forms the defect bb = xn - x_{k+1} and the gradient g = tau W (x - yr), terminal
// g = We (x_N - ye), and hands them to kkt_stage (qsp_ipm.hpp) unchanged.  The SQP kernels keep a stage load
// of their own (qsp_solver.hip, the LIN branch of qp_step_kernel) -- the comment above qp_outcome there records
// what sharing it costs them in registers -- so that on the merit SQP's converged lanes this function
// reproduces that solver's last test bit for bit only as long as the two agree:
// tests/test_gpu_kkt.py::test_reproduces_the_merit_sqp_test holds them together.
//
// Non-finite values: kkt_stage folds with fmax, which drops a NaN.  Both stage functions therefore return
// a flag beside their maxima -- every value the stage read, and its linearisation, is finite -- and the
// caller turns a lane with one unset flag into NaN (kkt_fold / the kernels' reduction).
#pragma once
#include "qsp_point.hpp"

namespace qsp {

// columns of the NLP parts table (QSP_KKT_* of include/qsp_nmpc.h) and of the QP residuals (counts: qsp_types.h)
enum KktPart : int { KP_STAT_U = 0, KP_STAT_X = 1, KP_STAT_TERM = 2, KP_EQ_DYN = 3, KP_EQ_X0 = 4, KP_INEQ = 5, KP_COMP = 6 };
enum KktQpRes : int { KQ_STAT_U = 0, KQ_STAT_X = 1, KQ_DYN = 2, KQ_INFEAS = 3, KQ_COMP = 4, KQ_DUAL = 5 };

// a stage's maxima into the lane's (all >= 0: fmax from 0), the flags combined
QSP_FN void kkt_fold(int n, const double* part, bool fin, double* lane, bool& lane_fin) {
    for (int q = 0; q < n; ++q) lane[q] = fmax(lane[q], part[q]);
    lane_fin = lane_fin && fin;
}

// the acados residuals of a parts row: res_stat, res_eq, res_ineq, res_comp
QSP_FN void kkt_res_of_parts(const double* part, double res[4]) {
    res[0] = fmax(part[KP_STAT_U], fmax(part[KP_STAT_X], part[KP_STAT_TERM]));
    res[1] = fmax(part[KP_EQ_DYN], part[KP_EQ_X0]);
    res[2] = part[KP_INEQ];
    res[3] = part[KP_COMP];
}

// Stage k of an NLP iterate: part[KKT_NPARTS], each the largest absolute residual of its kind at this
// stage (0 where the stage has none).  r: the point's rows at (lane, k); u, x_{k+1}, pi_k, lam_k are read for
// k < N only, pi_{k-1} for k >= 1, r.yr is yref_k (6) for k < N and yref_e (4) at k = N; r.x0: read at k = 0,
// nullptr: x_0 is taken as the initial state (KP_EQ_X0 = 0).  r.lam == nullptr: the implied multipliers
// (implied_lam, qsp_point.hpp).  That component's stationarity is then zero by construction and the
// optimality gap shows in KP_COMP; at a KKT point with strict complementarity they are the multipliers.
// Returns the finite flag.
QSP_FN bool kkt_nlp_stage(const ShapeDev& sh, const SolveParams& p, int k, const PointRows& r, double part[KKT_NPARTS]) {
    const int N = p.N;
    double a[6] = {}, Bm[8] = {}, bb[4] = {}, g[6] = {}, pk[4] = {}, pp[4] = {}, lam[6] = {}, x[4], u[2] = {};
    bool fin;
    if (k >= 1) load(pp, r.pip, 4);   // (checked by stage k - 1)
    if (k < N) {
        double xn[4], x1[4], y[6];
        fin = point_stage(sh, p.Ts, r.x, r.u, x, u, a, Bm, xn);
        load(x1, r.x1, 4);   // (checked by stage k + 1)
        fin &= load(y, r.yr, 6) & load(pk, r.pi, 4);
        for (int q = 0; q < 4; ++q) bb[q] = xn[q] - x1[q];
        for (int q = 0; q < 4; ++q) g[q] = p.tau * p.W[q] * (x[q] - y[q]);
        for (int q = 0; q < 2; ++q) g[4 + q] = p.tau * p.W[4 + q] * (u[q] - y[4 + q]);
        if (r.lam) fin &= load(lam, r.lam, 6);
        else implied_lam(k, g[3], g + 4, a, Bm, pk, pp, lam);
    } else {   // terminal stage: no dynamics (a, Bm, bb and the input gradient stay 0)
        double y[4];
        fin = load(x, r.x, 4) & load(y, r.yr, 4);
        for (int q = 0; q < 4; ++q) g[q] = p.We[q] * (x[q] - y[q]);
    }
    const double v[3] = {x[3], u[0], u[1]};
    double ru = 0.0, rx = 0.0, rt = 0.0, re = 0.0, ri = 0.0, rc = 0.0, r0 = 0.0;
    kkt_stage(p, k, a, Bm, g, bb, v, pk, pp, lam, ru, rx, rt, re, ri, rc);
    if (k == 0 && r.x0) {
        double z[4];
        fin &= load(z, r.x0, 4);
        for (int q = 0; q < 4; ++q) r0 = fmax(r0, fabs(z[q] - x[q]));
    }
    part[KP_STAT_U] = ru;
    part[KP_STAT_X] = rx;
    part[KP_STAT_TERM] = rt;
    part[KP_EQ_DYN] = re;
    part[KP_EQ_X0] = r0;
    part[KP_INEQ] = ri;
    part[KP_COMP] = rc;
    return fin;
}

// Stage k of a QP point against the QP min sum 0.5 z'Hz + g'z, dx_{k+1} = A dx_k + B du_k + b, dx_0 = dx0,
// lo <= (dx_k[3], du_k) <= hi with the sign conventions of qsp_qp_solve's multipliers:
//     inputs              H_u du_k + g_u + B_k' pi_k - lam_lo + lam_hi                       KQ_STAT_U
//     states, 0 < k < N   H_x dx_k + g_x + A_k' pi_k - pi_{k-1} + e_s (lam_hi - lam_lo)      KQ_STAT_X
//     terminal            H_N dx_N + g_N - pi_{N-1}                                          KQ_STAT_X
//     dynamics            dx_{k+1} - A_k dx_k - B_k du_k - b_k;  at k = 0 also dx_0 - dx0    KQ_DYN
//     bounds              -min(t, 0), |lam t|, -min(lam, 0) with t = (v - lo, hi - v)        KQ_INFEAS, _COMP, _DUAL
// A: full row-major 4 x 4, no structure required; B: row-major 4 x 2; H, g: the stage's 6 entries
// (x then u; 4 at k = N); lo, hi: 3; lam: (s lo, s hi, u_n lo, u_n hi, u_t lo, u_t hi).  The data are
// read as given.  The stage-0 s row enters KQ_INFEAS, _COMP and _DUAL only with s0_bound (dx_0's s is no
// variable of the QP otherwise).  A, B, b, lo, hi, duk, dxk1, PIk, LAMk are read for k < N only, PIp for
// k >= 1, dx0 at k = 0 (the rows of QpLaneData and PointRows, qsp_point.hpp).  Returns the finite flag.
QSP_FN bool kkt_qp_stage(int N, int s0_bound, int k, const double* A, const double* B, const double* b, const double* H,
                         const double* g, const double* lo, const double* hi, const double* dx0, const double* dxk,
                         const double* duk, const double* dxk1, const double* PIk, const double* PIp, const double* LAMk,
                         double res[KKT_QP_NRES]) {
    const int nh = k < N ? 6 : 4;
    double x[4], pp[4] = {0, 0, 0, 0}, h[6], gg[6];
    bool fin = load(x, dxk, 4) & load(h, H, nh) & load(gg, g, nh);
    if (k >= 1) load(pp, PIp, 4);   // (checked by stage k - 1)
    for (int q = 0; q < KKT_QP_NRES; ++q) res[q] = 0.0;
    if (k < N) {
        double Am[16], Bm[8], bv[4], l[3], hh[3], u[2], x1[4], pk[4], lam[6];
        fin &= load(Am, A, 16) & load(Bm, B, 8) & load(bv, b, 4) & load(pk, PIk, 4) & load(l, lo, 3) & load(hh, hi, 3) &
               load(u, duk, 2) & load(lam, LAMk, 6);
        load(x1, dxk1, 4);   // (checked by stage k + 1)
        for (int i = 0; i < 2; ++i) {
            double r = qfma(h[4 + i], u[i], gg[4 + i]);
            for (int j = 0; j < 4; ++j) r = qfma(Bm[2 * j + i], pk[j], r);
            r += lam[2 * (1 + i) + 1] - lam[2 * (1 + i)];
            res[KQ_STAT_U] = fmax(res[KQ_STAT_U], fabs(r));
        }
        if (k >= 1) {
            for (int i = 0; i < 4; ++i) {
                double r = qfma(h[i], x[i], gg[i]);
                for (int j = 0; j < 4; ++j) r = qfma(Am[4 * j + i], pk[j], r);
                r -= pp[i];
                if (i == 3) r += lam[1] - lam[0];
                res[KQ_STAT_X] = fmax(res[KQ_STAT_X], fabs(r));
            }
        }
        for (int i = 0; i < 4; ++i) {
            double r = x1[i] - bv[i];
            for (int j = 0; j < 4; ++j) r = qfma(-Am[4 * i + j], x[j], r);
            for (int j = 0; j < 2; ++j) r = qfma(-Bm[2 * i + j], u[j], r);
            res[KQ_DYN] = fmax(res[KQ_DYN], fabs(r));
        }
        const double v[3] = {x[3], u[0], u[1]};
        for (int j = 0; j < 3; ++j) {
            if (j == 0 && k == 0 && !s0_bound) continue;
            const double tl = v[j] - l[j], th = hh[j] - v[j];
            res[KQ_INFEAS] = fmax(res[KQ_INFEAS], fmax(-tl, -th));
            res[KQ_COMP] = fmax(res[KQ_COMP], fmax(fabs(lam[2 * j] * tl), fabs(lam[2 * j + 1] * th)));
            res[KQ_DUAL] = fmax(res[KQ_DUAL], fmax(-lam[2 * j], -lam[2 * j + 1]));
        }
    } else {
        for (int i = 0; i < 4; ++i) res[KQ_STAT_X] = fmax(res[KQ_STAT_X], fabs(qfma(h[i], x[i], gg[i]) - pp[i]));
    }
    if (k == 0) {
        double z[4];
        fin &= load(z, dx0, 4);
        for (int q = 0; q < 4; ++q) res[KQ_DYN] = fmax(res[KQ_DYN], fabs(x[q] - z[q]));
    }
    return fin;
}

}  // namespace qsp
