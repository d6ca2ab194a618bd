// qsp_kkt.hpp — KKT residuals recomputed from given numbers: one stage of an NLP iterate (X, U, PI, LAM
// against the OCP: qsp_eval_kkt) and one stage of a QP point (dx, du, pi, lam against caller-given QP
// data: qsp_qp_residuals).  Lane-local straight-line functions like the other arithmetic headers
// (qsp_fp.hpp): hipcc compiles them into qsp_kkt.hip, a plain C++ compiler into a host program
// (tests/stubs/kkt_main.cpp), as qsp_noise.hpp.
//
// kkt_nlp_stage writes the stage load of the SQP kernels out once more (qsp_solver.hip, the LIN branch of
// qp_step_kernel: defect bb = xn - x_{k+1}, gradient g = tau W (x - yr), terminal g = We (x_N - ye)) and
// hands it to kkt_stage (qsp_ipm.hpp) unchanged, so that on the merit SQP's converged lanes it reproduces
// that solver's last test bit for bit (tests/test_gpu_kkt.py::test_reproduces_the_merit_sqp_test holds
// the copies together).  The copy is deliberate: the comment above qp_outcome (qsp_solver.hip) records
// what sharing the stage load costs the SQP kernels in registers.
//
// Non-finite values: kkt_stage folds with fmax, which drops a NaN.  Both stage functions therefore return
// a flag beside their maxima -- every value the stage read, and its linearisation, is finite -- and the
// caller turns a lane with one unset flag into NaN (kkt_fold / the kernels' reduction).
#pragma once
#include "qsp_ipm.hpp"

namespace qsp {

// columns of the NLP parts table (QSP_KKT_* of include/qsp_nmpc.h) and of the QP residuals (counts: qsp_types.h)
enum KktPart : int { KP_STAT_U = 0, KP_STAT_X = 1, KP_STAT_TERM = 2, KP_EQ_DYN = 3, KP_EQ_X0 = 4, KP_INEQ = 5, KP_COMP = 6 };
enum KktQpRes : int { KQ_STAT_U = 0, KQ_STAT_X = 1, KQ_DYN = 2, KQ_INFEAS = 3, KQ_COMP = 4, KQ_DUAL = 5 };

QSP_FN bool kkt_finite(const double* v, int n) {
    bool f = true;
    for (int q = 0; q < n; ++q) f = f && __builtin_isfinite(v[q]);
    return f;
}

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
// stage (0 where the stage has none).  xk: x_k; uk, xk1 = x_{k+1}, PIk, LAMk: stage k's, read for k < N
// only; yr: yref_k (6) for k < N, yref_e (4) at k = N; PIp = pi_{k-1}, read for k >= 1; x0: read at k = 0,
// nullptr: x_0 is taken as the initial state (KP_EQ_X0 = 0).  LAMk == nullptr: the implied multipliers --
// for each bounded quantity of the stage (s_k for k >= 1, u_n, u_t) the raw stationarity r of that
// component (kkt_stage's expression with LAMk = 0) gives lam_lo = max(r, 0), lam_hi = max(-r, 0); the
// stage-0 s multipliers are 0.  That component's stationarity is then zero by construction and the
// optimality gap shows in KP_COMP; at a KKT point with strict complementarity they are the multipliers.
// Returns the finite flag.
QSP_FN bool kkt_nlp_stage(const ShapeDev& sh, const SolveParams& p, int k, const double* xk, const double* uk,
                          const double* xk1, const double* yr, const double* PIk, const double* PIp, const double* LAMk,
                          const double* x0, double part[KKT_NPARTS]) {
    const int N = p.N;
    double a[6], Bm[8], bb[4], g[6], pk[4] = {0, 0, 0, 0}, pp[4] = {0, 0, 0, 0}, lam[6] = {0, 0, 0, 0, 0, 0};
    double x[4], u[2] = {0, 0};
    for (int q = 0; q < 4; ++q) x[q] = xk[q];
    bool fin = kkt_finite(x, 4);
    if (k >= 1) {
        for (int q = 0; q < 4; ++q) pp[q] = PIp[q];   // (checked by stage k - 1)
    }
    if (k < N) {
        double x1[4], y[6];
        for (int q = 0; q < 2; ++q) u[q] = uk[q];
        for (int q = 0; q < 4; ++q) x1[q] = xk1[q];   // (checked by stage k + 1)
        for (int q = 0; q < 6; ++q) y[q] = yr[q];
        for (int q = 0; q < 4; ++q) pk[q] = PIk[q];
        fin = fin && kkt_finite(u, 2) && kkt_finite(y, 6) && kkt_finite(pk, 4);
        Lin Ln;
        rk4<true>(sh, p.Ts, x, u, Ln);
        fin = fin && kkt_finite(Ln.xn, 4) && kkt_finite(Ln.a, 6) && kkt_finite(Ln.B, 8);
        for (int q = 0; q < 6; ++q) a[q] = Ln.a[q];
        for (int q = 0; q < 8; ++q) Bm[q] = Ln.B[q];
        for (int q = 0; q < 4; ++q) bb[q] = Ln.xn[q] - x1[q];
        for (int q = 0; q < 4; ++q) g[q] = p.tau * p.W[q] * (x[q] - y[q]);
        for (int q = 0; q < 2; ++q) g[4 + q] = p.tau * p.W[4 + q] * (u[q] - y[4 + q]);
        if (LAMk) {
            for (int q = 0; q < 6; ++q) lam[q] = LAMk[q];
            fin = fin && kkt_finite(lam, 6);
        } else {
            for (int i = 0; i < 2; ++i) {
                const double r = g[4 + i] + qfma(Bm[6 + i], pk[3], qfma(Bm[4 + i], pk[2], qfma(Bm[2 + i], pk[1], Bm[i] * pk[0])));
                lam[2 * (1 + i)] = r > 0.0 ? r : 0.0;
                lam[2 * (1 + i) + 1] = r < 0.0 ? -r : 0.0;
            }
            if (k >= 1) {
                const double r = g[3] - pp[3] + qfma(a[5], pk[3], qfma(a[4], pk[2], qfma(a[3], pk[1], a[1] * pk[0])));
                lam[0] = r > 0.0 ? r : 0.0;
                lam[1] = r < 0.0 ? -r : 0.0;
            }
        }
    } else {   // terminal stage: no dynamics
        double y[4];
        for (int q = 0; q < 4; ++q) y[q] = yr[q];
        fin = fin && kkt_finite(y, 4);
        for (int q = 0; q < 6; ++q) a[q] = 0.0;
        for (int q = 0; q < 8; ++q) Bm[q] = 0.0;
        for (int q = 0; q < 4; ++q) bb[q] = 0.0;
        for (int q = 0; q < 4; ++q) g[q] = p.We[q] * (x[q] - y[q]);
        g[4] = 0.0;
        g[5] = 0.0;
    }
    const double v[3] = {x[3], u[0], u[1]};
    double ru = 0.0, rx = 0.0, rt = 0.0, re = 0.0, ri = 0.0, rc = 0.0, r0 = 0.0;
    kkt_stage(p, k, a, Bm, g, bb, v, pk, pp, lam, ru, rx, rt, re, ri, rc);
    if (k == 0 && x0) {
        double z[4];
        for (int q = 0; q < 4; ++q) z[q] = x0[q];
        fin = fin && kkt_finite(z, 4);
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
// k >= 1, dx0 at k = 0.  Returns the finite flag.
QSP_FN bool kkt_qp_stage(int N, int s0_bound, int k, const double* A, const double* B, const double* b, const double* H,
                         const double* g, const double* lo, const double* hi, const double* dx0, const double* dxk,
                         const double* duk, const double* dxk1, const double* PIk, const double* PIp, const double* LAMk,
                         double res[KKT_QP_NRES]) {
    double x[4], pp[4] = {0, 0, 0, 0};
    const int nh = k < N ? 6 : 4;
    double h[6], gg[6];
    for (int q = 0; q < 4; ++q) x[q] = dxk[q];
    for (int q = 0; q < nh; ++q) { h[q] = H[q]; gg[q] = g[q]; }
    bool fin = kkt_finite(x, 4) && kkt_finite(h, nh) && kkt_finite(gg, nh);
    if (k >= 1) {
        for (int q = 0; q < 4; ++q) pp[q] = PIp[q];   // (checked by stage k - 1)
    }
    for (int q = 0; q < KKT_QP_NRES; ++q) res[q] = 0.0;
    if (k < N) {
        double Am[16], Bm[8], bv[4], l[3], hh[3], u[2], x1[4], pk[4], lam[6];
        for (int q = 0; q < 16; ++q) Am[q] = A[q];
        for (int q = 0; q < 8; ++q) Bm[q] = B[q];
        for (int q = 0; q < 4; ++q) { bv[q] = b[q]; x1[q] = dxk1[q]; pk[q] = PIk[q]; }
        for (int q = 0; q < 3; ++q) { l[q] = lo[q]; hh[q] = hi[q]; }
        for (int q = 0; q < 2; ++q) u[q] = duk[q];
        for (int q = 0; q < 6; ++q) lam[q] = LAMk[q];
        fin = fin && kkt_finite(Am, 16) && kkt_finite(Bm, 8) && kkt_finite(bv, 4) && kkt_finite(pk, 4) && kkt_finite(l, 3) &&
              kkt_finite(hh, 3) && kkt_finite(u, 2) && kkt_finite(lam, 6);   // (x1 checked by stage k + 1)
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
        for (int q = 0; q < 4; ++q) z[q] = dx0[q];
        fin = fin && kkt_finite(z, 4);
        for (int q = 0; q < 4; ++q) res[KQ_DYN] = fmax(res[KQ_DYN], fabs(x[q] - z[q]));
    }
    return fin;
}

}  // namespace qsp
