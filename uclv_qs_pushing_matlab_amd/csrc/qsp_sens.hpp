// qsp_sens.hpp — solution sensitivities du_k/dx_0 of the OCP at a given point: the stage data of an NLP point
// (qsp_eval_sens), the backward and forward steps of the sensitivity walk (also qsp_qp_sens, on caller-given
// QP data) and the finite flag.  Lane-local straight-line functions like the other arithmetic headers
// (qsp_fp.hpp): hipcc compiles them into qsp_sens.hip, a plain C++ compiler into a host program
// (tests/stubs/sens_main.cpp), as qsp_kkt.hpp.
//
// Definition: the BARRIER-SMOOTHED GAUSS-NEWTON SENSITIVITY of lane i at a point (X, U) with bound multipliers LAM.
//   stage data   A_k, B_k from one RK4 step with sensitivities at (x_k, u_k), exactly as kkt_nlp_stage forms them;
//   Hessian      Hx = tau W[0..3], Hu = tau W[4..5] for k < N and We at N: the cost is linear least squares,
//                so this is the exact Gauss-Newton Hessian;
//   bounds       each of the six bound sides of h = [s; u_n; u_t] at stage k adds lam / max(slack, t_floor) to
//                that component's diagonal entry, slack = v - lh or uh - v (sens_barrier; the s pair at
//                stage 0 only with stage0_s_bound, as everywhere).  An inactive bound (lam = 0) adds nothing,
//                an active one lam / t_floor, which pins the component; as t_floor -> 0 under strict
//                complementarity this tends to the exact active-set sensitivity.  It is also what the interior
//                point's last factorisation holds;
//   backward     P_N = diag(We), then ric_factor_step (qsp_riccati.hpp, not restated) for k = N-1 .. 0 with
//                zero gradient and defect: K_k (2 x 4, du_k = K_k dx_k) and P_k.  Stage 0 does update P here:
//                P_0, the Hessian of the optimal value in dx_0, is an output;
//   forward      Phi_0 = I, dU_k = K_k Phi_k, Phi_{k+1} = A_k Phi_k + B_k dU_k (= (A_k + B_k K_k) Phi_k), column
//                by column through dyn_step (qsp_riccati.hpp) with a zero defect.
// It is the sensitivity of the Gauss-Newton QP at the point, not of the exact-Hessian NLP (no second
// derivatives of the dynamics enter), and parity against acados' own solution sensitivities is unpinned, as
// everywhere: no reference fixture fixes them.
//
// The implied multipliers (LAM not given, PI given) are those of kkt_nlp_stage, written out once more
// (sens_implied_lam): lam_lo = max(r, 0), lam_hi = max(-r, 0) from the component's stationarity r without
// bound multipliers; the stage-0 s pair is 0.  tests/test_gpu_sens.py holds the two statements together.
//
// Non-finite values: every function that reads or produces numbers returns a flag -- all of them finite --
// and the caller turns a lane with one unset flag into NaN in every output.
#pragma once
#include "qsp_ipm.hpp"
#include "qsp_riccati.hpp"

namespace qsp {

QSP_FN bool sens_finite(const double* v, int n) {
    bool f = true;
    for (int q = 0; q < n; ++q) f = f && __builtin_isfinite(v[q]);
    return f;
}

// The barrier diagonal of stage k: d[j] for v = (s, u_n, u_t), both sides of each summed (lower first).
QSP_FN void sens_barrier(const double lh[3], const double uh[3], int k, int s0_bound, double t_floor, const double v[3],
                         const double lam[6], double d[3]) {
    for (int j = 0; j < 3; ++j) {
        d[j] = 0.0;
        if (j == 0 && k == 0 && !s0_bound) continue;
        const double tl = v[j] - lh[j], th = uh[j] - v[j];
        d[j] = lam[2 * j] / fmax(tl, t_floor) + lam[2 * j + 1] / fmax(th, t_floor);
    }
}

// The implied multipliers of stage k < N (kkt_nlp_stage's, see above): y = yref_k, pk = pi_k, pp = pi_{k-1}
// (read for k >= 1).
QSP_FN void sens_implied_lam(const SolveParams& p, int k, const double x[4], const double u[2], const double y[6],
                             const double a[6], const double Bm[8], const double pk[4], const double pp[4], double lam[6]) {
    for (int q = 0; q < 6; ++q) lam[q] = 0.0;
    for (int i = 0; i < 2; ++i) {
        const double gu = p.tau * p.W[4 + i] * (u[i] - y[4 + i]);
        const double r = gu + qfma(Bm[6 + i], pk[3], qfma(Bm[4 + i], pk[2], qfma(Bm[2 + i], pk[1], Bm[i] * pk[0])));
        lam[2 * (1 + i)] = r > 0.0 ? r : 0.0;
        lam[2 * (1 + i) + 1] = r < 0.0 ? -r : 0.0;
    }
    if (k >= 1) {
        const double gs = p.tau * p.W[3] * (x[3] - y[3]);
        const double r = gs - pp[3] + qfma(a[5], pk[3], qfma(a[4], pk[2], qfma(a[3], pk[1], a[1] * pk[0])));
        lam[0] = r > 0.0 ? r : 0.0;
        lam[1] = r < 0.0 ? -r : 0.0;
    }
}

// Stage k < N of an NLP point: a (the six free entries of A_k), Bm, and the diagonal Hx, Hu with the barrier
// in it.  xk: x_k; uk: u_k; LAMk: the stage's multipliers, or nullptr: the implied ones from PIk, PIp
// (= pi_{k-1}, read for k >= 1) and yr = yref_k, or zero where PIk is nullptr too.  xN: x_N at k = N - 1, else
// nullptr -- nothing is computed from it (the terminal Hessian is We), it only counts in the flag, so that
// every row of X does.  Returns the finite flag.
QSP_FN bool sens_nlp_stage(const ShapeDev& sh, const SolveParams& p, int s0_bound, double t_floor, int k, const double* xk,
                           const double* uk, const double* yr, const double* PIk, const double* PIp, const double* LAMk,
                           const double* xN, double a[6], double Bm[8], double Hx[4], double Hu[2]) {
    double x[4], u[2], lam[6] = {0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) x[q] = xk[q];
    for (int q = 0; q < 2; ++q) u[q] = uk[q];
    bool fin = sens_finite(x, 4) && sens_finite(u, 2);
    if (xN) {
        double z[4];
        for (int q = 0; q < 4; ++q) z[q] = xN[q];
        fin = fin && sens_finite(z, 4);
    }
    Lin Ln;
    rk4<true>(sh, p.Ts, x, u, Ln);
    fin = fin && sens_finite(Ln.xn, 4) && sens_finite(Ln.a, 6) && sens_finite(Ln.B, 8);
    for (int q = 0; q < 6; ++q) a[q] = Ln.a[q];
    for (int q = 0; q < 8; ++q) Bm[q] = Ln.B[q];
    if (LAMk) {
        for (int q = 0; q < 6; ++q) lam[q] = LAMk[q];
        fin = fin && sens_finite(lam, 6);
    } else if (PIk) {
        double y[6], pk[4], pp[4] = {0, 0, 0, 0};
        for (int q = 0; q < 6; ++q) y[q] = yr[q];
        for (int q = 0; q < 4; ++q) pk[q] = PIk[q];
        if (k >= 1) {
            for (int q = 0; q < 4; ++q) pp[q] = PIp[q];
        }
        fin = fin && sens_finite(y, 6) && sens_finite(pk, 4) && sens_finite(pp, 4);
        sens_implied_lam(p, k, x, u, y, a, Bm, pk, pp, lam);
    }
    const double v[3] = {x[3], u[0], u[1]};
    double d[3];
    sens_barrier(p.lh, p.uh, k, s0_bound, t_floor, v, lam, d);
    for (int q = 0; q < 3; ++q) Hx[q] = p.tau * p.W[q];
    Hx[3] = p.tau * p.W[3] + d[0];
    Hu[0] = p.tau * p.W[4] + d[1];
    Hu[1] = p.tau * p.W[5] + d[2];
    return fin && sens_finite(Hx, 4) && sens_finite(Hu, 2);
}

// P_N = diag(He)
QSP_FN bool sens_terminal(const double He[4], double P[10]) {
    for (int q = 0; q < 10; ++q) P[q] = 0.0;
    P[0] = He[0]; P[4] = He[1]; P[7] = He[2]; P[9] = He[3];
    return sens_finite(He, 4);
}

// One backward step: P = P_{k+1} -> P_k and the stage gain K (row-major 2 x 4).  The flag covers the stage
// data, the gain, P and -R^-1, which carries 1/det.
QSP_FN bool sens_back_step(const double a[6], const double Bm[8], const double Hx[4], const double Hu[2], double P[10],
                           double K[8]) {
    const double z[4] = {0.0, 0.0, 0.0, 0.0};
    double pv[4] = {0.0, 0.0, 0.0, 0.0}, Rn[3], kk[2];
    ric_factor_step(a, Bm, z, Hx, Hu, z, z, P, pv, K, Rn, kk, true);
    return sens_finite(a, 6) && sens_finite(Bm, 8) && sens_finite(Hx, 4) && sens_finite(Hu, 2) && sens_finite(Rn, 3) &&
           sens_finite(K, 8) && sens_finite(P, 10);
}

// One forward step: dU = K Phi (row-major 2 x 4), then Phi <- A Phi + B dU.  Phi is kept by columns:
// Phi[4 * j + i] = d x_k[i] / d x_0[j].
QSP_FN bool sens_fwd_step(const double a[6], const double Bm[8], const double K[8], double Phi[16], double dU[8]) {
    const double z[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < 4; ++j) {
        double* c = Phi + 4 * j;
        double du[2];
        for (int i = 0; i < 2; ++i)
            du[i] = qfma(K[4 * i + 3], c[3], qfma(K[4 * i + 2], c[2], qfma(K[4 * i + 1], c[1], K[4 * i] * c[0])));
        dU[j] = du[0];
        dU[4 + j] = du[1];
        dyn_step(a, Bm, z, du, c);
    }
    return sens_finite(dU, 8) && sens_finite(Phi, 16);
}

QSP_FN void sens_identity(double Phi[16]) {
    for (int q = 0; q < 16; ++q) Phi[q] = (q % 5 == 0) ? 1.0 : 0.0;
}

}  // namespace qsp
