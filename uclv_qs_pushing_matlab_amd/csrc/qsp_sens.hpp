// qsp_sens.hpp — solution sensitivities du_k/dx_0 of the OCP at a given point: the stage data of an NLP point
// (qsp_eval_sens), the backward and forward steps of the sensitivity walk (also qsp_qp_sens, on caller-given
// QP data) and the finite flag.  Lane-local straight-line functions like the other arithmetic headers
// (qsp_fp.hpp): hipcc compiles them into qsp_sens.hip, a plain C++ compiler into a host program
// (tests/stubs/sens_main.cpp), as qsp_kkt.hpp.
//
// Definition: the BARRIER-SMOOTHED GAUSS-NEWTON SENSITIVITY of lane i at a point (X, U) with bound multipliers LAM.
//   stage data   A_k, B_k from one RK4 step with sensitivities at (x_k, u_k): point_stage (qsp_point.hpp), as kkt_nlp_stage;
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
// The implied multipliers (LAM not given, PI given) are kkt_nlp_stage's: implied_lam (qsp_point.hpp).  The SQP
// kernels keep a stage load of their own (qsp_solver.hip; the comment above qp_outcome there says why);
// tests/test_gpu_sens.py::test_eval_sens_is_qp_sens_of_its_own_stage_data holds this header's to qsp_eval_rk4.
//
// Non-finite values: every function that reads or produces numbers returns a flag -- all of them finite --
// and the caller turns a lane with one unset flag into NaN in every output.
#pragma once
#include "qsp_point.hpp"
#include "qsp_riccati.hpp"

namespace qsp {

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

// Stage k < N of an NLP point: a (the six free entries of A_k), Bm, and the diagonal Hx, Hu with the barrier
// in it.  r: the point's rows at (lane, k), x0 standing for X's row 0 where given; r.lam: the stage's
// multipliers, or nullptr: the implied ones from r.pi, r.pip (read for k >= 1) and r.yr, or zero where r.pi is
// nullptr too.  At k = N - 1 nothing is computed from x_N (the terminal Hessian is We), it only counts in the
// flag, so that every row of X does.  Returns the finite flag.
QSP_FN bool sens_nlp_stage(const ShapeDev& sh, const SolveParams& p, int s0_bound, double t_floor, int k, const PointRows& r,
                           double a[6], double Bm[8], double Hx[4], double Hu[2]) {
    double x[4], u[2], xn[4], lam[6] = {0, 0, 0, 0, 0, 0};
    bool fin = point_stage(sh, p.Ts, r.x_or_x0(k), r.u, x, u, a, Bm, xn);
    double z[4];
    if (k == p.N - 1) fin &= load(z, r.x1, 4);
    if (r.lam) {
        fin &= load(lam, r.lam, 6);
    } else if (r.pi) {
        double y[6], pk[4], pp[4] = {0, 0, 0, 0};
        fin &= load(y, r.yr, 6) & load(pk, r.pi, 4);
        if (k >= 1) fin &= load(pp, r.pip, 4);
        const double gu[2] = {p.tau * p.W[4] * (u[0] - y[4]), p.tau * p.W[5] * (u[1] - y[5])};
        implied_lam(k, p.tau * p.W[3] * (x[3] - y[3]), gu, a, Bm, pk, pp, lam);
    }
    const double v[3] = {x[3], u[0], u[1]};
    double d[3];
    sens_barrier(p.lh, p.uh, k, s0_bound, t_floor, v, lam, d);
    for (int q = 0; q < 3; ++q) Hx[q] = p.tau * p.W[q];
    Hx[3] = p.tau * p.W[3] + d[0];
    Hu[0] = p.tau * p.W[4] + d[1];
    Hu[1] = p.tau * p.W[5] + d[2];
    return fin && all_finite(Hx, 4) && all_finite(Hu, 2);
}

// P_N = diag(He)
QSP_FN bool sens_terminal(const double He[4], double P[10]) {
    for (int q = 0; q < 10; ++q) P[q] = 0.0;
    P[0] = He[0]; P[4] = He[1]; P[7] = He[2]; P[9] = He[3];
    return all_finite(He, 4);
}

// One backward step: P = P_{k+1} -> P_k and the stage gain K (row-major 2 x 4).  The flag covers the stage
// data, the gain, P and -R^-1, which carries 1/det.
QSP_FN bool sens_back_step(const double a[6], const double Bm[8], const double Hx[4], const double Hu[2], double P[10],
                           double K[8]) {
    const double z[4] = {0.0, 0.0, 0.0, 0.0};
    double pv[4] = {0.0, 0.0, 0.0, 0.0}, Rn[3], kk[2];
    ric_factor_step(a, Bm, z, Hx, Hu, z, z, P, pv, K, Rn, kk, true);
    return all_finite(a, 6) && all_finite(Bm, 8) && all_finite(Hx, 4) && all_finite(Hu, 2) && all_finite(Rn, 3) &&
           all_finite(K, 8) && all_finite(P, 10);
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
    return all_finite(dU, 8) && all_finite(Phi, 16);
}

QSP_FN void sens_identity(double Phi[16]) {
    for (int q = 0; q < 16; ++q) Phi[q] = (q % 5 == 0) ? 1.0 : 0.0;
}

}  // namespace qsp
