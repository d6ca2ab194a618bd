// qsp_riccati.hpp — the lane-local arithmetic of the QP: the structured Riccati step and its
// difference form, the stage dynamics, the affine maps and the conditional value-function elements
// of the scans, the adjoint step and the merit function's stage term.  Straight-line functions of a
// lane's own registers; nothing here reads another lane (the walks, scans, reductions and the
// matrix-core product that hand values between lanes are qsp_solver.hip's).  qsp_solver.hip compiles
// them into the kernels; the CPU twin (oracle/qsp_twin.cpp) compiles the same text for the host and
// restates only the orchestration around them (the qualifier macro: qsp_fp.hpp).
#pragma once
#include "qsp_fp.hpp"
#include "qsp_types.h"

namespace qsp {

// symmetric 4x4 stored as 10 entries: (0,0)(0,1)(0,2)(0,3)(1,1)(1,2)(1,3)(2,2)(2,3)(3,3)
QSP_FN int sidx(int i, int j) {
    if (i > j) { int t = i; i = j; j = t; }
    return i == 0 ? j : (i == 1 ? 3 + j : (i == 2 ? 5 + j : 9));
}

// --------------------------------------------------------- Riccati primitives
// Terminal value function: P = diag(We), p = g_N
QSP_FN void ric_terminal(const SolveParams& p, const double g[6], double P[10], double pv[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) P[i] = 0.0;
    P[0] = p.We[0]; P[4] = p.We[1]; P[7] = p.We[2]; P[9] = p.We[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i] = g[i];
}

// One backward factorisation step exploiting A = [[1,0,a0,a1],[0,1,a2,a3],[0,0,1,a4],[0,0,0,a5]].
// Hx, Hu: diagonal stage Hessian (incl. barrier); gx, gu: gradient (incl. barrier).
// Every sum is one left-to-right FMA chain from its additive term (or its first product).
QSP_FN void ric_factor_step(const double a[6], const double B[8], const double bb[4],
                           const double Hx[4], const double Hu[2],
                           const double gx[4], const double gu[2],
                           double P[10], double pv[4],
                           double K[8], double Rn[3], double kk[2], bool upd = true) {
    // full symmetric P
    double Pm[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Pm[i][j] = P[sidx(i, j)];
    // PA (columns 0, 1 of A are e0, e1)
    double PA[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        PA[i][0] = Pm[i][0];
        PA[i][1] = Pm[i][1];
        PA[i][2] = qfma(Pm[i][1], a[2], qfma(Pm[i][0], a[0], Pm[i][2]));
        PA[i][3] = qfma(Pm[i][3], a[5], qfma(Pm[i][2], a[4], qfma(Pm[i][1], a[3], Pm[i][0] * a[1])));
    }
    // PB
    double PB[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            PB[i][j] = qfma(Pm[i][3], B[6 + j], qfma(Pm[i][2], B[4 + j], qfma(Pm[i][1], B[2 + j], Pm[i][0] * B[j])));
    // pp = p + P b
    double pp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        pp[i] = qfma(Pm[i][3], bb[3], qfma(Pm[i][2], bb[2], qfma(Pm[i][1], bb[1], qfma(Pm[i][0], bb[0], pv[i]))));
    // R~ = Hu + B'PB (sym), S~ = B'PA (2x4), r~ = gu + B'pp
    const double R00 = qfma(B[6], PB[3][0], qfma(B[4], PB[2][0], qfma(B[2], PB[1][0], qfma(B[0], PB[0][0], Hu[0]))));
    const double R01 = qfma(B[6], PB[3][1], qfma(B[4], PB[2][1], qfma(B[2], PB[1][1], B[0] * PB[0][1])));
    const double R11 = qfma(B[7], PB[3][1], qfma(B[5], PB[2][1], qfma(B[3], PB[1][1], qfma(B[1], PB[0][1], Hu[1]))));
    // S~ = B'PA = (PB)'A with the structure of A
    double St[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        St[i][0] = PB[0][i];
        St[i][1] = PB[1][i];
        St[i][2] = qfma(PB[1][i], a[2], qfma(PB[0][i], a[0], PB[2][i]));
        St[i][3] = qfma(PB[3][i], a[5], qfma(PB[2][i], a[4], qfma(PB[1][i], a[3], PB[0][i] * a[1])));
    }
    double rt[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
        rt[i] = qfma(B[6 + i], pp[3], qfma(B[4 + i], pp[2], qfma(B[2 + i], pp[1], qfma(B[i], pp[0], gu[i]))));
    // Q~ = Hx + A'PA  (upper triangle), q~ = gx + A'pp
    double Qt[10];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double c0 = PA[0][j], c1 = PA[1][j], c2 = PA[2][j], c3 = PA[3][j];
        if (j >= 0) Qt[sidx(0, j)] = c0;
        if (j >= 1) Qt[sidx(1, j)] = c1;
        if (j >= 2) Qt[sidx(2, j)] = qfma(a[2], c1, qfma(a[0], c0, j == 2 ? Hx[2] + c2 : c2));
        if (j >= 3) Qt[sidx(3, j)] = qfma(a[5], c3, qfma(a[4], c2, qfma(a[3], c1, qfma(a[1], c0, Hx[3]))));
    }
    Qt[0] += Hx[0]; Qt[4] += Hx[1];
    double qt[4];
    qt[0] = gx[0] + pp[0];
    qt[1] = gx[1] + pp[1];
    qt[2] = qfma(a[2], pp[1], qfma(a[0], pp[0], gx[2] + pp[2]));
    qt[3] = qfma(a[5], pp[3], qfma(a[4], pp[2], qfma(a[3], pp[1], qfma(a[1], pp[0], gx[3]))));
    // Rn = -R~^-1 (kept negated: the sign folds into the multiplies)
    const double idet = rcp(qfma(R00, R11, -(R01 * R01)));
    Rn[0] = (-R11) * idet; Rn[1] = R01 * idet; Rn[2] = (-R00) * idet;
    // K = -R~^-1 S~ ; kk = -R~^-1 r~
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        K[j] = qfma(Rn[1], St[1][j], Rn[0] * St[0][j]);
        K[4 + j] = qfma(Rn[2], St[1][j], Rn[1] * St[0][j]);
    }
    kk[0] = qfma(Rn[1], rt[1], Rn[0] * rt[0]);
    kk[1] = qfma(Rn[2], rt[1], Rn[1] * rt[0]);
    // P = Q~ + S~'K ; p = q~ + K'r~ (not at stage 0: nothing reads P_0, p_0; upd is uniform)
    if (!upd) return;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) P[sidx(i, j)] = qfma(St[1][i], K[4 + j], qfma(St[0][i], K[j], Qt[sidx(i, j)]));
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i] = qfma(K[4 + i], rt[1], qfma(K[i], rt[0], qt[i]));
}

// Vector-only backward step of the Mehrotra corrector, on the DIFFERENCE to the predictor:
// the corrector changes only the gradient, by dg = (0, 0, 0, dgx3; dgu0, dgu1) (barrier
// correction terms), and the recursion is linear in the gradient with the same factors, so
//   dr = dgu + B' dp,  dq = dgx + A' dp,  dkk = Rn dr,  dp <- dq + K' dr,  dp_N = 0
// (P b cancels in the difference; kk_corr = kk_pred + dkk).
QSP_FN void ric_delta_step(const double a[6], const double B[8], double dgx3, const double dgu[2],
                          const double K[8], const double Rn[3], double pv[4], double dkk[2]) {
    double rt[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
        rt[i] = qfma(B[6 + i], pv[3], qfma(B[4 + i], pv[2], qfma(B[2 + i], pv[1], qfma(B[i], pv[0], dgu[i]))));
    double qt[4];
    qt[0] = pv[0];
    qt[1] = pv[1];
    qt[2] = qfma(a[2], pv[1], qfma(a[0], pv[0], pv[2]));
    qt[3] = qfma(a[5], pv[3], qfma(a[4], pv[2], qfma(a[3], pv[1], qfma(a[1], pv[0], dgx3))));
    dkk[0] = qfma(Rn[1], rt[1], Rn[0] * rt[0]);
    dkk[1] = qfma(Rn[2], rt[1], Rn[1] * rt[0]);
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i] = qfma(K[4 + i], rt[1], qfma(K[i], rt[0], qt[i]));
}

// dx_{k+1} = A dx + B du + b
QSP_FN void dyn_step(const double a[6], const double B[8], const double bb[4],
                    const double du[2], double dx[4]) {
    const double n0 = qfma(B[1], du[1], qfma(B[0], du[0], qfma(a[1], dx[3], qfma(a[0], dx[2], bb[0] + dx[0]))));
    const double n1 = qfma(B[3], du[1], qfma(B[2], du[0], qfma(a[3], dx[3], qfma(a[2], dx[2], bb[1] + dx[1]))));
    const double n2 = qfma(B[5], du[1], qfma(B[4], du[0], qfma(a[4], dx[3], bb[2] + dx[2])));
    const double n3 = qfma(B[7], du[1], qfma(B[6], du[0], qfma(a[5], dx[3], bb[3])));
    dx[0] = n0; dx[1] = n1; dx[2] = n2; dx[3] = n3;
}

// ------------------------------------------------ the affine maps of the S = 2 scans
struct Aff { double F[16], c[4]; };   // x -> F x + c

// g <- g o f (f applied first), in place row by row: row i of the result needs only row i of g
QSP_FN void aff_compose(Aff& g, const Aff& f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double r[5];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            r[j] = qfma(g.F[4 * i + 3], f.F[12 + j], qfma(g.F[4 * i + 2], f.F[8 + j],
                        qfma(g.F[4 * i + 1], f.F[4 + j], g.F[4 * i] * f.F[j])));
        r[4] = qfma(g.F[4 * i + 3], f.c[3], qfma(g.F[4 * i + 2], f.c[2], qfma(g.F[4 * i + 1], f.c[1],
                    qfma(g.F[4 * i], f.c[0], g.c[i]))));
#pragma unroll
        for (int j = 0; j < 4; ++j) g.F[4 * i + j] = r[j];
        g.c[i] = r[4];
    }
}
QSP_FN void aff_apply(const Aff& m, const double x[4], double y[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        y[i] = qfma(m.F[4 * i + 3], x[3], qfma(m.F[4 * i + 2], x[2], qfma(m.F[4 * i + 1], x[1], qfma(m.F[4 * i], x[0], m.c[i]))));
}
QSP_FN void aff_identity(Aff& m) {
#pragma unroll
    for (int q = 0; q < 16; ++q) m.F[q] = (q % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) m.c[q] = 0.0;
}
// closed-loop forward map of a stage: dx -> (A + B K) dx + (B kk + b)
QSP_FN void aff_forward(const double a[6], const double B[8], const double bb[4], const double K[8],
                       const double kk[2], Aff& m) {
    const double Am[4][4] = {{1.0, 0.0, a[0], a[1]}, {0.0, 1.0, a[2], a[3]}, {0.0, 0.0, 1.0, a[4]}, {0.0, 0.0, 0.0, a[5]}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) m.F[4 * i + q] = qfma(B[2 * i + 1], K[4 + q], qfma(B[2 * i], K[q], Am[i][q]));
        m.c[i] = qfma(B[2 * i + 1], kk[1], qfma(B[2 * i], kk[0], bb[i]));
    }
}
// backward map of the corrector's difference recursion: dp -> (A + B K)' dp + (K' dgu + dgx3 e3)
QSP_FN void aff_delta(const double a[6], const double B[8], const double K[8], double dgx3,
                     const double dgu[2], Aff& m) {
    const double Am[4][4] = {{1.0, 0.0, a[0], a[1]}, {0.0, 1.0, a[2], a[3]}, {0.0, 0.0, 1.0, a[4]}, {0.0, 0.0, 0.0, a[5]}};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) m.F[4 * q + i] = qfma(B[2 * i + 1], K[4 + q], qfma(B[2 * i], K[q], Am[i][q]));
        m.c[i] = qfma(K[4 + i], dgu[1], qfma(K[i], dgu[0], i == 3 ? dgx3 : 0.0));
    }
}

// ---------------------------------- S = 2: the factorisation as an associative scan
// The conditional value-function element of a stage (Sarkka & Garcia-Fernandez, "Temporal
// parallelization of dynamic programming and linear quadratic control", IEEE TAC 2023):
//   e_k = (A, b, C, eta, J) = (A_k, c_k - B Hu^-1 gu, B Hu^-1 B', -gx, diag Hx),
//   e_N = (0, 0, 0, -g_N, We);
// combining e_ij with e_jk (M = (I + C_ij J_jk)^-1):
//   A = A_jk M A_ij, b = A_jk M (b_ij + C_ij eta_jk) + b_jk, C = A_jk M C_ij A_jk' + C_jk,
//   eta = A_ij' M' (eta_jk - J_jk b_ij) + eta_ij, J = A_ij' M' J_jk A_ij + J_ij.
// The suffix product over stages k..N holds the value function of stage k: P_k = J, p_k = -eta.
// (scripts/ubench/riccati_scan_s2.hip: 0.125 ms vs the walk's 0.149 ms per factorisation of the
// configs[4] batch.)
struct VElem { double A[16], b[4], C[10], eta[4], J[10]; };
constexpr int VELEM_N = 44;

QSP_FN void velem_stage(const double a[6], const double B[8], const double bb[4], const double Hx[4],
                       const double Hu[2], const double gx[4], const double gu[2], VElem& e) {
    const double F[16] = {1.0, 0.0, a[0], a[1], 0.0, 1.0, a[2], a[3], 0.0, 0.0, 1.0, a[4], 0.0, 0.0, 0.0, a[5]};
#pragma unroll
    for (int q = 0; q < 16; ++q) e.A[q] = F[q];
    // IEEE division, not rcp: the pivots below are often 1 + tiny, where rcp's refinement of the hardware
    // estimate ends one ulp off the correctly rounded 1/x (scripts/ubench/rcp_check.hip); the division
    // is the correctly rounded 1/x on the device as on the host
    const double ih0 = 1.0 / Hu[0], ih1 = 1.0 / Hu[1];
    const double v0 = ih0 * gu[0], v1 = ih1 * gu[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e.b[i] = qfma(-B[2 * i + 1], v1, qfma(-B[2 * i], v0, bb[i]));
        e.eta[i] = -gx[i];
        const double w0 = B[2 * i] * ih0, w1 = B[2 * i + 1] * ih1;
#pragma unroll
        for (int j = i; j < 4; ++j) {
            e.C[sidx(i, j)] = qfma(w1, B[2 * j + 1], w0 * B[2 * j]);
            e.J[sidx(i, j)] = (i == j) ? Hx[i] : 0.0;
        }
    }
}
QSP_FN void velem_terminal(const double We[4], const double g[6], VElem& e) {
#pragma unroll
    for (int q = 0; q < 16; ++q) e.A[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 10; ++q) { e.C[q] = 0.0; e.J[q] = 0.0; }
#pragma unroll
    for (int q = 0; q < 4; ++q) { e.b[q] = 0.0; e.eta[q] = -g[q]; e.J[sidx(q, q)] = We[q]; }
}
// e <- e (x) f  (e the earlier stages, f the later ones), in place
QSP_FN void velem_combine(VElem& e, const VElem& f) {
    // T = I + C_ij J_jk, inverted in place by Gauss-Jordan without pivoting (C, J symmetric positive
    // semidefinite: the eigenvalues of I + C J are >= 1)
    double T[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            T[i][j] = qfma(e.C[sidx(i, 3)], f.J[sidx(3, j)], qfma(e.C[sidx(i, 2)], f.J[sidx(2, j)],
                      qfma(e.C[sidx(i, 1)], f.J[sidx(1, j)], qfma(e.C[sidx(i, 0)], f.J[sidx(0, j)], i == j ? 1.0 : 0.0))));
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double piv = 1.0 / T[c][c];
        T[c][c] = 1.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) T[c][j] *= piv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double fct = T[r][c];
            T[r][c] = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) T[r][j] = qfma(-fct, T[c][j], T[r][j]);
        }
    }
    // TA = A_jk M ; U = A_ij' M'
    double TA[4][4], Um[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            TA[i][j] = qfma(f.A[4 * i + 3], T[3][j], qfma(f.A[4 * i + 2], T[2][j], qfma(f.A[4 * i + 1], T[1][j], f.A[4 * i] * T[0][j])));
            Um[i][j] = qfma(e.A[12 + i], T[j][3], qfma(e.A[8 + i], T[j][2], qfma(e.A[4 + i], T[j][1], e.A[i] * T[j][0])));
        }
    // w = b_ij + C_ij eta_jk ; z = eta_jk - J_jk b_ij
    double w[4], z[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = qfma(e.C[sidx(i, 3)], f.eta[3], qfma(e.C[sidx(i, 2)], f.eta[2], qfma(e.C[sidx(i, 1)], f.eta[1], qfma(e.C[sidx(i, 0)], f.eta[0], e.b[i]))));
        z[i] = qfma(-f.J[sidx(i, 3)], e.b[3], qfma(-f.J[sidx(i, 2)], e.b[2], qfma(-f.J[sidx(i, 1)], e.b[1], qfma(-f.J[sidx(i, 0)], e.b[0], f.eta[i]))));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e.b[i] = qfma(TA[i][3], w[3], qfma(TA[i][2], w[2], qfma(TA[i][1], w[1], qfma(TA[i][0], w[0], f.b[i]))));
        e.eta[i] = qfma(Um[i][3], z[3], qfma(Um[i][2], z[2], qfma(Um[i][1], z[1], qfma(Um[i][0], z[0], e.eta[i]))));
    }
    // J = (U J_jk) A_ij + J_ij  (needs the old A_ij: before A is replaced)
    {
        double Y[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                Y[i][j] = qfma(Um[i][3], f.J[sidx(3, j)], qfma(Um[i][2], f.J[sidx(2, j)], qfma(Um[i][1], f.J[sidx(1, j)], Um[i][0] * f.J[sidx(0, j)])));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j)
                e.J[sidx(i, j)] = qfma(Y[i][3], e.A[12 + j], qfma(Y[i][2], e.A[8 + j], qfma(Y[i][1], e.A[4 + j], qfma(Y[i][0], e.A[j], e.J[sidx(i, j)]))));
    }
    // C = (TA C_ij) A_jk' + C_jk
    {
        double X[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                X[i][j] = qfma(TA[i][3], e.C[sidx(3, j)], qfma(TA[i][2], e.C[sidx(2, j)], qfma(TA[i][1], e.C[sidx(1, j)], TA[i][0] * e.C[sidx(0, j)])));
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = i; j < 4; ++j)
                e.C[sidx(i, j)] = qfma(X[i][3], f.A[4 * j + 3], qfma(X[i][2], f.A[4 * j + 2], qfma(X[i][1], f.A[4 * j + 1], qfma(X[i][0], f.A[4 * j], f.C[sidx(i, j)]))));
    }
    // A = TA A_ij, column by column (column j of the result needs column j of A_ij only)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double c0 = e.A[j], c1 = e.A[4 + j], c2 = e.A[8 + j], c3 = e.A[12 + j];
#pragma unroll
        for (int i = 0; i < 4; ++i) e.A[4 * i + j] = qfma(TA[i][3], c3, qfma(TA[i][2], c2, qfma(TA[i][1], c1, TA[i][0] * c0)));
    }
}

// ------------------------------------------------------------------ adjoint, merit
// One step of the adjoint recursion  pi_{k-1} = Hx dx_k + gx_k + A_k' pi_k + (lam_hi - lam_lo)_s
QSP_FN void adjoint_step(const SolveParams& p, const double a[6], const double dx[4],
                        const double g[6], double dlam_s, double pi[4]) {
    double np[4];
    np[0] = qfma(p.tau * p.W[0], dx[0], g[0]) + pi[0];
    np[1] = qfma(p.tau * p.W[1], dx[1], g[1]) + pi[1];
    np[2] = qfma(p.tau * p.W[2], dx[2], g[2]) + (qfma(a[2], pi[1], a[0] * pi[0]) + pi[2]);
    np[3] = qfma(p.tau * p.W[3], dx[3], g[3]) + qfma(a[5], pi[3], qfma(a[4], pi[2], qfma(a[3], pi[1], a[1] * pi[0])));
    np[3] += dlam_s;
#pragma unroll
    for (int i = 0; i < 4; ++i) pi[i] = np[i];
}

// l1 merit contribution of stage k (oracle merit_eval): stage cost, nu'|defect|,
// eta'(bound violation) on (s_k, u_n, u_t); the terminal lane adds the terminal cost.
QSP_FN double merit_stage(const SolveParams& p, int k, const double x[4], const double u[2],
                         const double* yr, const double* ye, const double def[4],
                         const double nu[4], const double eta[6]) {
    if (k == p.N) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double r = x[i] - ye[i]; s = qfma(p.We[i] * r, r, s); }
        return 0.5 * s;
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const double r = x[i] - yr[i]; s = qfma(p.W[i] * r, r, s); }
#pragma unroll
    for (int i = 0; i < 2; ++i) { const double r = u[i] - yr[4 + i]; s = qfma(p.W[4 + i] * r, r, s); }
    double ph = 0.5 * p.tau * s;
#pragma unroll
    for (int i = 0; i < 4; ++i) ph = qfma(nu[i], fabs(def[i]), ph);
    const double v[3] = {x[3], u[0], u[1]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j == 0 && k == 0 && !p.s0_bound) continue;
        const double vl = p.lh[j] - v[j], vh = v[j] - p.uh[j];
        if (vl > 0.0) ph = qfma(eta[2 * j], vl, ph);
        if (vh > 0.0) ph = qfma(eta[2 * j + 1], vh, ph);
    }
    return ph;
}

}  // namespace qsp
