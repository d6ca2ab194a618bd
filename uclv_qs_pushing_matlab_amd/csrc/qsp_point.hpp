// qsp_point.hpp — what the evaluators beside the solve path (qsp_kkt.hpp, qsp_sens.hpp) share: the rows, the
// stage and the implied multipliers of a point given by the caller, and the layout of caller-given QP arrays.
// Lane-local functions and plain structs of pointers like the other arithmetic headers (qsp_fp.hpp): for the
// kernels of qsp_kkt.hip and qsp_sens.hip, the host side of qsp_capi.hip and the host programs of tests/stubs.
// The SQP kernels keep a stage load of their own: the comment above qp_outcome (qsp_solver.hip) says why.
#pragma once
#include <stddef.h>

#include "qsp_ipm.hpp"

namespace qsp {

QSP_FN bool all_finite(const double* v, int n) {
    bool f = true;
    for (int q = 0; q < n; ++q) f = f && __builtin_isfinite(v[q]);
    return f;
}
// n values copied; returns their finite flag
QSP_FN bool load(double* dst, const double* src, int n) {
    for (int q = 0; q < n; ++q) dst[q] = src[q];
    return all_finite(dst, n);
}

// The inputs of an NLP point in an evaluator's argument block (qsp_kernels.h); an array not given is nullptr.
struct PointIn {
    const ShapeDev* shapes;
    int32_t n_shapes;
    const int32_t* shape_id;            // B (nullptr: shape 0); clamped into [0, n_shapes)
    const double *x0, *X, *U, *PI;      // B x 4, B x (N+1) x 4, B x N x 2, B x N x 4
    const double *LAM, *yref, *yref_e;  // B x N x 6, B x N x 6, B x 4
};

// The rows of lane i at stage k = 0 .. N.  U, PI, LAM and x_{k+1} have rows k < N only: at k = N the view holds
// their last row (as pi_{k-1} holds row 0 at k = 0), which the stage functions do not read, so every pointer
// stays inside its array.  A row of an array not given is nullptr.  x0 is handed on as it is, because it means
// two things: to qsp_eval_kkt an extra equality row beside x (X's row 0 is still read), to qsp_eval_sens the
// point of stage 0 in place of X's row 0 (x_or_x0).
struct PointRows {
    const double *x0, *x, *x1, *u, *pi, *pip, *lam, *yr;   // x_k, x_{k+1}, u_k, pi_k, pi_{k-1}, lam_k, yref_k (yref_e at N)
    QSP_HD_MEMBER_FN PointRows(const PointIn& in, int N, size_t i, int k) {
        const size_t ku = (size_t)(k < N ? k : N - 1), kp = (size_t)(k >= 1 ? k - 1 : 0), n = (size_t)N;
        const double* X = in.X + i * (n + 1) * 4;
        x0 = in.x0 ? in.x0 + i * 4 : nullptr;
        x = X + 4 * (size_t)k;
        x1 = X + 4 * (ku + 1);
        u = in.U + (i * n + ku) * 2;
        pi = in.PI ? in.PI + (i * n + ku) * 4 : nullptr;
        pip = in.PI ? in.PI + (i * n + kp) * 4 : nullptr;
        lam = in.LAM ? in.LAM + (i * n + ku) * 6 : nullptr;
        yr = k < N ? (in.yref ? in.yref + (i * n + ku) * 6 : nullptr) : (in.yref_e ? in.yref_e + i * 4 : nullptr);
    }
    QSP_HD_MEMBER_FN const double* x_or_x0(int k) const { return (k == 0 && x0) ? x0 : x; }
};

// The stage of a point at k < N: x, u from their rows and one RK4 step with sensitivities at them -- a (the six
// free entries of A_k), Bm (row-major 4 x 2), xn.  Returns the finite flag of all five.
QSP_FN bool point_stage(const ShapeDev& sh, double Ts, const double* xk, const double* uk, double x[4], double u[2],
                        double a[6], double Bm[8], double xn[4]) {
    const bool fin = load(x, xk, 4) & load(u, uk, 2);
    Lin Ln;
    rk4<true>(sh, Ts, x, u, Ln);
    for (int q = 0; q < 6; ++q) a[q] = Ln.a[q];
    for (int q = 0; q < 8; ++q) Bm[q] = Ln.B[q];
    for (int q = 0; q < 4; ++q) xn[q] = Ln.xn[q];
    return fin && all_finite(xn, 4) && all_finite(a, 6) && all_finite(Bm, 8);
}

// The implied multipliers of stage k < N: for each bounded quantity (s_k for k >= 1, u_n, u_t) the stationarity r
// of that component without bound multipliers gives lam_lo = max(r, 0), lam_hi = max(-r, 0); the stage-0 s pair
// is 0.  gs, gu: the cost gradient's s and input components.  tests/sens_ref.py::implied_lam follows it.
QSP_FN void implied_lam(int k, double gs, const double gu[2], const double a[6], const double Bm[8], const double pk[4],
                        const double pp[4], double lam[6]) {
    for (int q = 0; q < 6; ++q) lam[q] = 0.0;
    for (int i = 0; i < 2; ++i) {
        const double r = gu[i] + qfma(Bm[6 + i], pk[3], qfma(Bm[4 + i], pk[2], qfma(Bm[2 + i], pk[1], Bm[i] * pk[0])));
        lam[2 * (1 + i)] = r > 0.0 ? r : 0.0;
        lam[2 * (1 + i) + 1] = r < 0.0 ? -r : 0.0;
    }
    if (k >= 1) {
        const double r = gs - pp[3] + qfma(a[5], pk[3], qfma(a[4], pk[2], qfma(a[3], pk[1], a[1] * pk[0])));
        lam[0] = r > 0.0 ? r : 0.0;
        lam[1] = r < 0.0 ? -r : 0.0;
    }
}

// One lane of the arrays of qsp_qp_solve, qsp_qp_residuals and qsp_qp_sens: per stage k < N a full row-major
// 4 x 4 A_k, a row-major 4 x 2 B_k, b_k (4) and lo_k, hi_k (3: s, u_n, u_t); H and g hold 6 entries per stage
// (x then u) and 4 more for the terminal state.  An array not given is nullptr.  Rows by k = 0 .. N: at k = N
// those of A, B, b, lo, hi are the last stage's (not read, inside the array), those of H and g the terminal four.
struct QpLaneData {
    static constexpr size_t NA = 16, NB = 8, Nb = 4, NBOUND = 3;    // doubles per stage
    static QSP_HD_MEMBER_FN size_t hg(size_t N) { return 6 * N + 4; }   // doubles per lane of H and of g
    const double *A, *B, *b, *H, *g, *lo, *hi;
    int N;
    QSP_HD_MEMBER_FN QpLaneData(const double* A_, const double* B_, const double* b_, const double* H_, const double* g_,
                                const double* lo_, const double* hi_, int N_, size_t i)
        : A(at(A_, i * N_ * NA)), B(at(B_, i * N_ * NB)), b(at(b_, i * N_ * Nb)), H(at(H_, i * hg(N_))), g(at(g_, i * hg(N_))),
          lo(at(lo_, i * N_ * NBOUND)), hi(at(hi_, i * N_ * NBOUND)), N(N_) {}
    QSP_HD_MEMBER_FN const double* Ak(int k) const { return A + NA * ku(k); }
    QSP_HD_MEMBER_FN const double* Bk(int k) const { return B + NB * ku(k); }
    QSP_HD_MEMBER_FN const double* bk(int k) const { return b + Nb * ku(k); }
    QSP_HD_MEMBER_FN const double* Hk(int k) const { return H + 6 * (size_t)k; }
    QSP_HD_MEMBER_FN const double* gk(int k) const { return g + 6 * (size_t)k; }
    QSP_HD_MEMBER_FN const double* lok(int k) const { return lo + NBOUND * ku(k); }
    QSP_HD_MEMBER_FN const double* hik(int k) const { return hi + NBOUND * ku(k); }

    // The pusher-slider structure the Riccati steps assume of A_k (qsp_math.hpp, Lin): has_structure: the ten
    // fixed entries are exactly those of columns e0, e1 and row (0, 0, 1, a23) (a NaN there fails); free_entries:
    // the other six in Lin's order a = {a02, a03, a12, a13, a23, a33}, the order of the L_A fields.
    static QSP_HD_MEMBER_FN bool has_structure(const double* Ak) {
        const double st[10] = {Ak[0] - 1.0, Ak[1], Ak[4], Ak[5] - 1.0, Ak[8], Ak[9], Ak[10] - 1.0, Ak[12], Ak[13], Ak[14]};
        bool ok = true;
        for (int q = 0; q < 10; ++q) ok = ok && st[q] == 0.0;
        return ok;
    }
    static QSP_HD_MEMBER_FN void free_entries(const double* Ak, double a[6]) {
        const double av[6] = {Ak[2], Ak[3], Ak[6], Ak[7], Ak[11], Ak[15]};
        for (int q = 0; q < 6; ++q) a[q] = av[q];
    }
    QSP_HD_MEMBER_FN size_t ku(int k) const { return (size_t)(k < N ? k : N - 1); }
    static QSP_HD_MEMBER_FN const double* at(const double* p, size_t n) { return p ? p + n : nullptr; }
};

}  // namespace qsp
