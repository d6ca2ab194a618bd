/*
 * qsp_twin.cpp — the CPU oracle's kernel-order twin.
 *
 * TEST INFRASTRUCTURE ONLY.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
 * may load this library, and only as the checker; the product (uclv_qs_pushing_matlab_amd/) never
 * links or calls it.
 *
 * PARITY STATUS: UNPINNED against acados/CasADi/HPIPM (not runnable here), as
 * qsp_oracle.c.  This file runs the same reference path as qsp_oracle.c -- the B-spline contour
 * (acados_nmpc/bspline_shape.m:40-116, 137-152), the motion-cone dynamics
 * (PusherSliderModel.m:503-603), ERK/RK4 with sensitivities (NMPC_controller.m:272), the linear-LS
 * OCP with bgh bounds (NMPC_controller.m:174-268), the Mehrotra interior point standing in for
 * HPIPM (:272-276), fixed-K and merit-backtracking SQP (:271-276), the NMPC_controller.solve
 * wrapper (:329-423) and helper.closed_loop_matlab (helper.m:195-322) -- in the device library's
 * formulation and operation order.
 *
 * Division of labour.  The lane-local arithmetic -- qfma, rcp, sin_cos, the span-based
 * de Boor, the dynamics with its hand-derived Jacobian, RK4, the contact re-projection, the structured
 * Riccati step, the scans' maps and elements, the adjoint and merit stage terms, the IPM's barrier
 * terms, directions, step and exit test, the merit SQP's KKT residuals and updates -- and the per-lane code
 * around the solve -- the shape table's entries, the parameters from the options, which factorisation a
 * handle takes, get_y_ref's staging, the controller's prologue, status rule, shifted warm start and cost,
 * the closed loop's disturbance, delay prediction and input buffers, the building blocks' output layout,
 * the QP-level entry's mapping and status -- are NOT restated here: this file compiles the kernels' own headers
 * (csrc/qsp_fp.hpp, qsp_math.hpp, qsp_riccati.hpp, qsp_ipm.hpp) for the host, with
 * -ffp-contract=off as the library.  What it restates, as plain sequential loops, is the
 * ORCHESTRATION the device runs in DPP moves, LDS records and matrix-core instructions: which lane
 * walks when, the lane-group reductions' summation tree, the scans' levels, the matrix-core
 * product's element order, the IPM and SQP loops, the controller wrapper and the closed loop.
 * Still written out here as in the kernels, each for a measured reason (profiles/ipm_shared/README.md
 * section B): qp_ipm's t.lm sum and centring scalar and load_stage (as shared functions they cost the
 * SQP kernels registers), qp_ipm's start point (registers equal, but 0.4 % slower on the headline
 * workload), merit_ls's directional-derivative term (its kernel's instruction count
 * moves by more than 1 %).  The operations are IEEE-exact on
 * both sides (checked on the device by scripts/ubench/fp_exact.hip), so this twin reproduces the
 * library's results BIT FOR BIT, lane by lane, including lanes where the fixed-K SQP is chaotic:
 * the comparison proves that the GPU's compiler and hardware evaluate the shared source as x86 does
 * and that the device executes the algorithm.  qsp_oracle.c's literal restatement (full basis sum,
 * AD; plain C, no product header) pins the formulas independently to rounding level
 * (tests/test_oracle.py, tests/test_twin.py); tests/golden/twin_bits.npz pins this twin's bits in time.
 * Kernel counterparts are cited as qsp_solver.hip function names.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "or_opts.h"
#include "qsp_layout.h"    /* the library's own layout rules: stages per lane, lanes per instance, factor_walk_of */
#include "qsp_math.hpp"    /* the library's own lane arithmetic: qsp_fp.hpp, the model ... */
#include "qsp_riccati.hpp" /* ... the QP's per-lane steps ... */
#include "qsp_ipm.hpp"     /* ... and the per-stage arithmetic of the interior point and the SQP */

using namespace qsp;

#define TW_MAX_N 128
#define TW_MAX_SLOTS (TW_MAX_N + 2)

/* ------------------------------------------------------------------ shapes (qsp_set_shapes) */
static void make_shape(ShapeDev *d, const int32_t *n_ctrl, const double *ctrl, const double *knots,
                       const double *params, int max_ctrl, int id, double xwidth)
{
    shape_entry(*d, n_ctrl[id], ctrl + (size_t)id * max_ctrl * 2, knots + (size_t)id * (max_ctrl + 4), params[3 * id],
                params[3 * id + 1], params[3 * id + 2], xwidth);
}

/* ================================================================== the QP (qp_ipm) */
typedef struct {
    double a[6], B[8], bb[4], g[6], v[3];
    double K[8], Rn[3], kk[2], M[16];
    double t[6], lm[6], rt[6], hg[6];
    double VA[3], VN[3], du[2], dxs[4];
    double at[6], al[6], dt[6], dl[6];
} tw_stage;

/* one slot as the view qsp_ipm.hpp's functions take (the kernels': Stage<S>, with the slot number ls) */
struct tw_view {
    tw_stage *s;
    double &t(int, int q) const { return s->t[q]; }
    double &lm(int, int q) const { return s->lm[q]; }
    double &rt(int, int q) const { return s->rt[q]; }
    double &v(int, int j) const { return s->v[j]; }
    double &va(int, int j) const { return s->VA[j]; }
    double &vn(int, int j) const { return s->VN[j]; }
    double &hg(int, int i) const { return s->hg[i]; }
    double &du(int, int i) const { return s->du[i]; }
};

/* the solve parameters the kernels read, plus the layout and the factorisation (FactorWalk) they imply
 * (mfw_on / mfw_is, the kernels' record layout, stay unset) */
struct tw_par : SolveParams {
    int S, L, walk;
};

static void make_par(tw_par *p, const or_opts *o)
{
    *p = tw_par{};
    params_from_options(*p, *o);
    p->S = stages_per_lane(o->N, o->nlp_mode, o->stages_per_lane);
    p->L = lanes_per_instance(p->N, p->S);
    /* the library's developer switch, and the twin's own to the lane walk's order */
    p->mfma_walk = mfma_walk_default() && !o->lane_walk;
    p->walk = factor_walk_of(p->N, p->S, p->mfma_walk, p->factor_scan);
    p->tau = o->tau;
    memcpy(p->W, o->W, sizeof p->W);
    memcpy(p->We, o->We, sizeof p->We);
    memcpy(p->lh, o->lh, sizeof p->lh);
    memcpy(p->uh, o->uh, sizeof p->uh);
    p->cp = CtrlParams{o->v_alpha, o->d_v, o->t_angle0, o->u_n_lb, o->u_t_ub};
}

/* The factorisation the twin emulates for these options, in the library's QSP_WALK_* coding
 * (qsp_get_factor_walk reports the library's side of the same choice). */
extern "C" int tw_factor_walk(const or_opts *o)
{
    tw_par p;
    make_par(&p, o);
    return p.walk;
}

/* group_sum: the kernel's log-step shuffle tree towards the group's first lane */
static double group_sum(double *v, int L)
{
    double tmp[64];
    for (int off = 1; off < L; off <<= 1) {
        for (int i = 0; i < L; ++i) tmp[i] = v[i] + ((i + off < L) ? v[i + off] : 0.0);
        memcpy(v, tmp, sizeof(double) * (size_t)L);
    }
    return v[0];
}
/* group_min / group_max of non-NaN values (exact in any order) */
static double group_min(const double *v, int L)
{
    double r = v[L - 1];
    for (int i = L - 2; i >= 0; --i) r = (v[i] < r) ? v[i] : r;
    return r;
}
static double group_max(const double *v, int L)
{
    double r = v[L - 1];
    for (int i = L - 2; i >= 0; --i) r = (v[i] > r) ? v[i] : r;
    return r;
}

/* ---- S = 2: the affine passes as scans (riccati_solve<2, ...>; Aff, aff_*: qsp_riccati.hpp) */
/* the S = 2 difference pass: suffix scan of the lanes' backward maps (slot 1's, then slot 0's;
 * identity past the horizon), dp_N = 0; each slot's dkk from the dp reaching it */
static void delta_scan_s2(const tw_par *p, tw_stage *st, const double *gx3, double (*gu)[2])
{
    const int N = p->N, L = p->L;
    Aff d[64], nd[64];
    for (int l = 0; l < L; ++l) {
        const int k0 = 2 * l;
        if (k0 + 1 < N) {
            const tw_stage *s0 = st + k0, *s1 = st + k0 + 1;
            Aff m1;
            aff_delta(s0->a, s0->B, s0->K, gx3[k0], gu[k0], d[l]);
            aff_delta(s1->a, s1->B, s1->K, gx3[k0 + 1], gu[k0 + 1], m1);
            aff_compose(d[l], m1);
        } else if (k0 < N) {
            aff_delta(st[k0].a, st[k0].B, st[k0].K, gx3[k0], gu[k0], d[l]);
        } else {
            aff_identity(d[l]);
        }
    }
    for (int off = 1; off < L; off <<= 1) {
        for (int l = 0; l < L; ++l) {
            nd[l] = d[l];
            if (l + off < L) aff_compose(nd[l], d[l + off]);
        }
        memcpy(d, nd, sizeof(Aff) * (size_t)L);
    }
    for (int l = 0; l < L; ++l) {
        double pv[4];
        for (int i = 0; i < 4; ++i) pv[i] = (l + 1 < L) ? d[l + 1].c[i] : 0.0;
        for (int ls = 1; ls >= 0; --ls) {
            const int k = 2 * l + ls;
            if (k < N) {
                tw_stage *s = st + k;
                double dkk[2];
                ric_delta_step(s->a, s->B, gx3[k], gu[k], s->K, s->Rn, pv, dkk);
                s->kk[0] += dkk[0];
                s->kk[1] += dkk[1];
            }
        }
    }
}

/* the S = 2 forward pass: prefix scan of the lanes' closed-loop maps (slot 0's, then slot 1's); the
 * state entering lane l is T_{l-1}(dx0); slot 0 forms du and steps the dynamics, slot 1 forms du */
static void forward_scan_s2(const tw_par *p, tw_stage *st, const double dx0[4], int factor)
{
    const int N = p->N, L = p->L;
    Aff e[64], ne[64];
    for (int l = 0; l < L; ++l) {
        const int k0 = 2 * l;
        if (k0 + 1 < N) {   /* the last lane's map is consumed by no lane (values there are unused) */
            const tw_stage *s0 = st + k0, *s1 = st + k0 + 1;
            Aff m1;
            aff_forward(s0->a, s0->B, s0->bb, s0->K, s0->kk, e[l]);
            aff_forward(s1->a, s1->B, s1->bb, s1->K, s1->kk, m1);
            aff_compose(m1, e[l]);
            e[l] = m1;
        } else {
            aff_identity(e[l]);
        }
    }
    for (int off = 1; off < L; off <<= 1) {
        for (int l = 0; l < L; ++l) {
            ne[l] = e[l];
            if (l >= off) aff_compose(ne[l], e[l - off]);
        }
        memcpy(e, ne, sizeof(Aff) * (size_t)L);
    }
    for (int l = 0; l < L; ++l) {
        double dx[4];
        if (l == 0) memcpy(dx, dx0, sizeof dx);
        else aff_apply(e[l - 1], dx0, dx);
        for (int ls = 0; ls < 2; ++ls) {
            const int k = 2 * l + ls;
            if (k >= N) break;
            tw_stage *s = st + k;
            double du[2];
            du[0] = qfma(s->K[3], dx[3], qfma(s->K[2], dx[2], qfma(s->K[1], dx[1], qfma(s->K[0], dx[0], s->kk[0]))));
            du[1] = qfma(s->K[7], dx[3], qfma(s->K[6], dx[2], qfma(s->K[5], dx[1], qfma(s->K[4], dx[0], s->kk[1]))));
            double *out = factor ? s->VA : s->VN;
            out[0] = dx[3];
            out[1] = du[0];
            out[2] = du[1];
            if (ls == 0) dyn_step(s->a, s->B, s->bb, du, dx);
        }
    }
}

/* ---- S = 2: the factorisation as an associative scan (riccati_solve<2, true>): the conditional
 * value-function elements (VElem, velem_*: qsp_riccati.hpp) combined in the kernel's association
 * order; P_k = J, p_k = -eta of the suffix product over k..N */
/* developer check of the element arithmetic (scripts/ubench/velem_check.hip runs the same on the
 * device): per case two stages (a, B, bb, Hx, Hu, gx, gu: 30 doubles each) and a terminal (We, g: 8);
 * out = e0 (x) e1, then (x) the terminal element (We[0] > 0) or (x) e1 (x) e0 (We[0] <= 0): 2 x 44 doubles */
extern "C" void tw_velem_check(int32_t n, const double *in, double *out)
{
    for (int i = 0; i < n; ++i) {
        const double *c = in + (size_t)i * 68;
        VElem e, e1, t;
        velem_stage(c, c + 6, c + 14, c + 18, c + 22, c + 24, c + 28, e);
        velem_stage(c + 30, c + 36, c + 44, c + 48, c + 52, c + 54, c + 58, e1);
        velem_combine(e, e1);
        memcpy(out + (size_t)i * 88, &e, sizeof e);
        const double g6[6] = {c[64], c[65], c[66], c[67], 0.0, 0.0};
        if (c[60] > 0.0) {
            velem_terminal(c + 60, g6, t);
        } else {   /* a general element on the right: the case's two stages combined in the other order */
            VElem u;
            velem_stage(c + 30, c + 36, c + 44, c + 48, c + 52, c + 54, c + 58, t);
            velem_stage(c, c + 6, c + 14, c + 18, c + 22, c + 24, c + 28, u);
            velem_combine(t, u);
        }
        velem_combine(e, t);
        memcpy(out + (size_t)i * 88 + 44, &e, sizeof e);
    }
}

/* the S = 2 factorisation: lane l combines its slots' elements, Hillis-Steele suffix levels over the
 * lanes, slot 1's suffix from the next lane's result; each slot then forms K, Rn, kk from its
 * successor's value function (ric_factor_step without the P update) */
static void factor_scan_s2(const tw_par *p, tw_stage *st, const double *hx3, double (*hu)[2], const double *gx3,
                           double (*gu)[2])
{
    const int N = p->N, L = p->L;
    VElem e[64], ne[64], e1[64];
    for (int l = 0; l < L; ++l) {
        const int k0 = 2 * l, k1 = k0 + 1;
        for (int ls = 0; ls < 2; ++ls) {
            const int k = k0 + ls;
            VElem &d = ls == 0 ? e[l] : e1[l];
            if (k < N) {
                const tw_stage *s = st + k;
                const double Hx[4] = {p->tau * p->W[0], p->tau * p->W[1], p->tau * p->W[2], hx3[k]};
                const double gx[4] = {s->g[0], s->g[1], s->g[2], gx3[k]};
                velem_stage(s->a, s->B, s->bb, Hx, hu[k], gx, gu[k], d);
            } else if (k == N) {
                velem_terminal(p->We, st[N].g, d);
            }
        }
        if (k1 <= N) velem_combine(e[l], e1[l]);
    }
    for (int off = 1; off < L; off <<= 1) {
        for (int l = 0; l < L; ++l) {
            ne[l] = e[l];
            if (l + off < L) velem_combine(ne[l], e[l + off]);
        }
        memcpy(e, ne, sizeof(VElem) * (size_t)L);
    }
    for (int l = 0; l < L; ++l) {
        const int k0 = 2 * l, k1 = k0 + 1;
        if (k1 < N) {
            const VElem &f = e[l + 1];
            velem_combine(e1[l], f);
            double Pn[10], pn[4];
            for (int q = 0; q < 10; ++q) Pn[q] = f.J[q];
            for (int q = 0; q < 4; ++q) pn[q] = -f.eta[q];
            tw_stage *s = st + k1;
            const double gx[4] = {s->g[0], s->g[1], s->g[2], gx3[k1]};
            const double Hx[4] = {p->tau * p->W[0], p->tau * p->W[1], p->tau * p->W[2], hx3[k1]};
            ric_factor_step(s->a, s->B, s->bb, Hx, hu[k1], gx, gu[k1], Pn, pn, s->K, s->Rn, s->kk, false);
        }
        if (k0 < N) {
            double Pn[10], pn[4];
            for (int q = 0; q < 10; ++q) Pn[q] = e1[l].J[q];
            for (int q = 0; q < 4; ++q) pn[q] = -e1[l].eta[q];
            tw_stage *s = st + k0;
            const double gx[4] = {s->g[0], s->g[1], s->g[2], gx3[k0]};
            const double Hx[4] = {p->tau * p->W[0], p->tau * p->W[1], p->tau * p->W[2], hx3[k0]};
            ric_factor_step(s->a, s->B, s->bb, Hx, hu[k0], gx, gu[k0], Pn, pn, s->K, s->Rn, s->kk, false);
        }
    }
}

/* riccati_solve: factor (predictor) or the corrector's difference recursion, then the forward pass
 * writing the bounded solution components into VA (factor) / VN (corrector) */
/* mfma4: D = X'Y + C for 4x4 blocks held row-major (X read transposed, as the kernel's A operand);
 * every element is one fused multiply-add chain over k = 0..3 starting from C, the order of
 * v_mfma_f64_4x4x4_4b_f64 (scripts/ubench/mfma_f64_round.hip: 1 920 000 of 1 920 000 elements) */
static void mfma4(const double X[16], const double Y[16], const double C[16], double D[16])
{
    double T[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double d = C[4 * i + j];
            for (int k = 0; k < 4; ++k) d = fma(X[4 * k + i], Y[4 * k + j], d);
            T[4 * i + j] = d;
        }
    memcpy(D, T, sizeof T);
}

/* factor_walk_mfma (qsp_solver.hip): the factorisation of one stage per lane on the matrix cores.
 * The value function is a full symmetric 4x4 P and p replicated across the columns; a step is
 * T1 = P'A, T2 = P'[B | b | 0] + [0 | 0 | p | 0], Q = A'T1 + Hx, Y = G'T1, Z = G'T2 + [Hu | gu],
 * q = A'pp + gx, K = (-adj R~)'S~ / det, P = Y'K + Q (upper triangle; lower = K'Y + Q' elementwise,
 * its exact transpose), p = K'[r~] + q; the stage keeps K and forms -R~^-1 and kk from Z's R~, r~. */
static void factor_walk_mfma(const tw_par *p, tw_stage *st, const double *hx3, double (*hu)[2], const double *gx3,
                             double (*gu)[2])
{
    const int N = p->N;
    static const double zero[16] = {0};
    double P[16] = {0}, pv[16];
    for (int i = 0; i < 4; ++i) P[5 * i] = p->We[i];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) pv[4 * r + c] = st[N].g[r];
    for (int k = N - 1; k >= 0; --k) {
        tw_stage *s = st + k;
        const double *a = s->a;
        const double Am[16] = {1.0, 0.0, a[0], a[1], 0.0, 1.0, a[2], a[3], 0.0, 0.0, 1.0, a[4], 0.0, 0.0, 0.0, a[5]};
        const double gx[4] = {s->g[0], s->g[1], s->g[2], gx3[k]};
        double G2[16], CH[16] = {0}, CZ[16] = {0}, GQ[16], C2[16] = {0}, PP[16];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                G2[4 * r + c] = c < 2 ? s->B[2 * r + c] : (c == 2 ? s->bb[r] : 0.0);
                GQ[4 * r + c] = gx[r];
            }
        CH[0] = p->tau * p->W[0];
        CH[5] = p->tau * p->W[1];
        CH[10] = p->tau * p->W[2];
        CH[15] = hx3[k];
        CZ[0] = hu[k][0];
        CZ[5] = hu[k][1];
        CZ[2] = gu[k][0];
        CZ[6] = gu[k][1];
        for (int r = 0; r < 4; ++r) C2[4 * r + 2] = pv[4 * r + 2];
        double T1[16], T2[16], Q[16], Y[16], Z[16], QV[16], KA[16], Kf[16];
        mfma4(P, Am, zero, T1);
        mfma4(P, G2, C2, T2);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) PP[4 * r + c] = T2[4 * r + 2];
        mfma4(Am, T1, CH, Q);
        mfma4(G2, T1, zero, Y);
        mfma4(G2, T2, CZ, Z);
        mfma4(Am, PP, GQ, QV);
        const double R00 = Z[0], R01 = Z[1], rt0 = Z[2], R11 = Z[5], rt1 = Z[6];
        const double idet = rcp(qfma(R00, R11, -(R01 * R01)));
        double Xa[16] = {0};
        Xa[0] = -R11; Xa[1] = R01; Xa[4] = R01; Xa[5] = -R00;
        mfma4(Xa, Y, zero, KA);
        for (int q = 0; q < 16; ++q) Kf[q] = KA[q] * (q < 8 ? idet : 0.0);
        for (int q = 0; q < 8; ++q) s->K[q] = Kf[q];
        s->Rn[0] = (-R11) * idet;
        s->Rn[1] = R01 * idet;
        s->Rn[2] = (-R00) * idet;
        s->kk[0] = qfma(s->Rn[1], rt1, s->Rn[0] * rt0);
        s->kk[1] = qfma(s->Rn[2], rt1, s->Rn[1] * rt0);
        if (k > 0) {
            /* P = Q~ + S~'K keeps its upper triangle; the lower one is the same products transposed
             * (K'S~ + Q~', with Q~' = T1'A + Hx: bit for bit the transposes), so P stays symmetric as the
             * lane walk's */
            double RT[16] = {0}, QT[16], PT[16];
            for (int c = 0; c < 4; ++c) { RT[c] = rt0; RT[4 + c] = rt1; }
            mfma4(T1, Am, CH, QT);
            mfma4(Y, Kf, Q, P);
            mfma4(Kf, Y, QT, PT);
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < r; ++c) P[4 * r + c] = PT[4 * r + c];
            mfma4(Kf, RT, QV, pv);
        }
    }
}

static void riccati_solve(const tw_par *p, tw_stage *st, const double dx0[4], int factor)
{
    const int N = p->N, S = p->S;
    double hx3[TW_MAX_SLOTS], hu[TW_MAX_SLOTS][2], gx3[TW_MAX_SLOTS], gu[TW_MAX_SLOTS][2];
    for (int k = 0; k < N; ++k) {
        const tw_stage *s = st + k;
        if (factor) {
            hx3[k] = qfma(p->tau, p->W[3], s->hg[0]);
            hu[k][0] = qfma(p->tau, p->W[4], s->hg[1]);
            hu[k][1] = qfma(p->tau, p->W[5], s->hg[2]);
            gx3[k] = s->g[3] + s->hg[3];
            gu[k][0] = s->g[4] + s->hg[4];
            gu[k][1] = s->g[5] + s->hg[5];
        } else {
            gx3[k] = s->hg[3];
            gu[k][0] = s->hg[4];
            gu[k][1] = s->hg[5];
        }
    }
    if (S == 1 && !factor) {
        /* closed-loop difference walk: dp_k = e_k + (A + B K)' dp_{k+1}, dp_N = 0; each stage k
         * forms kk += Rn (dg_u + B' dp_{k+1}) from the dp that reaches it */
        double dp[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = N - 1; k >= 0; --k) {
            tw_stage *s = st + k;
            double rt[2];
            for (int i = 0; i < 2; ++i)
                rt[i] = qfma(s->B[6 + i], dp[3], qfma(s->B[4 + i], dp[2], qfma(s->B[2 + i], dp[1], qfma(s->B[i], dp[0], gu[k][i]))));
            s->kk[0] = qfma(s->Rn[1], rt[1], qfma(s->Rn[0], rt[0], s->kk[0]));
            s->kk[1] = qfma(s->Rn[2], rt[1], qfma(s->Rn[1], rt[0], s->kk[1]));
            if (k >= 1) {
                double e[4], n[4];
                for (int i = 0; i < 4; ++i) e[i] = qfma(s->K[4 + i], gu[k][1], qfma(s->K[i], gu[k][0], i == 3 ? gx3[k] : 0.0));
                for (int i = 0; i < 4; ++i)
                    n[i] = qfma(s->M[12 + i], dp[3], qfma(s->M[8 + i], dp[2], qfma(s->M[4 + i], dp[1], qfma(s->M[i], dp[0], e[i]))));
                memcpy(dp, n, sizeof dp);
            }
        }
    } else if (S == 2 && !factor) {
        delta_scan_s2(p, st, gx3, gu);
    } else if (factor && p->walk == WALK_SCAN) {
        factor_scan_s2(p, st, hx3, hu, gx3, gu);
    } else if (factor && p->walk == WALK_MFMA) {
        factor_walk_mfma(p, st, hx3, hu, gx3, gu);
    } else {   /* the factorisation by the lane walk (both difference passes are taken above) */
        double P[10], pv[4];
        ric_terminal(*p, st[N].g, P, pv);
        for (int k = N - 1; k >= 0; --k) {
            tw_stage *s = st + k;
            const double gx[4] = {s->g[0], s->g[1], s->g[2], gx3[k]};
            const double Hx[4] = {p->tau * p->W[0], p->tau * p->W[1], p->tau * p->W[2], hx3[k]};
            ric_factor_step(s->a, s->B, s->bb, Hx, hu[k], gx, gu[k], P, pv, s->K, s->Rn, s->kk, k > 0);
        }
    }
    double dx[4] = {dx0[0], dx0[1], dx0[2], dx0[3]};
    if (S == 1) {
        if (factor) {
            for (int k = 0; k < N; ++k) {
                tw_stage *s = st + k;
                const double *a = s->a, *B = s->B, *K = s->K;
                const double Am[4][4] = {{1.0, 0.0, a[0], a[1]}, {0.0, 1.0, a[2], a[3]}, {0.0, 0.0, 1.0, a[4]},
                                         {0.0, 0.0, 0.0, a[5]}};
                for (int i = 0; i < 4; ++i)
                    for (int q = 0; q < 4; ++q) s->M[4 * i + q] = qfma(B[2 * i + 1], K[4 + q], qfma(B[2 * i], K[q], Am[i][q]));
            }
        }
        for (int k = 0; k < N; ++k) {
            tw_stage *s = st + k;
            const double *K = s->K;
            double *out = factor ? s->VA : s->VN;
            out[0] = dx[3];
            out[1] = qfma(K[3], dx[3], qfma(K[2], dx[2], qfma(K[1], dx[1], qfma(K[0], dx[0], s->kk[0]))));
            out[2] = qfma(K[7], dx[3], qfma(K[6], dx[2], qfma(K[5], dx[1], qfma(K[4], dx[0], s->kk[1]))));
            double cv[4], n[4];
            for (int i = 0; i < 4; ++i) cv[i] = qfma(s->B[2 * i + 1], s->kk[1], qfma(s->B[2 * i], s->kk[0], s->bb[i]));
            for (int i = 0; i < 4; ++i)
                n[i] = qfma(s->M[4 * i + 3], dx[3], qfma(s->M[4 * i + 2], dx[2], qfma(s->M[4 * i + 1], dx[1], qfma(s->M[4 * i], dx[0], cv[i]))));
            memcpy(dx, n, sizeof dx);
        }
        return;
    }
    forward_scan_s2(p, st, dx0, factor);
}

/* qp_ipm: slots 0 .. L*S-1 of st are filled (a, B, bb, g, v; padding slots past N hold the terminal
 * stage's data as the kernel loads them).  Returns the iterations taken; *exit why it stopped. */
static int qp_ipm(const tw_par *p, tw_stage *st, const double dx0[4], int *exit, int skip)
{
    const int N = p->N, S = p->S, L = p->L;
    const double m = 2.0 * (3.0 * N - (p->s0_bound ? 0.0 : 1.0));
    /* the start point and its residuals: written out here as in the kernel's qp_ipm (as one shared
     * function it cost the headline workload 0.4 %, profiles/ipm_shared/README.md): edit both */
    double r0 = 0.0, rg0 = 0.0, rb0 = 0.0;
    for (int k = 0; k < L * S; ++k) {
        tw_stage *s = st + k;
        double lo[3], hi[3], gl[3];
        bnd_lohi(*p, tw_view{s}, 0, lo, hi);
        for (int j = 0; j < 3; ++j) {
            const int act = bnd_act(*p, N, k, j);
            const double tl = fmax(-lo[j], p->t_min), th = fmax(hi[j], p->t_min);
            if (act) r0 = fmax(r0, fmax(tl + lo[j], th - hi[j]));
            const double rl = rcp(tl), rh = rcp(th);
            s->t[2 * j] = act ? tl : 1.0;
            s->t[2 * j + 1] = act ? th : 1.0;
            s->rt[2 * j] = act ? rl : 1.0;
            s->rt[2 * j + 1] = act ? rh : 1.0;
            s->lm[2 * j] = act ? p->mu0 * rl : 0.0;
            s->lm[2 * j + 1] = act ? p->mu0 * rh : 0.0;
            gl[j] = act ? qfma(p->mu0, rh, -(p->mu0 * rl)) : 0.0;
        }
        if (k <= N) {
            rg0 = fmax(rg0, fmax(fmax(fabs(s->g[0]), fabs(s->g[1])), fmax(fabs(s->g[2]), fabs(s->g[3] + gl[0]))));
            rg0 = fmax(rg0, fmax(fabs(s->g[4] + gl[1]), fabs(s->g[5] + gl[2])));
            rb0 = fmax(rb0, fmax(fmax(fabs(s->bb[0]), fabs(s->bb[1])), fmax(fabs(s->bb[2]), fabs(s->bb[3]))));
            if (k == 0) rb0 = fmax(rb0, fmax(fmax(fabs(dx0[0]), fabs(dx0[1])), fmax(fabs(dx0[2]), fabs(dx0[3]))));
        }
        s->du[0] = s->du[1] = 0.0;
        for (int q = 0; q < 3; ++q) s->VA[q] = s->VN[q] = 0.0;
    }
    double rs_stop = p->res_stop / r0;
    const double rs_g = p->qp_tol_stat / rg0, rs_b = p->qp_tol_eq / rb0;
    rs_stop = rs_g < rs_stop ? rs_g : rs_stop;
    rs_stop = rs_b < rs_stop ? rs_b : rs_stop;
    double rscale = 1.0;
    int nit = 0, stall = 0;
    bool conv = false, stalled = false, div = false;
    double lane[64], num[64], den[64];
    for (int it = 0;; ++it) {
        for (int l = 0; l < L; ++l) {
            double acc = 0.0;   /* the lane's t.lm sum, as the kernel's loop-top tl_sum */
            for (int ls = 0; ls < S; ++ls)
                for (int q = 0; q < 6; ++q) acc = qfma(st[l * S + ls].t[q], st[l * S + ls].lm[q], acc);
            lane[l] = acc;
        }
        const double mu = group_sum(lane, L) / m;
        ipm_exit_test(*p, mu, rscale, rs_stop, stall, skip != 0, div, conv, stalled);
        const int done = conv || div || stalled;
        if (it == p->qp_iters || done) break;
        nit++;
        /* predictor */
        for (int k = 0; k < L * S; ++k)
            for (int j = 0; j < 3; ++j) barrier_term(*p, N, tw_view{st + k}, 0, k, j, st[k].hg);
        riccati_solve(p, st, dx0, 1);
        for (int l = 0; l < L; ++l) {
            num[l] = 1.0;
            den[l] = 1.0;
            for (int k = l * S; k < l * S + S; ++k) affine_dirs(*p, N, tw_view{st + k}, 0, k, st[k].at, st[k].al, num[l], den[l]);
            lane[l] = num[l] / den[l];
        }
        const double aa = group_min(lane, L);
        for (int l = 0; l < L; ++l) {
            double ma = 0.0;
            for (int k = l * S; k < l * S + S; ++k) ma = affine_mu_part(*p, N, tw_view{st + k}, 0, k, st[k].at, st[k].al, aa, ma);
            lane[l] = ma;
        }
        const double mua = group_sum(lane, L) / m;
        const double r = mua / mu;
        const double sg = fmax(r * r * r, p->sigma_min);
        const double smu = sg * mu;
        /* corrector */
        for (int k = 0; k < L * S; ++k) corrector_terms(*p, N, tw_view{st + k}, 0, k, st[k].at, st[k].al, smu);
        riccati_solve(p, st, dx0, 0);
        for (int l = 0; l < L; ++l) {
            num[l] = 1.0;
            den[l] = p->frac;
            for (int k = l * S; k < l * S + S; ++k)
                corrector_dirs(*p, N, tw_view{st + k}, 0, k, st[k].at, st[k].al, smu, st[k].dt, st[k].dl, num[l], den[l]);
            lane[l] = num[l] / den[l];
        }
        double alpha = p->frac * group_min(lane, L);
        alpha = fmin(alpha, 1.0);
        stall = alpha < p->qp_stall_alpha ? stall + 1 : 0;
        rscale *= 1.0 - alpha;
        for (int k = 0; k < L * S; ++k) {
            apply_step(tw_view{st + k}, 0, st[k].dt, st[k].dl, alpha);
            damp_du(tw_view{st + k}, 0, alpha);
        }
    }
    *exit = ipm_exit_code(conv, div, stalled);
    return nit;
}

/* qp_rollout: state step of the damped QP solution */
static void qp_rollout(const tw_par *p, tw_stage *st, const double dx0[4])
{
    double dx[4] = {dx0[0], dx0[1], dx0[2], dx0[3]};
    for (int k = 0; k <= p->N; ++k) {
        memcpy(st[k].dxs, dx, sizeof dx);
        if (k < p->N) dyn_step(st[k].a, st[k].B, st[k].bb, st[k].du, dx);
    }
}

/* the QP's dynamics multipliers pi_k (k = 0..N-1) by the adjoint recursion (qp_adjoint_store) */
static void qp_adjoint(const tw_par *p, const tw_stage *st, double *PI /* N x 4 */)
{
    const int N = p->N;
    double pi[4];
    for (int i = 0; i < 4; ++i) pi[i] = qfma(p->We[i], st[N].dxs[i], st[N].g[i]);
    for (int k = N - 1; k >= 0; --k) {
        memcpy(PI + 4 * k, pi, sizeof pi);
        if (k >= 1) adjoint_step(*p, st[k].a, st[k].dxs, st[k].g, st[k].lm[1] - st[k].lm[0], pi);
    }
}

/* ================================================================== one instance's SQP */
typedef struct {
    tw_stage st[TW_MAX_SLOTS];
    double nlpPI[TW_MAX_N * 4], LAM[TW_MAX_N * 6], NU[TW_MAX_N * 4], ETA[TW_MAX_N * 6];
    double qPI[TW_MAX_N * 4];
    double kkt[8];   /* diagnostics of the last NLP KKT test (nlp_mode 1): see tw_set_kkt_diag */
} tw_ws;

/* KKT diagnostics (nlp_mode 1), per lane 8 doubles, as or_set_kkt_diag: u-, x- and terminal
 * stationarity, equality, inequality, complementarity residuals of the last KKT test, its SQP
 * iteration, the last line-search step length.  NULL: off. */
static double *g_kkt_diag = NULL;
extern "C" void tw_set_kkt_diag(double *buf) { g_kkt_diag = buf; }

/* stage data of slot k from the SQP iterate (qp_step_kernel's LIN block) */
static void load_stage(const tw_par *p, const ShapeDev *sh, tw_stage *s, int k, const double *X, const double *U,
                       const double *yref, const double *ye, int lin_live)
{
    const int N = p->N;
    const int kc = k <= N ? k : N, ku = k < N ? k : N - 1;
    if (kc < N && lin_live) {
        const double *xk = X + 4 * kc, *uk = U + 2 * kc;
        Lin Ln;
        rk4<true>(*sh, p->Ts, xk, uk, Ln);
        const double *yr = yref + 6 * kc;
        memcpy(s->a, Ln.a, sizeof s->a);
        memcpy(s->B, Ln.B, sizeof s->B);
        for (int q = 0; q < 4; ++q) s->bb[q] = Ln.xn[q] - X[4 * (kc + 1) + q];
        for (int q = 0; q < 4; ++q) s->g[q] = p->tau * p->W[q] * (xk[q] - yr[q]);
        for (int q = 0; q < 2; ++q) s->g[4 + q] = p->tau * p->W[4 + q] * (uk[q] - yr[4 + q]);
    } else {
        memset(s->a, 0, sizeof s->a);
        memset(s->B, 0, sizeof s->B);
        memset(s->bb, 0, sizeof s->bb);
        for (int q = 0; q < 4; ++q) s->g[q] = p->We[q] * (X[4 * N + q] - ye[q]);
        s->g[4] = s->g[5] = 0.0;
    }
    s->v[0] = X[4 * kc + 3];
    s->v[1] = U[2 * ku];
    s->v[2] = U[2 * ku + 1];
}

/* nlp_converged: KKT residuals of the NLP iterate against tol_* (nlp_mode 1) */
static int nlp_converged(const tw_par *p, const tw_stage *st, const double *PI, const double *LAM, double *kkt)
{
    const int N = p->N;
    double re = 0.0, ri = 0.0, rc = 0.0, ru = 0.0, rx = 0.0, rt = 0.0;
    for (int k = 0; k <= N; ++k) {
        const tw_stage *s = st + k;
        const double zero[6] = {0, 0, 0, 0, 0, 0};
        const double *PIk = k < N ? PI + 4 * k : zero, *LAMk = k < N ? LAM + 6 * k : zero;
        const double *PIp = k >= 1 ? PI + 4 * (k - 1) : zero;
        kkt_stage(*p, k, s->a, s->B, s->g, s->bb, s->v, PIk, PIp, LAMk, ru, rx, rt, re, ri, rc);
    }
    const double rs = fmax(fmax(ru, rx), rt);   /* the kernel keeps the three in one maximum */
    kkt[0] = ru; kkt[1] = rx; kkt[2] = rt; kkt[3] = re; kkt[4] = ri; kkt[5] = rc;
    return rs < p->tol_stat && re < p->tol_eq && ri < p->tol_ineq && rc < p->tol_comp;
}

/* merit_ls_kernel for one instance (stages = lanes 0..N of its group) */
static void merit_ls(const tw_par *p, const ShapeDev *sh, tw_ws *w, double *X, double *U, const double *yref,
                     const double *ye)
{
    const int N = p->N, L = N + 1;
    const tw_stage *st = w->st;
    double NUk[TW_MAX_N + 1][4], ETAk[TW_MAX_N + 1][6], dph[TW_MAX_N + 1], lane[64] = {0};
    double xk[TW_MAX_N + 1][4], uk[TW_MAX_N + 1][2], dxk[TW_MAX_N + 1][4], duk[TW_MAX_N + 1][2];
    for (int k = 0; k <= N; ++k) {
        const int stg = k < N, ku = stg ? k : N - 1;
        for (int q = 0; q < 4; ++q) { xk[k][q] = X[4 * k + q]; dxk[k][q] = st[k].dxs[q]; }
        uk[k][0] = U[2 * ku];
        uk[k][1] = U[2 * ku + 1];
        duk[k][0] = stg ? st[k].du[0] : 0.0;
        duk[k][1] = stg ? st[k].du[1] : 0.0;
        for (int q = 0; q < 4; ++q) NUk[k][q] = stg ? w->NU[4 * k + q] : 0.0;
        for (int q = 0; q < 6; ++q) ETAk[k][q] = stg ? w->ETA[6 * k + q] : 0.0;
        if (stg) {
            for (int q = 0; q < 4; ++q) NUk[k][q] = merit_weight(NUk[k][q], fabs(w->qPI[4 * k + q]));
            for (int q = 0; q < 6; ++q) ETAk[k][q] = merit_weight(ETAk[k][q], fabs(st[k].lm[q]));
        }
        double d = 0.0;
        for (int i = 0; i < 4; ++i) d = qfma(st[k].g[i], dxk[k][i], d);
        if (stg) {
            d = qfma(st[k].g[5], duk[k][1], qfma(st[k].g[4], duk[k][0], d));
            for (int i = 0; i < 4; ++i) d = qfma(-NUk[k][i], fabs(st[k].bb[i]), d);
            const double v[3] = {xk[k][3], uk[k][0], uk[k][1]};
            for (int j = 0; j < 3; ++j) {
                if (j == 0 && k == 0 && !p->s0_bound) continue;
                const double lo = p->lh[j] - v[j], hi = p->uh[j] - v[j];
                if (lo > 0.0) d = qfma(-ETAk[k][2 * j], lo, d);
                if (hi < 0.0) d = qfma(ETAk[k][2 * j + 1], hi, d);
            }
        }
        dph[k] = d;
    }
    for (int k = 0; k <= N; ++k) {
        const int ku = k < N ? k : N - 1;
        lane[k] = merit_stage(*p, k, xk[k], uk[k], yref + 6 * ku, ye, st[k].bb, NUk[k], ETAk[k]);
    }
    const double phi0 = group_sum(lane, L);
    for (int k = 0; k <= N; ++k) lane[k] = dph[k];
    const double dphi = group_sum(lane, L);
    double alpha = 1.0;
    for (;;) {
        double xt[TW_MAX_N + 1][4], ut[TW_MAX_N + 1][2];
        for (int k = 0; k <= N; ++k) {
            for (int q = 0; q < 4; ++q) xt[k][q] = qfma(alpha, dxk[k][q], xk[k][q]);
            ut[k][0] = qfma(alpha, duk[k][0], uk[k][0]);
            ut[k][1] = qfma(alpha, duk[k][1], uk[k][1]);
        }
        for (int k = 0; k <= N; ++k) {
            double def[4] = {0.0, 0.0, 0.0, 0.0};
            if (k < N) {
                Lin Lt;
                rk4<false>(*sh, p->Ts, xt[k], ut[k], Lt);
                for (int q = 0; q < 4; ++q) def[q] = Lt.xn[q] - xt[k + 1][q];
            }
            const int ku = k < N ? k : N - 1;
            lane[k] = merit_stage(*p, k, xt[k], ut[k], yref + 6 * ku, ye, def, NUk[k], ETAk[k]);
        }
        const double phi = group_sum(lane, L);
        if (phi <= qfma(p->ls_eps * alpha, dphi, phi0)) break;
        const double an = alpha * p->ls_alpha_red;
        if (an < p->ls_alpha_min) break;
        alpha = an;
    }
    w->kkt[7] = alpha;
    for (int k = 0; k <= N; ++k) {
        for (int q = 0; q < 4; ++q) X[4 * k + q] = qfma(alpha, dxk[k][q], xk[k][q]);
        if (k < N) {
            U[2 * k] = qfma(alpha, duk[k][0], uk[k][0]);
            U[2 * k + 1] = qfma(alpha, duk[k][1], uk[k][1]);
            for (int q = 0; q < 4; ++q) w->nlpPI[4 * k + q] = damp_update(alpha, w->qPI[4 * k + q], w->nlpPI[4 * k + q]);
            for (int q = 0; q < 6; ++q) w->LAM[6 * k + q] = damp_update(alpha, st[k].lm[q], w->LAM[6 * k + q]);
            memcpy(w->NU + 4 * k, NUk[k], sizeof(double) * 4);
            memcpy(w->ETA + 6 * k, ETAk[k], sizeof(double) * 6);
        }
    }
}

typedef struct {
    int status, sqp_iter, qp_iter, qp_capped, qp_stalled;
    int pi_written;
} tw_out;

/* launch_sqp for one instance between prologue and epilogue: X, U (the iterate), x0 (wx0), the
 * staged y_ref; PI_out (N x 4) receives the multipliers (nlp_mode 0: the last successful QP's,
 * shifted when `shift`; nlp_mode 1: the NLP iterate's, written by the epilogue).  PI_in: the
 * initial dynamics multipliers (nlp_mode 1; NULL: zeros). */
static void sqp_solve(const tw_par *p, const ShapeDev *sh, tw_ws *w, const double x0[4], const double *yref,
                      const double *ye, double *X, double *U, const double *PI_in, double *PI_out, int shift,
                      int wdone0, tw_out *o)
{
    const int N = p->N, S = p->S, L = p->L;
    int wdone = wdone0;   /* 0 running, 1 converged (nlp 1), 2 non-finite QP, 3 infeasible s0, 4 diverged QP */
    o->sqp_iter = 0;
    o->qp_iter = 0;
    o->qp_capped = 0;
    o->qp_stalled = 0;
    o->pi_written = 0;
    memset(w->kkt, 0, sizeof w->kkt);
    if (p->nlp_mode == 1) {
        for (int k = 0; k < N; ++k)
            for (int q = 0; q < 4; ++q) w->nlpPI[4 * k + q] = PI_in ? PI_in[4 * k + q] : 0.0;
        memset(w->LAM, 0, sizeof(double) * 6 * N);
        memset(w->NU, 0, sizeof(double) * 4 * N);
        memset(w->ETA, 0, sizeof(double) * 6 * N);
    }
    if (wdone0 == 3) o->sqp_iter = 0;
    for (int it = 0; it < p->sqp_iters; ++it) {
        const int was_done = wdone != 0;
        const int lin_live = !was_done;
        for (int k = 0; k < L * S; ++k) load_stage(p, sh, w->st + k, k, X, U, yref, ye, lin_live);
        double dx0[4];
        for (int q = 0; q < 4; ++q) dx0[q] = x0[q] - X[q];
        int skip = was_done;
        if (p->nlp_mode == 1) {
            const int conv = !was_done && nlp_converged(p, w->st, w->nlpPI, w->LAM, w->kkt);
            if (!was_done) w->kkt[6] = it;
            skip = was_done || conv;
            if (conv) {
                wdone = 1;
                o->sqp_iter = it;
            }
        }
        if (skip && p->nlp_mode == 0) continue;   /* a stopped instance does nothing in nlp_mode 0 */
        int exit;
        const int nit = qp_ipm(p, w->st, dx0, &exit, skip);
        qp_rollout(p, w->st, dx0);
        int failed = 0;
        if (!skip) {
            if (exit == QP_EXIT_CAP) o->qp_capped++;
            if (exit == QP_EXIT_STALL) o->qp_stalled++;
            int bad = 0;
            for (int k = 0; k <= N; ++k)
                for (int q = 0; q < 4; ++q) bad |= !isfinite(w->st[k].dxs[q]);
            for (int k = 0; k < N; ++k) bad |= !(isfinite(w->st[k].du[0]) && isfinite(w->st[k].du[1]));
            const int dv = exit == QP_EXIT_DIVERGED;
            failed = dv || bad;
            if (failed) {
                wdone = dv ? 4 : 2;
                o->sqp_iter = it;
            }
        }
        if (p->nlp_mode == 1) {
            o->qp_iter += nit;
            if (skip || failed) continue;
            qp_adjoint(p, w->st, w->qPI);
            merit_ls(p, sh, w, X, U, yref, ye);
            continue;
        }
        if (failed) continue;
        double pik[TW_MAX_N * 4];
        qp_adjoint(p, w->st, pik);
        shift_rows<4>(N, shift, pik, 4, 1, PI_out);   /* adjoint_from_record's rows */
        o->pi_written = 1;
        for (int k = 0; k <= N; ++k)
            for (int q = 0; q < 4; ++q) X[4 * k + q] += w->st[k].dxs[q];
        for (int k = 0; k < N; ++k) {
            U[2 * k] += w->st[k].du[0];
            U[2 * k + 1] += w->st[k].du[1];
        }
        o->qp_iter += nit;
    }
    /* epilogue_kernel (status; cost and outputs by the callers) */
    o->status = solve_status(*p, iterate_nonfinite(N, X, U, x0), wdone, o->sqp_iter);
    if (p->nlp_mode == 1) {
        shift_rows<4>(N, shift, w->nlpPI, 4, 1, PI_out);
        o->pi_written = 1;
    }
}

/* ================================================================== exported API (as qsp_oracle.c) */
extern "C" {

int tw_spline_eval(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
                   int max_ctrl, int32_t n, const int32_t *shape_id, const double *s,
                   double *C, double *D, double *Dd, double *kappa)
{
    for (int32_t i = 0; i < n; ++i) {
        ShapeDev sh;
        make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
        SplineEval e;
        spline_eval(sh, s[i], e);
        for (int c = 0; c < 2; ++c) { C[2 * i + c] = e.C[c]; D[2 * i + c] = e.D[c]; Dd[2 * i + c] = e.Dd[c]; }
        kappa[i] = angle_rate_of(e);
    }
    return 0;
}

int tw_dynamics(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
                int max_ctrl, int32_t n, const int32_t *shape_id, const double *x, const double *u, double *f, double *J)
{
    #pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < n; ++i) {
        ShapeDev sh;
        make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
        DynOut d;
        dynamics<true>(sh, x[4 * i + 2], x[4 * i + 3], u[2 * i], u[2 * i + 1], d);
        double Jn[24];   /* a caller without J */
        pack_dynamics(d, f + 4 * i, J ? J + (size_t)24 * i : Jn);
    }
    return 0;
}

int tw_rk4(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
           int max_ctrl, int32_t n, const int32_t *shape_id, double h, const double *x, const double *u,
           double *xn, double *A, double *B)
{
    #pragma omp parallel for schedule(static)
    for (int32_t i = 0; i < n; ++i) {
        ShapeDev sh;
        make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
        Lin L;
        rk4<true>(sh, h, x + 4 * i, u + 2 * i, L);
        pack_lin(L, xn + 4 * i, A + (size_t)16 * i, B + (size_t)8 * i);
    }
    return 0;
}

int tw_vbound(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
              int max_ctrl, const or_opts *o, int32_t n, const int32_t *shape_id, const double *s, double *vb)
{
    for (int32_t i = 0; i < n; ++i) {
        ShapeDev sh;
        make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
        vb[i] = v_bound(sh, CtrlParams{o->v_alpha, o->d_v, o->t_angle0, o->u_n_lb, o->u_t_ub}, s[i]);
    }
    return 0;
}

/* QP level (qsp_qp_solve): the library's own mapping onto the kernel's parameters and iterate
 * (qp_level_params, qp_level_iterate) and its qp_status (qp_level_status: 0 stop test met, 1 non-finite,
 * 2 cap, 3 infeasible stage-0 s, 4 stall, 5 diverged), qsp_ipm.hpp. */
int tw_qp_batch(const or_opts *o, int32_t nb, const double *A, const double *B, const double *b,
                const double *H, const double *g, const double *lo, const double *hi, const uint8_t *act,
                const double *dx0, double *dx, double *du, double *pi, double *lam, int32_t *iters, int32_t *qp_status)
{
    (void)act;
    const int N = o->N;
    if (N > TW_MAX_N) return -1;
    tw_par p;
    make_par(&p, o);
    qp_level_params(p, H, lo, hi);
    int fail = 0;
    #pragma omp parallel
    {
        tw_ws *w = (tw_ws *)malloc(sizeof(tw_ws));
        #pragma omp for schedule(dynamic, 4)
        for (int32_t l = 0; l < nb; ++l) {
            const int L = p.L, S = p.S;
            const double *lol = lo + (size_t)l * N * 3, *hil = hi + (size_t)l * N * 3;
            double X[(TW_MAX_N + 1) * 4], U[TW_MAX_N * 2], x0w[4], d0[4];
            qp_level_iterate(N, lol, dx0 + 4 * l, X, U, x0w);
            for (int k = 0; k < L * S; ++k) {
                tw_stage *s = w->st + k;
                const int kc = k <= N ? k : N, ku = k < N ? k : N - 1;
                memset(s, 0, sizeof *s);
                if (kc < N) {
                    const double *Ak = A + ((size_t)l * N + kc) * 16;
                    const double av[6] = {Ak[2], Ak[3], Ak[6], Ak[7], Ak[11], Ak[15]};
                    memcpy(s->a, av, sizeof av);
                    memcpy(s->B, B + ((size_t)l * N + kc) * 8, sizeof s->B);
                    memcpy(s->bb, b + ((size_t)l * N + kc) * 4, sizeof s->bb);
                    memcpy(s->g, g + (size_t)l * (6 * N + 4) + 6 * kc, sizeof s->g);
                } else {
                    memcpy(s->g, g + (size_t)l * (6 * N + 4) + 6 * N, sizeof(double) * 4);
                }
                /* v through the workspace X (s of stage kc; X_N's s is 0) and U (stage ku), as load_stage */
                s->v[0] = X[4 * kc + 3];
                s->v[1] = U[2 * ku];
                s->v[2] = U[2 * ku + 1];
            }
            for (int q = 0; q < 4; ++q) d0[q] = x0w[q] - X[q];   /* the kernels' dx0 = wx0 - X_0 */
            int exit;
            const int nit = qp_ipm(&p, w->st, d0, &exit, 0);
            qp_rollout(&p, w->st, d0);
            for (int k = 0; k <= N; ++k) memcpy(dx + ((size_t)l * (N + 1) + k) * 4, w->st[k].dxs, sizeof(double) * 4);
            for (int k = 0; k < N; ++k) {
                memcpy(du + ((size_t)l * N + k) * 2, w->st[k].du, sizeof(double) * 2);
                memcpy(lam + ((size_t)l * N + k) * 6, w->st[k].lm, sizeof(double) * 6);
            }
            qp_adjoint(&p, w->st, pi + (size_t)l * N * 4);
            if (iters) iters[l] = nit;
            const int qs = qp_level_status(p, dx + (size_t)l * (N + 1) * 4, du + (size_t)l * N * 2, lol, hil, dx0 + 4 * l,
                                           qp_exit_status(exit));
            if (qp_status) qp_status[l] = qs;
            if (qs == 1) {   /* 1 = non-finite only: qp_exit_status never returns it (0, 2, 4, 5), nor the infeasible 3 */
                #pragma omp atomic write
                fail = 1;
            }
        }
        free(w);
    }
    return fail;
}

/* acados-level solve (qsp_solve): X, U = the initial guess in, the solution out; PI: init_pi in
 * (nlp_mode 1), the multipliers out (see sqp_solve); lam: the NLP's bound multipliers (nlp_mode 1). */
int tw_ocp_solve(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
                 int max_ctrl, const or_opts *o, int32_t nb, const int32_t *shape_id,
                 const double *x0, const double *yref, const double *yref_e,
                 double *X, double *U, double *PI, double *lam, int32_t *status, int32_t *iters, int32_t *qp_iter,
                 double *cost, int nthreads, int32_t *qp_capped, int32_t *qp_stalled)
{
    const int N = o->N;
    if (N > TW_MAX_N) return -1;
    tw_par p;
    make_par(&p, o);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    #pragma omp parallel
    {
        tw_ws *w = (tw_ws *)malloc(sizeof(tw_ws));
        #pragma omp for schedule(dynamic, 1)
        for (int32_t i = 0; i < nb; ++i) {
            ShapeDev sh;
            make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
            double *Xi = X + (size_t)i * 4 * (N + 1), *Ui = U + (size_t)i * 2 * N, *Pi = PI + (size_t)i * 4 * N;
            const double *yr = yref + (size_t)i * 6 * N, *ye = yref_e + (size_t)i * 4;
            double PIin[TW_MAX_N * 4];
            memcpy(PIin, Pi, sizeof(double) * 4 * N);
            tw_out out;
            const int w0 = s0_infeasible(p, x0[4 * i + 3]) ? 3 : 0;
            sqp_solve(&p, &sh, w, x0 + 4 * i, yr, ye, Xi, Ui, PIin, Pi, 0, w0, &out);
            status[i] = out.status;
            if (iters) iters[i] = out.sqp_iter;
            if (qp_iter) qp_iter[i] = out.qp_iter;
            if (qp_capped) qp_capped[i] = out.qp_capped;
            if (qp_stalled) qp_stalled[i] = out.qp_stalled;
            if (g_kkt_diag) memcpy(g_kkt_diag + (size_t)8 * i, w->kkt, sizeof w->kkt);
            if (lam) {
                if (p.nlp_mode == 1) memcpy(lam + (size_t)i * 6 * N, w->LAM, sizeof(double) * 6 * N);
                else memset(lam + (size_t)i * 6 * N, 0, sizeof(double) * 6 * N);
            }
            cost[i] = solve_cost(p, Xi, Ui, yr, ye);
        }
        free(w);
    }
    return 0;
}

/* NMPC_controller.solve on one lane (prologue_kernel in controller mode, the SQP, the epilogue's
 * shifted warm start).  Warm X/U/PI + valid in/out; returns the status. */
static int ctrl_lane(const tw_par *p, const ShapeDev *sh, tw_ws *w, const double x0_in[4], const double *traj,
                     int32_t T, int32_t D, int32_t index_time, double *Xw, double *Uw, double *PIw, uint8_t *valid,
                     double u0[2], tw_out *out, double *cost)
{
    const int N = p->N;
    double yref[TW_MAX_N * 6], ye[4], X[(TW_MAX_N + 1) * 4], U[TW_MAX_N * 2];
    stage_yref(traj, T, D, index_time, N, yref, ye);
    double x0[4] = {x0_in[0], x0_in[1], x0_in[2], x0_in[3]};
    const int cold = !*valid;
    controller_guess(*sh, *p, cold, Uw, x0, U, X);   /* with the handle's controller parameters */
    double PIin[TW_MAX_N * 4];
    memcpy(PIin, PIw, sizeof(double) * 4 * N);
    const int w0 = s0_infeasible(*p, x0[3]) ? 3 : 0;
    sqp_solve(p, sh, w, x0, yref, ye, X, U, cold ? NULL : PIin, PIw, 1, w0, out);
    if (cost) *cost = solve_cost(*p, X, U, yref, ye);
    u0[0] = U[0];
    u0[1] = U[1];
    shift_rows<4>(N + 1, 1, X, 4, 1, Xw);
    shift_rows<2>(N, 1, U, 2, 1, Uw);
    *valid = 1;
    return out->status;
}

int tw_controller_solve(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
                        int max_ctrl, const or_opts *o, int32_t nb, const int32_t *shape_id,
                        const double *x0_in, const double *traj, int32_t T, const int32_t *index_time,
                        double *Xw, double *Uw, double *PIw, uint8_t *warm_valid,
                        double *u0, int32_t *status, int32_t *iters, int32_t *qp_iter, double *cost, int nthreads,
                        int32_t *qp_capped, int32_t delay_cols, int32_t traj_per_lane, int32_t *qp_stalled)
{
    const int N = o->N;
    if (N > TW_MAX_N) return -1;
    tw_par p;
    make_par(&p, o);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    #pragma omp parallel
    {
        tw_ws *w = (tw_ws *)malloc(sizeof(tw_ws));
        #pragma omp for schedule(dynamic, 1)
        for (int32_t i = 0; i < nb; ++i) {
            ShapeDev sh;
            make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
            tw_out out;
            status[i] = ctrl_lane(&p, &sh, w, x0_in + 4 * i, traj + (traj_per_lane ? (size_t)i * T * 6 : 0), T,
                                  delay_cols, index_time[i], Xw + (size_t)i * 4 * (N + 1), Uw + (size_t)i * 2 * N,
                                  PIw + (size_t)i * 4 * N, warm_valid + i, u0 + 2 * i, &out, cost + i);
            if (iters) iters[i] = out.sqp_iter;
            if (qp_iter) qp_iter[i] = out.qp_iter;
            if (qp_capped) qp_capped[i] = out.qp_capped;
            if (qp_stalled) qp_stalled[i] = out.qp_stalled;
            if (g_kkt_diag) memcpy(g_kkt_diag + (size_t)8 * i, w->kkt, sizeof w->kkt);
        }
        free(w);
    }
    return 0;
}

/* contact re-projection: reproject_contact, qsp_math.hpp */
int tw_reproject_contact(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
                         int max_ctrl, int32_t n, const int32_t *shape_id, const double *px, const double *py,
                         const double *s0, double *s)
{
    for (int32_t i = 0; i < n; ++i) {
        ShapeDev sh;
        make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], 0.0);
        s[i] = reproject_contact(sh, px[i], py[i], s0[i]);
    }
    return 0;
}

/* helper.closed_loop_matlab on the device (qsp_closed_loop_ex: closed_loop_pre_kernel, the controller
 * solve, plant_kernel), per lane: cold start; the plant's input buffer starts at zero, the
 * controller's u_buff_contr at ubc0 (B x delay_cols x 2, NULL: zero -- as set_delay_comp leaves it). */
int tw_closed_loop(const int32_t *n_ctrl, const double *ctrl, const double *knots, const double *params,
                   int max_ctrl, const or_opts *o, int32_t nb, const int32_t *shape_id, const double *x0_in,
                   const double *traj, int32_t T, const int32_t *index0, int32_t n_steps, const double *noise,
                   int32_t delay_cols, int32_t plant_delay_cols, int32_t dist_step, const double *dist_amp,
                   const double *xwidth, double *Xtraj, double *Xsim, double *Utraj, int32_t *Straj, int nthreads,
                   const double *ubc0)
{
    const int N = o->N;
    if (N > TW_MAX_N || delay_cols < 0 || plant_delay_cols < 0 || delay_cols > 1024 || plant_delay_cols > 1024) return -1;
    tw_par p;
    make_par(&p, o);
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#endif
    if (g_kkt_diag) memset(g_kkt_diag, 0, sizeof(double) * 8 * (size_t)nb);
    #pragma omp parallel
    {
        tw_ws *w = (tw_ws *)malloc(sizeof(tw_ws));
        double *Xw = (double *)malloc(sizeof(double) * 4 * (N + 1)), *Uw = (double *)malloc(sizeof(double) * 2 * N);
        double *PIw = (double *)malloc(sizeof(double) * 4 * N);
        double *ubc = (double *)calloc(2 * (size_t)(delay_cols + 1), sizeof(double));
        double *ubp = (double *)calloc(2 * (size_t)(plant_delay_cols + 1), sizeof(double));
        #pragma omp for schedule(dynamic, 1)
        for (int32_t i = 0; i < nb; ++i) {
            ShapeDev sh;
            make_shape(&sh, n_ctrl, ctrl, knots, params, max_ctrl, shape_id[i], xwidth ? xwidth[shape_id[i]] : 0.0);
            uint8_t valid = 0;
            memset(Xw, 0, sizeof(double) * 4 * (N + 1));
            memset(Uw, 0, sizeof(double) * 2 * N);
            memset(PIw, 0, sizeof(double) * 4 * N);
            memset(ubc, 0, sizeof(double) * 2 * (size_t)(delay_cols + 1));
            if (ubc0 && delay_cols > 0) memcpy(ubc, ubc0 + (size_t)i * delay_cols * 2, sizeof(double) * 2 * (size_t)delay_cols);
            memset(ubp, 0, sizeof(double) * 2 * (size_t)(plant_delay_cols + 1));
            double x[4];
            memcpy(x, x0_in + 4 * i, sizeof x);
            for (int32_t t = 0; t < n_steps; ++t) {
                /* closed_loop_pre_kernel */
                if (dist_step > 0 && t + 1 == dist_step) {
                    disturb_contact(sh, dist_amp ? dist_amp[i] : 0.0, x);
                }
                if (noise)
                    for (int c = 0; c < 4; ++c) x[c] += noise[((size_t)t * nb + i) * 4 + c];
                memcpy(Xtraj + ((size_t)i * (n_steps + 1) + t) * 4, x, sizeof x);
                double xs[4];
                memcpy(xs, x, sizeof xs);
                delay_predict(sh, ShapeCM{}, p.Ts, delay_cols, ubc, xs);
                if (Xsim) memcpy(Xsim + ((size_t)i * n_steps + t) * 4, xs, sizeof xs);
                double u[2];
                tw_out out;
                const int st = ctrl_lane(&p, &sh, w, xs, traj, T, delay_cols, index0[i] + t + delay_cols, Xw, Uw, PIw,
                                         &valid, u, &out, NULL);
                /* plant_kernel */
                double ua[2];
                buffers_step(ubc, delay_cols, ubp, plant_delay_cols, u, ua);
                euler_step(sh, p.Ts, x, ua[0], ua[1]);
                memcpy(Utraj + ((size_t)i * n_steps + t) * 2, u, sizeof u);
                if (Straj) Straj[(size_t)i * n_steps + t] = st;
                if (g_kkt_diag && st == 2) {
                    /* closed loop: per lane, over its status-2 steps, how often each KKT residual
                     * failed (stat, eq, ineq, comp), the steps, those failing stationarity alone,
                     * and those whose stationarity residual is below 1e-3 (near misses) */
                    double *dg = g_kkt_diag + (size_t)8 * i;
                    const double rs = fmax(fmax(w->kkt[0], w->kkt[1]), w->kkt[2]);
                    const int f0 = rs >= p.tol_stat, f1 = w->kkt[3] >= p.tol_eq, f2 = w->kkt[4] >= p.tol_ineq,
                              f3 = w->kkt[5] >= p.tol_comp;
                    dg[0] += f0; dg[1] += f1; dg[2] += f2; dg[3] += f3;
                    dg[4] += 1.0;
                    dg[5] += (f0 && !f1 && !f2 && !f3);
                    dg[6] += rs < 1e-3;
                }
            }
            memcpy(Xtraj + ((size_t)i * (n_steps + 1) + n_steps) * 4, x, sizeof x);
        }
        free(w); free(Xw); free(Uw); free(PIw); free(ubc); free(ubp);
    }
    return 0;
}

}   /* extern "C" */
