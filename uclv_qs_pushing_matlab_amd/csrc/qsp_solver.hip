// qsp_solver.hip — batched pusher–slider NMPC solve on gfx950 (FP64).
//
// Lane layout: one NMPC instance owns a group of L = ceil((N+1)/S)
// consecutive lanes of a wavefront; lane `lig` of the group owns the S horizon
// stages k = lig*S .. lig*S+S-1 (stage N is the terminal stage).  Every per-stage
// quantity (stage model, IPM slacks/multipliers, Riccati factors) lives in that
// lane's VGPRs or its LDS column for the whole QP; nothing spills to HBM between
// IPM iterations.  Stage-parallel work (barrier terms, step lengths) runs on all
// lanes at once; the horizon recursions (Riccati backward, state forward, adjoint)
// walk the group lane by lane, handing the 4x4 value function / state step to the
// neighbour lane with one DPP wave shift.  With one stage per lane the walks after the
// factorisation run in closed-loop form (one 4x4 affine map per step).
//
// One solve = prologue (NMPC_controller.solve wrapper) + K x qp_step [linearisation
// (RK4 + sensitivities, one lane per stage) and one QP per instance] + epilogue.
// Before each QP launch the instances are packed into waves by the IPM iteration
// count of their previous QP, longest first (sort_by_iters_kernel, on a histogram the
// QP kernel accumulates).
//
// Algorithm (restating the reference OCP, NMPC_controller.m:174-300):
//   SQP  : nlp_mode 0 — fixed-K full Gauss-Newton steps (BASELINE "SQP-RTI, K iterations");
//          nlp_mode 1 — the reference's 'SQP' + 'merit_backtracking': KKT test with
//          tol 1e-6, l1-merit Armijo backtracking (qp_step<1, true> + merit_ls_kernel)
//   QP   : box-constrained LQ-OCP, Mehrotra predictor-corrector interior point,
//          Riccati factorisation reused by the corrector, whose backward pass runs
//          on the difference to the predictor (stands in for HPIPM);
//          stops on mu < mu_stop and bound residual < res_stop, or at qp_iters
//   model: RK4 (1 step, h = Ts) + forward sensitivities of f (qsp_math.hpp)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/qsp_nmpc.h"
#include "qsp_layout.h"
#include "qsp_math.hpp"
#include "qsp_riccati.hpp"
#include "qsp_ipm.hpp"
#include "qsp_kernels.h"

#ifndef QSP_MIN_WAVES
#define QSP_MIN_WAVES 1
#endif

namespace qsp {

// Diagnostic build only (-DQSP_SEGSTAMP, scripts/segstamps.py): wave cycles per QP-kernel segment, summed
// over the waves by lane 0 of each (s_memtime; the stamps themselves cost ~10 % of the wave time).
#ifdef QSP_SEGSTAMP
#ifndef QSP_SEGMASK
#define QSP_SEGMASK 0xffffffffu   // which segments are stamped (fewer stamps: less distortion)
#endif
__device__ unsigned long long g_seg[32];
__device__ __forceinline__ unsigned long long seg_now() { return __builtin_amdgcn_s_memtime(); }
__device__ __forceinline__ void seg_add(int i, unsigned long long t0) {
    if (!((QSP_SEGMASK >> i) & 1u)) return;
    const unsigned long long t = seg_now();
    if ((threadIdx.x & 63) == 0) atomicAdd(&g_seg[i], t - t0);
}
#define SEG_T(v) unsigned long long v = seg_now()
#define SEG_ADD(i, v) seg_add(i, v)
#define SEG_NEXT(i, v) do { seg_add(i, v); v = seg_now(); } while (0)
#else
#define SEG_T(v)
#define SEG_ADD(i, v)
#define SEG_NEXT(i, v)
#endif

// ------------------------------------------------------------- group helpers
// Reductions over the L lanes of an instance group (lanes base .. base+L-1), leaving the
// same value in every lane of the group (identical decisions in all lanes of an instance).
// Minima and maxima: a segmented inclusive scan over the whole wave with DPP row shifts
// (1, 2, 4, 8 inside each row of 16) and the row broadcasts of lanes 15 and 31 —
// register-to-register moves on the VALU, no LDS round trip — gathers the group's value in
// its last lane; one shuffle broadcasts it.  A lane takes a shifted value only when its
// source lane lies in the same group, so groups of any length L <= 64 and any alignment
// reduce independently.  Sums: see group_sum.
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_move(double v) {
    // lanes without a source (row edge, rows outside ROWS) read 0, which the caller's group
    // mask never takes.  (update_dpp, not mov_dpp: the move must stay outside the masked
    // select — a DPP read from a lane disabled by EXEC does not return that lane's value.)
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false);
    return __hiloint2double(hi, lo);
}

// Lane masks of a compiled horizon (NC > 0; lane_mask_*: qsp_layout.h).  A lane test whose outcome is known
// when the kernel is built is taken from the 64-bit constant: the scalar pair is the region's exec mask as it
// stands, where the per-lane form pays a v_cmp, holds the mask in scalar registers through the IPM loop and
// spills it (fetched back by v_readlane).  Taken so: the closed-loop lane walks' one region each, the stage role
// lig < N and the factor walk's publish and collect regions.  Measured and not taken: the group reductions'
// levels and scan flags, the factor walk's block-lane roles (profiles/lane_masks/README.md).
__device__ __forceinline__ bool lanes_in(lane_mask_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
template <lane_mask_t M>   // a mask the build knows: a literal, never evaluated on the device
__device__ __forceinline__ bool lanes_of() { return lanes_in(M); }
// A lane test that some lane of every wave reaching it passes (by the wave's geometry or the enclosing loop's
// exit condition), used directly as the `if` condition.  The compiler guards a divergent region with a branch
// around it for the wave in which no lane enters (s_cbranch_execz); told that the region is always entered it
// drops that branch, which such a wave never takes and resolves all the same at every pass.  The hint changes no
// result: a region run under an empty exec mask does nothing.  (A macro, not a function: the weight belongs to
// the branch it is written on, and is lost through an inlined function; [[likely]] on the statement gives the
// same code.)  Taken so: the regions of the three closed-loop lane walks, and the runtime-horizon kernels'
// lane tests (lane-walk factorisation steps, stage role, factor-walk publish and collect, the scans' take).
// Measured and not taken: the compiled kernel's constant stage-role, publish and collect regions
// (profiles/skip_branches/README.md).
// Never on a test that data decides (a frozen instance, the ratio tests, bnd_act): such a region can be empty.
#define QSP_SOME_LANE(cond) __builtin_expect_with_probability((cond), true, 1.0)

// Which scan steps a lane takes (its source lane lies in the same group); computed once.
struct GroupScan {
    bool s1, s2, s4, s8, b15, b31;
    int last;   // the group's last lane, where the scan completes
    int base, L;
    __device__ void init(int base_, int L_) {
        base = base_;
        L = L_;
        const int lane = (int)(threadIdx.x & 63);
        const int lig = lane - base_, col = lane & 15, row = lane >> 4;
        s1 = col >= 1 && lig >= 1;
        s2 = col >= 2 && lig >= 2;
        s4 = col >= 4 && lig >= 4;
        s8 = col >= 8 && lig >= 8;
        b15 = (row & 1) && lig > col;          // row_bcast:15 into rows 1, 3 (source 16 row - 1)
        b31 = row >= 2 && lig >= lane - 31;    // row_bcast:31 into rows 2, 3 (source 31)
        last = base_ + L_ - 1;
    }
};

// op(v, take ? o : identity) as a select on the moved value (never a branch: the DPP move
// must execute with every lane enabled)
struct OpMin {
    __device__ double operator()(double v, double o, bool take) const { return (take && o < v) ? o : v; }
};
struct OpMax {
    __device__ double operator()(double v, double o, bool take) const { return (take && o > v) ? o : v; }
};

template <class Op>
__device__ __forceinline__ double group_reduce(double v, const GroupScan& g, Op op) {
    v = op(v, dpp_move<0x111, 0xf>(v), g.s1);    // row_shr:1
    v = op(v, dpp_move<0x112, 0xf>(v), g.s2);    // row_shr:2
    v = op(v, dpp_move<0x114, 0xf>(v), g.s4);    // row_shr:4
    v = op(v, dpp_move<0x118, 0xf>(v), g.s8);    // row_shr:8
    v = op(v, dpp_move<0x142, 0xa>(v), g.b15);   // row_bcast:15
    v = op(v, dpp_move<0x143, 0xc>(v), g.b31);   // row_bcast:31
    return __shfl(v, g.last);
}
// Sums keep a log-step shuffle tree towards the group's first lane: its association depends
// only on the lane's place in the group, so an instance's result does not depend on where
// the wave packing puts it (a row-aligned scan would round differently at another offset;
// min and max are exact in any order).
__device__ __forceinline__ double group_sum(double v, const GroupScan& g) {
    const int lane = (int)(threadIdx.x & 63);
    const int lig = lane - g.base;
    for (int off = 1; off < g.L; off <<= 1) {
        const double o = __shfl(v, lane + off);
        v += (lig + off < g.L) ? o : 0.0;
    }
    return __shfl(v, g.base);
}
// The same tree with NP pieces of work that do not depend on the sum, work(0) .. work(NP - 1), placed
// under it.  Every level of the tree ends in an LDS round trip (ds_bpermute) with nothing of the sum's
// own to issue meanwhile.  For 16 < L <= 32 (wave-uniform) the five levels are written out, so that
// they and the pieces between them are one straight-line region the scheduler can interleave; any
// other L does the pieces first and takes the loop.  Partner, mask and the first-lane read are
// group_sum's: the association does not change.
template <int NP, class Work>
__device__ __forceinline__ double group_sum_over(double v, const GroupScan& g, Work work) {
    if (g.L > 16 && g.L <= 32) {
        const int lane = (int)(threadIdx.x & 63);
        const int lig = lane - g.base;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int off = 1 << i;
            const double o = __shfl(v, lane + off);
#pragma unroll
            for (int q = 0; q < NP; ++q)
                if (q * 5 / NP == i) work(q);
            v += (lig + off < g.L) ? o : 0.0;
        }
        return __shfl(v, g.base);
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) work(q);
    return group_sum(v, g);
}
// group_sum with its levels written out where they can be: what the caller issues next and does not
// need the sum for (operand loads) moves under the round trips.
__device__ __forceinline__ double group_sum_flat(double v, const GroupScan& g) {
    return group_sum_over<0>(v, g, [](int) {});
}
__device__ __forceinline__ double group_min(double v, const GroupScan& g) { return group_reduce(v, g, OpMin()); }
__device__ __forceinline__ double group_max(double v, const GroupScan& g) { return group_reduce(v, g, OpMax()); }

// rcp(x): 1/x from the hardware reciprocal and two Newton steps (qsp_fp.hpp; ≈ 5 instructions
// instead of the ≈ 10 of the IEEE division sequence, and the correctly rounded 1/x)
// sidx, the Riccati step and its difference form, dyn_step, the scans' maps and elements (Aff, VElem),
// adjoint_step and merit_stage -- everything that works on a lane's own registers only: qsp_riccati.hpp

// Wave packing.  wnit holds an instance's last four IPM iteration counts c1 | c2 << 8 |
// c3 << 16 | c4 << 24 (c1 the last; 0 = not yet recorded).  The fixed-K SQP settles into
// period-2 cycles on many lanes, so the count two iterations back predicts the coming QP
// better than the last one (bench workload, oracle: equal to it on 71 % of the QPs against
// 58 %).  The key orders by the prediction p = c2 where the lane repeats with period 2
// (c2 == c4), else c1, longest first (LPT, so a launch does not end on a tail of long waves),
// ties by c2.  Over 50 SQP iterations of 3 072 bench lanes (3 instances per wave) waves then
// run 1.060x the mean iteration count, against 1.065x ordering by (c1, c2), 1.094x by c1 alone
// and 1.244x unsorted (perfect prediction: 1.001x).
// PACK_KEYS_MAX = (maxkey + 1)^2 keys (qsp_kernels.h).
// key levels: IPM counts above 31 share the last level (qp_iters up to 50 and more: the
// acados default cap; such QPs are rare, ~0.1 % of the bench workload's)
__host__ __device__ __forceinline__ int pack_maxkey(int qp_iters) { return qp_iters < 31 ? qp_iters : 31; }
__device__ __forceinline__ int pack_key(int packed, int maxkey) {
    const int c1 = packed & 0xff, c2 = (packed >> 8) & 0xff, c4 = (packed >> 24) & 0xff;
    const int pred = (c4 != 0 && c2 == c4) ? c2 : c1;
    const int p = min(max(pred, 0), maxkey), q = min(max(c2, 0), maxkey);
    return (maxkey - p) * (maxkey + 1) + (maxkey - q);
}
__device__ __forceinline__ int pack_record(int old, int nit) { return (int)(((unsigned)old << 8) | (unsigned)(nit & 0xff)); }

// ------------------------------------------------------------- per-lane state
// The LDS fields of a lane (LdsField) and the workgroup's LDS size: qsp_layout.h.
constexpr int BLOCK = WAVE;                // threads per workgroup: one wave (see launch_qp_waves)
constexpr int lds_bytes(int S) { return lds_doubles(S) * 8; }

template <int S>
struct Stage {
    double g[S][6];          // cost gradient (stage: tau W (y - y_ref); terminal: We (x - y_ref_e))
    double a[S][6];          // free entries of A_k (qsp_math.hpp rk4)
    double B[S][8];
    double bb[S][4];         // defect phi(x_k,u_k) - x_{k+1}
    double K[S][8], Rn[S][3], kk[S][2];   // Rn = -R~^-1
    double* lds;             // this thread's column of the workgroup's LDS block
    __device__ __forceinline__ double& f(int field, int ls, int i) const { return lds[((field + i) * S + ls) * BLOCK]; }
    __device__ __forceinline__ double& t(int ls, int q) const { return f(F_T, ls, q); }
    __device__ __forceinline__ double& lm(int ls, int q) const { return f(F_LM, ls, q); }
    __device__ __forceinline__ double& v(int ls, int i) const { return f(F_V, ls, i); }
    __device__ __forceinline__ double& du(int ls, int i) const { return f(F_DU, ls, i); }
    __device__ __forceinline__ double& dxs(int ls, int i) const { return f(F_DX, ls, i); }
    __device__ __forceinline__ double& hg(int ls, int i) const { return f(F_HG, ls, i); }
    __device__ __forceinline__ double& rt(int ls, int q) const { return f(F_RT, ls, q); }
    // with the accessors above, the view of this lane's slots that qsp_ipm.hpp's functions take
    __device__ __forceinline__ double& va(int ls, int j) const { return f(F_VA, ls, j); }
    __device__ __forceinline__ double& vn(int ls, int j) const { return f(F_VN, ls, j); }
};

struct Ctx {
    int lane, L, grp, lig, base, N;
    int mis;   // compiled horizon: doubles between the instances' factor-walk records (else -1: SolveParams::mfw_is)
    bool real;
    int inst;
    GroupScan gs;
};

// Wave geometry of a thread (qsp_layout.h): its group of L lanes, its place in it, and the instance
// of the launch's range [0, nI) the group holds (real: there is one).
// NC > 0: the horizon as a compile-time constant (the caller launches such a kernel only at
// p.N == NC, launch_qp_any).  Everything derived from it -- L, G, the IPM's m, the factor walk's phase
// split and record stride, every walk's trip count and the form of the group sums -- then folds, where
// the kernel of a runtime horizon (NC = 0) recomputes it, holds it in registers or spills it.
template <int S, int NC = 0>
__device__ __forceinline__ Ctx ctx_of(int lane, int N, int nI) {
    Ctx c;
    if (NC) N = NC;
    c.lane = lane;
    c.N = N;
    c.L = lanes_per_instance(N, S);
    const int G = WAVE / c.L;
    c.mis = NC ? mfw_stride(mfw_records(NC), instances_per_wave(NC, S)) : -1;
    c.grp = c.lane / c.L;
    c.lig = c.lane - c.grp * c.L;
    c.base = c.grp * c.L;
    c.gs.init(c.base, c.L);
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    c.inst = wave * G + c.grp;
    c.real = (c.grp < G) && (c.inst < nI);
    return c;
}

template <int S>
__device__ __forceinline__ int kof(const Ctx& c, int ls) { return c.lig * S + ls; }

// chain hand-over along the wavefront without an LDS round trip (DPP wave shift)
// (lanes without a source keep their own value, so the move can be done in place)
__device__ __forceinline__ double wave_from_next(double v) {   // lane i <- lane i+1
    const int l = __double2loint(v), h = __double2hiint(v);
    const int lo = __builtin_amdgcn_update_dpp(l, l, 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(h, h, 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// lane i <- lane i+1's v; lanes without a source keep `old`.  With old = the value
// the register held before the step, a hand-over inside a divergent region needs no
// extra copy to merge the lanes that sat the step out.
__device__ __forceinline__ double wave_from_next(double old, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), 0x130, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// lane i <- lane i-1's v; lane 0 keeps `old` (the walks never read it there), so the
// result can take old's register in a loop without a copy
__device__ __forceinline__ double wave_from_prev(double old, double v) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_from_prev(double v) {   // lane i <- lane i-1
    const int l = __double2loint(v), h = __double2hiint(v);
    const int lo = __builtin_amdgcn_update_dpp(l, l, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(h, h, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// ------------------------------------- S = 1: the factorisation on the FP64 matrix cores
// The factor walk's step is a handful of 4x4 products, which v_mfma_f64_4x4x4_4b_f64 computes for
// four independent blocks of 16 lanes at once: lane l holds element (l >> 4, l & 3) of block
// (l >> 2) & 3 of each operand, and the A operand is read transposed (mfma4(X, Y, C) = X'Y + C per
// block; scripts/ubench/mfma_f64_probe.hip).  Block b walks instance min(b, G - 1) of the wave with
// its value function held one element per lane, so a step costs eleven matrix-core products and
// ~45 VALU instead of the lane walk's ~210 VALU on 1 of 21 lanes.
// The stage data reaches the blocks through LDS: before the walk every stage lane writes a
// 27-double record (MfwSlot) over the fields that are free while the predictor factorises (F_VA ..
// F_HG and mfw_extra(S) more); the block lanes read their operand elements from it, one step ahead,
// and write the stage's K and [R~ | r~] back over its first 16 slots, which the stage lane collects
// after the walk (forming -R~^-1 and kk itself, in parallel).  The records of a wave's G instances do not fit at once: the walk runs in two
// phases (stages H .. N-1 with the terminal record, then 0 .. H-1).
// (a record row-major in the order the block lanes read it: [B | b] row by row, so the lanes of two matrix
// rows read at most six consecutive doubles per operand, which the three instances' records -- 9 apart
// mod 32 at N = 20 -- keep on disjoint LDS banks)
// (MfwSlot, MfwOut, MfwConst and the region's size: qsp_layout.h)
static_assert(mfw_region(1) >= 33 * MFW_REC + C_COUNT, "S = 1: records of G (N/2 + 1) stages, 12 <= N <= 31");
static_assert(mfw_region(2) >= 64 * MFW_REC + C_COUNT, "S = 2: records of G (N/2 + 1) stages, N <= 127");
// The walk's prefetch reads one record past a phase's last stage: for block 0 in phase 1 that is the
// record below the region, on the live fields F_T .. F_RT, and must stay inside the allocation.
static_assert(F_VA * BLOCK >= MFW_REC, "the record below the region lies in the workgroup's LDS");

__device__ __forceinline__ double mfma4(double a, double b, double c) {   // a'b + c per 4x4 block
    return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}
// The walk hands data between lanes of the one wave through LDS (stage lanes publish, block lanes read,
// and back).  LDS executes a wave's instructions in order; this makes the order explicit to the compiler
// (no instruction on a single wave).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int CTRL>
__device__ __forceinline__ double quad_bcast(double v) {   // DPP quad_perm: one lane of each quad to all four
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// Which horizons take the walk: mfw_fits (qsp_layout.h).  One stage per lane takes it as its ALT kernel
// variant; two stages per lane by a uniform switch, since ALT is the factorisation scan there.
__host__ __device__ __forceinline__ bool mfw_use(const SolveParams& p, int S) { return p.mfw_on[S - 1] != 0; }
// (host, whenever N or mfma_walk change: the kernels read the choice and the stride instead of searching it)
void mfw_prepare(SolveParams& p) {
    for (int S = 1; S <= 2; ++S) {
        const int G = instances_per_wave(p.N, S), CM = mfw_records(p.N);
        p.mfw_on[S - 1] = p.mfma_walk != 0 && mfw_fits(p.N, S);
        p.mfw_is[S - 1] = G >= 1 && G <= 4 ? mfw_stride(CM, G) : CM * MFW_REC;
    }
}

// (NC: the horizon where it is compiled in, one stage per lane; the publish and collect regions' lanes are
// then lane_mask_mfw_publish's and lane_mask_mfw_collect's constants)
template <int S, int NC = 0>
__device__ __forceinline__ void factor_walk_mfma(const Ctx& c, const SolveParams& p, Stage<S>& st, const double (&hx3)[S],
                                                 const double (&hu)[S][2], const double (&gx3)[S], const double (&gu)[S][2]) {
    const int N = c.N, G = WAVE / c.L;
    const int H = mfw_split(N);                   // phase split (CM = mfw_records(N) records per instance and phase)
    const int IS = c.mis >= 0 ? c.mis : p.mfw_is[S - 1];   // doubles from one instance's records to the next's (mfw_prepare)
    double* const reg = st.lds - (threadIdx.x & 63) + F_VA * S * BLOCK;
    // block-lane geometry and the record slot of each operand element (-1: structural constant)
    // (an opaque lane id: derived from c.lane, the geometry would be hoisted out of the IPM loop and
    // kept live through it)
    int l = c.lane;
    asm volatile("" : "+v"(l));
    const int b = (l >> 2) & 3, r = l >> 4, cc = l & 3;
    const int bg = b < G ? b : G - 1;   // a block beyond the wave's instances walks the last one again, bit for bit
    // each operand element's record slot (-1: a structural constant, read from the constant slots instead)
    int ao = -1;
    if (cc >= 2 && r < 2) ao = R_A + 2 * r + (cc - 2);
    else if (cc == 3 && r >= 2) ao = R_A + 2 + r;
    const int go = cc < 3 ? R_G + 3 * r + cc : -1;
    const int ho = (r == 3 && cc == 3) ? R_HX3 : -1;   // Q's C (Hx): only hx3 varies
    int zo = -1;                                       // Z's C: Hu on the diagonal, gu in column 2
    if (r < 2 && r == cc) zo = R_HU + r;
    else if (r < 2 && cc == 2) zo = R_GU + r;
    const int qo = cc == 2 ? R_GX + r : -1;            // q~'s C: gx in column 2 (p lives there only)
    double* const cst = reg + mfw_region(S) - C_COUNT;
    const int ac = r == cc ? C_ONE : C_ZERO, hc = r == cc && r < 3 ? C_HX + r : C_ZERO;
    if (c.lane < C_COUNT)   // the constants (the region's other fields change between walks)
        cst[c.lane] = c.lane == C_ONE ? 1.0 : (c.lane == C_ZERO ? 0.0 : p.tau * p.W[c.lane < C_HX ? 0 : c.lane - C_HX]);
    double P = 0.0, pv = 0.0;
    for (int ph = 0; ph < 2; ++ph) {
        const int kb = ph == 0 ? H : 0, ke = ph == 0 ? N : H - 1;   // records kb .. ke
        // publish: the stage lanes write the records of their slots' stages (one stage per lane written
        // as the lane test: the slot loop, the same test, costs the S = 1 kernel 2 % in issue order)
        if constexpr (S == 1) {
            if (NC ? (ph == 0 ? lanes_of<lane_mask_mfw_publish(NC, 0)>() : lanes_of<lane_mask_mfw_publish(NC, 1)>())
                   : QSP_SOME_LANE(c.grp < G && c.lig >= kb && c.lig <= ke)) {
                double* rw = reg + c.grp * IS + (c.lig - kb) * MFW_REC;
                if (NC ? lanes_of<lane_mask_stage(NC, 1)>() : QSP_SOME_LANE(c.lig < N)) {
#pragma unroll
                    for (int q = 0; q < 6; ++q) rw[R_A + q] = st.a[0][q];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        rw[R_G + 3 * q] = st.B[0][2 * q];
                        rw[R_G + 3 * q + 1] = st.B[0][2 * q + 1];
                        rw[R_G + 3 * q + 2] = st.bb[0][q];
                    }
#pragma unroll
                    for (int q = 0; q < 3; ++q) rw[R_GX + q] = st.g[0][q];
                    rw[R_GX + 3] = gx3[0];
                    rw[R_HX3] = hx3[0];
                    rw[R_HU] = hu[0][0];
                    rw[R_HU + 1] = hu[0][1];
                    rw[R_GU] = gu[0][0];
                    rw[R_GU + 1] = gu[0][1];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) rw[R_GX + q] = st.g[0][q];   // terminal: p_N = g_N
                }
            }
        } else {
    #pragma unroll
            for (int ls = 0; ls < S; ++ls) {
                const int k = kof<S>(c, ls);
                if (QSP_SOME_LANE(c.grp < G && k >= kb && k <= ke)) {
                    double* rw = reg + c.grp * IS + (k - kb) * MFW_REC;
                    if (k < N) {
    #pragma unroll
                        for (int q = 0; q < 6; ++q) rw[R_A + q] = st.a[ls][q];
    #pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            rw[R_G + 3 * q] = st.B[ls][2 * q];
                            rw[R_G + 3 * q + 1] = st.B[ls][2 * q + 1];
                            rw[R_G + 3 * q + 2] = st.bb[ls][q];
                        }
    #pragma unroll
                        for (int q = 0; q < 3; ++q) rw[R_GX + q] = st.g[ls][q];
                        rw[R_GX + 3] = gx3[ls];
                        rw[R_HX3] = hx3[ls];
                        rw[R_HU] = hu[ls][0];
                        rw[R_HU + 1] = hu[ls][1];
                        rw[R_GU] = gu[ls][0];
                        rw[R_GU + 1] = gu[ls][1];
                    } else {
    #pragma unroll
                        for (int q = 0; q < 4; ++q) rw[R_GX + q] = st.g[ls][q];   // terminal: p_N = g_N
                    }
                }
            }
        }
        wave_lds_sync();
        const double* rb = reg + bg * IS;   // this block's records of the phase
        if (ph == 0) {
            P = r == cc ? (r == 0 ? p.We[0] : (r == 1 ? p.We[1] : (r == 2 ? p.We[2] : p.We[3]))) : 0.0;
            pv = cc == 2 ? rb[(N - kb) * MFW_REC + R_GX + r] : 0.0;   // p_N = g_N (column 2)
        }
        const int kf = ph == 0 ? N - 1 : H - 1;
        // Where a lane stores its element of K and of Z in the phase's first record (mfw_store_k, mfw_store_z:
        // qsp_layout.h).  At one stage per lane every lane stores: the stores need no exec mask and the closing
        // products are free to pass them: rows 0, 1 to the output slots; rows 2, 3 to dump slots among the
        // record's operand slots 16 .. 23, dead by then (all of record k is read one step before step k runs, by
        // the prefetch below, and only slots 0 .. 15 are read again, by the collect; the terminal record, whose
        // p_N is read above, is never stored to); a duplicate block (b >= G) to the addresses of the block it
        // repeats, with the same values.
        // (indexed by the step's offset, constant where the horizon is compiled in: pointers stepping one record
        // down per step make the compiler roll that kernel's walk again.  Two stages per lane keep the lane
        // test: that kernel's registers are full, and each form of the full-wave stores tried costs
        // qp_step_kernel<2, false, true, false> 68 bytes of scratch -- scripts/kres.sh)
        double* const wk = reg + bg * IS + mfw_store_k(r, cc);
        double* const wz = reg + bg * IS + mfw_store_z(r, cc);
        // one step of the walk from its operand elements (Am: A, G2: [B | b | 0], CH and CZ: the C operands
        // of Q and Z, gq: gx); p lives in column 2 of pv, zero in the others, so T2 takes it as its C operand
        auto step = [&](int k, double Am, double G2, double CH, double CZ, double gq) {
            const double T1 = mfma4(P, Am, 0.0);                    // P'A
            const double T2 = mfma4(P, G2, pv);                     // P'[B | b | 0] + [0 | 0 | p | 0]
            const double Y = mfma4(G2, T1, 0.0);                    // rows 0, 1: S~ = B'P'A
            const double Z = mfma4(G2, T2, CZ);                     // rows 0, 1: [R~ | r~]
            const double Q = mfma4(Am, T1, CH);                     // Hx + A'P'A
            const double Qt = mfma4(T1, Am, CH);                    // its transpose (below)
            const double pp = cc == 2 ? T2 : 0.0;                   // p + P'b (column 2)
            const double qv = mfma4(Am, pp, gq);                    // q~ = gx + A'pp (column 2; the others +0)
            // R~ on the lanes of rows 0 and 1: v_permlane16_swap puts row 0 of Z into rows 0, 1 of its
            // first result and row 1 into rows 0, 1 of the second; quad broadcasts pick columns
            const auto slo = __builtin_amdgcn_permlane16_swap(__double2loint(Z), __double2loint(Z), false, false);
            const auto shi = __builtin_amdgcn_permlane16_swap(__double2hiint(Z), __double2hiint(Z), false, false);
            const double w0 = __hiloint2double(shi[0], slo[0]), w1 = __hiloint2double(shi[1], slo[1]);
            const double R00 = quad_bcast<0x00>(w0), R01 = quad_bcast<0x55>(w0), R11 = quad_bcast<0x55>(w1);
            // K = -R~^-1 S~ = (Xa'S~) / det with Xa = -adj R~: the product does not wait for the reciprocal
            const double det = qfma(R00, R11, -(R01 * R01));
            const double Xa = (r < 2 && cc < 2) ? (r != cc ? R01 : (r == 0 ? -R11 : -R00)) : 0.0;
            const double Ka = mfma4(Xa, Y, 0.0);
            const double idet = rcp(det);
            const double Kf = Ka * (r < 2 ? idet : 0.0);            // rows 0, 1: K; rows 2, 3: 0
            // (rows 2, 3 hold no R~: their idet is not finite, and Kf's zero rows enter P and p)
            // stage k's K and [R~ | r~] over the record's first slots (its operands are already read)
            if constexpr (S == 1) {
                wk[(k - kb) * MFW_REC] = Kf;
                wz[(k - kb) * MFW_REC] = Z;
            } else {
                double* rk = reg + bg * IS + (k - kb) * MFW_REC;
                if (b < G && r < 2) {
                    rk[O_K + 4 * r + cc] = Kf;
                    rk[O_Z + 4 * r + cc] = Z;
                }
            }
            if (k > 0) {   // P_k, p_k (nothing reads P_0, p_0)
                // P keeps its upper triangle and takes the lower one from the transposed products
                // (K'S~ + Q~', Q~' = T1'A + Hx: the same products in the same order, so bit for bit the
                // transpose): a symmetric P as the lane walk's.  Left to drift apart, the two triangles
                // cost the ill-conditioned QPs up to 1e3x the walk's error (tests/test_gpu_parity.py).
                const double RT = r < 2 && cc == 2 ? Z : 0.0;       // r~ (column 2)
                const double Pu = mfma4(Y, Kf, Q);                  // Q~ + S~'K
                const double Pl = mfma4(Kf, Y, Qt);                 // its transpose
                P = r <= cc ? Pu : Pl;
                pv = mfma4(Kf, RT, qv);                             // q~ + K'r~ (column 2; the others +0)
            }
        };
        // two operand sets, each read one step ahead, so the prefetch never waits on the step it feeds.
        // A lane reads each operand element through its own pointer: a record slot, stepping one record
        // down per step, or a constant slot, standing still (stride 0) -- no per-step selects
        const double* r0 = rb + (kf - kb) * MFW_REC;
        const double *pa = ao >= 0 ? r0 + ao : cst + ac, *pg = go >= 0 ? r0 + go : cst + C_ZERO;
        const double *ph_ = ho >= 0 ? r0 + ho : cst + hc, *pz = zo >= 0 ? r0 + zo : cst + C_ZERO;
        const double* pq = qo >= 0 ? r0 + qo : cst + C_ZERO;
        const int sa = ao >= 0 ? MFW_REC : 0, sg = go >= 0 ? MFW_REC : 0, sh = ho >= 0 ? MFW_REC : 0;
        const int sz = zo >= 0 ? MFW_REC : 0, sq = qo >= 0 ? MFW_REC : 0;
        double aA = *pa, gA = *pg, hA = *ph_, zA = *pz, qA = *pq, aB = 0.0, gB = 0.0, hB = 0.0, zB = 0.0, qB = 0.0;
        pa -= sa; pg -= sg; ph_ -= sh; pz -= sz; pq -= sq;
        // (the reads one record past the phase's last stage land inside the workgroup's LDS and go unused)
        for (int k = kf;; k -= 2) {
            aB = *pa; gB = *pg; hB = *ph_; zB = *pz; qB = *pq;
            pa -= sa; pg -= sg; ph_ -= sh; pz -= sz; pq -= sq;
            step(k, aA, gA, hA, zA, qA);
            if (k == kb) break;
            aA = *pa; gA = *pg; hA = *ph_; zA = *pz; qA = *pq;
            pa -= sa; pg -= sg; ph_ -= sh; pz -= sz; pq -= sq;
            step(k - 1, aB, gB, hB, zB, qB);
            if (k - 1 == kb) break;
        }
        wave_lds_sync();
        // collect: the stage lanes take their slots' factors (stages k < N)
        if constexpr (S == 1) {
            if (NC ? (ph == 0 ? lanes_of<lane_mask_mfw_collect(NC, 0)>() : lanes_of<lane_mask_mfw_collect(NC, 1)>())
                   : QSP_SOME_LANE(c.grp < G && c.lig >= kb && c.lig <= ke && c.lig < N)) {
                const double* rr = reg + c.grp * IS + (c.lig - kb) * MFW_REC;
#pragma unroll
                for (int q = 0; q < 8; ++q) st.K[0][q] = rr[O_K + q];
                // Rn = -R~^-1 and kk = -R~^-1 r~ from the R~ the walk inverted (the same operations)
                const double* rz = rr + O_Z;
                const double R00 = rz[0], R01 = rz[1], rt0 = rz[2], R11 = rz[5], rt1 = rz[6];
                const double idet = rcp(qfma(R00, R11, -(R01 * R01)));
                st.Rn[0][0] = (-R11) * idet;
                st.Rn[0][1] = R01 * idet;
                st.Rn[0][2] = (-R00) * idet;
                st.kk[0][0] = qfma(st.Rn[0][1], rt1, st.Rn[0][0] * rt0);
                st.kk[0][1] = qfma(st.Rn[0][2], rt1, st.Rn[0][1] * rt0);
            }
        } else {
    #pragma unroll
            for (int ls = 0; ls < S; ++ls) {
                const int k = kof<S>(c, ls);
                if (QSP_SOME_LANE(c.grp < G && k >= kb && k <= ke && k < N)) {
                    const double* rr = reg + c.grp * IS + (k - kb) * MFW_REC;
    #pragma unroll
                    for (int q = 0; q < 8; ++q) st.K[ls][q] = rr[O_K + q];
                    // Rn = -R~^-1 and kk = -R~^-1 r~ from the R~ the walk inverted (the same operations)
                    const double* rz = rr + O_Z;
                    const double R00 = rz[0], R01 = rz[1], rt0 = rz[2], R11 = rz[5], rt1 = rz[6];
                    const double idet = rcp(qfma(R00, R11, -(R01 * R01)));
                    st.Rn[ls][0] = (-R11) * idet;
                    st.Rn[ls][1] = R01 * idet;
                    st.Rn[ls][2] = (-R00) * idet;
                    st.kk[ls][0] = qfma(st.Rn[ls][1], rt1, st.Rn[ls][0] * rt0);
                    st.kk[ls][1] = qfma(st.Rn[ls][2], rt1, st.Rn[ls][1] * rt0);
                }
            }
        }
        wave_lds_sync();   // the next phase's records overwrite these
    }
    // the overlaid fields read later: the terminal and padding slots' F_VA / F_VN stay zero (the
    // forward passes write them on the stages k < N only; qp_ipm's start defines them)
    // (one stage per lane: written as the lane test, which keeps the kernel within two waves per SIMD
    // (249 registers); the unrolled slot loop, the same test, costs it the second wave)
    if constexpr (S == 1) {
        if (NC ? !lanes_of<lane_mask_stage(NC, 1)>() : c.lig >= N) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                st.f(F_VA, 0, q) = 0.0;
                st.f(F_VN, 0, q) = 0.0;
            }
        }
    } else {
#pragma unroll
        for (int ls = 0; ls < S; ++ls) {
            if (kof<S>(c, ls) >= N) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    st.f(F_VA, ls, q) = 0.0;
                    st.f(F_VN, ls, q) = 0.0;
                }
            }
        }
    }
}

// ------------------------------------------------ S = 2: the affine passes as scans
// With two stages per lane (N + 1 > 32: configs[4]) the kernel runs one wave per SIMD, where a
// serial lane walk is latency-bound.  The forward passes and the corrector's difference pass are
// affine recursions, so they run as Hillis-Steele scans over the group's lanes instead
// (scripts/ubench/fwd_scan_s2.hip: 0.50x the walk's time at that occupancy).  Partner maps move by
// ds_bpermute; every composition is a fixed FMA order (Aff, aff_*: qsp_riccati.hpp).

__device__ __forceinline__ double lane_read(double v, int src) {
    const int lo = __shfl(__double2loint(v), src), hi = __shfl(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void aff_read(const Aff& e, int src, Aff& f) {
#pragma unroll
    for (int q = 0; q < 16; ++q) f.F[q] = lane_read(e.F[q], src);
#pragma unroll
    for (int q = 0; q < 4; ++q) f.c[q] = lane_read(e.c[q], src);
}

// S = 2, the factorisation as an associative scan: a partner's element (VElem, velem_*: qsp_riccati.hpp)
__device__ __forceinline__ void velem_read(const VElem& e, int src, VElem& f) {
    const double* s = &e.A[0];
    double* d = &f.A[0];
#pragma unroll
    for (int q = 0; q < VELEM_N; ++q) d[q] = lane_read(s[q], src);
}

// ------------------------------------------------------------------ QP core
// (the slots' barrier terms, directions and step: qsp_ipm.hpp, with Stage<S> as the view)
// Backward pass over the group (factorisation, or the corrector's difference recursion),
// then forward pass writing the bounded components of the solution into LDS field `out`
// (F_VA / F_VN).
// NC: the horizon where it is compiled in (ctx_of).  The closed-loop lane walks (S = 1) then have constant
// trip counts and run QSP_WALK_UNROLL steps per loop iteration: a rolled step pays two branches and the
// loop counter beside its 16 FMA and 8 DPP moves.  Measured at N = 20 (profiles/fixed_horizon/README.md):
// 2 +1.2 %, 4 +2.0 % over the rolled walks, both at the rolled kernel's 253 VGPRs; 5 (+2.2 %) and the full
// unroll (+1.9 %) take 256 VGPRs, 10 takes 264 (one wave per SIMD).  NC = 0 keeps the rolled loops (count 1).
// With the steps' exec masks as constants the masks no longer spilled and the counts were measured again
// (profiles/lane_masks/README.md): 4 and 5 at 245 VGPRs, written out in full (every step's mask a literal) at
// 246 and the fastest, +0.2 % over 4.  32 covers every horizon at one stage per lane (L - 1 <= 31 steps).
// Each walk now runs under one exec mask for all its steps (below; profiles/walk_regions/README.md), written out
// in full as before.
#ifndef QSP_WALK_UNROLL
#define QSP_WALK_UNROLL 32
#endif
template <int S, bool FACTOR, bool ALT = false, int NC = 0>
__device__ __forceinline__ void riccati_solve(const Ctx& c, const SolveParams& p, Stage<S>& st, const double dx0[4],
                                              int out, double (&M)[S][16], const double (&hgv)[S][6]) {
    SEG_T(t_rs);
    double P[10], pv[4];
#pragma unroll
    for (int i = 0; i < 10; ++i) P[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) pv[i] = 0.0;
    // Branch-free walk: every lane evaluates the step on its own slot data; only the
    // lane whose turn it is (lig == j) keeps its factors, and only its chain value is
    // consumed by the neighbour after the hand-over.  The terminal stage k = N sits in
    // slot N % S of the last lane; the walk starts there.
    const int lsN = c.N - (c.L - 1) * S;
    if (FACTOR) {
#pragma unroll
        for (int ls = 0; ls < S; ++ls)
            if (ls == lsN) ric_terminal(p, st.g[ls], P, pv);
    }   // corrector difference: dp_N = 0
    // the barrier-modified diagonal and gradient entries are fixed during the walk: formed
    // once per slot instead of at every step
    double hx3[S], hu[S][2], gx3[S], gu[S][2];
#pragma unroll
    for (int ls = 0; ls < S; ++ls) {
        if (FACTOR) {
            hx3[ls] = qfma(p.tau, p.W[3], hgv[ls][0]);
            hu[ls][0] = qfma(p.tau, p.W[4], hgv[ls][1]);
            hu[ls][1] = qfma(p.tau, p.W[5], hgv[ls][2]);
            gx3[ls] = st.g[ls][3] + hgv[ls][3];
            gu[ls][0] = st.g[ls][4] + hgv[ls][4];
            gu[ls][1] = st.g[ls][5] + hgv[ls][5];
        } else {
            gx3[ls] = st.hg(ls, 3);
            gu[ls][0] = st.hg(ls, 4);
            gu[ls][1] = st.hg(ls, 5);
        }
    }
    if constexpr (S == 1 && !FACTOR) {
        // corrector difference walk in closed-loop form: dp_k = e_k + (A + B K)' dp_{k+1} with
        // e = dg_x + K' dg_u (ric_delta_step with dr = dg_u + B' dp substituted), a 4x4 map per
        // step; each lane keeps the dp that reaches it and forms dkk = Rn (dg_u + B' dp)
        // afterwards, in parallel
        const double* K = st.K[0];
        double e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e[i] = qfma(K[4 + i], gu[0][1], qfma(K[i], gu[0][0], i == 3 ? gx3[0] : 0.0));
        // The walk is a pipeline under one exec mask, lig <= L - 2, for all of its L - 2 steps: every enabled lane
        // forms n = e + M' pv from its own loop-invariant M, e and its current pv, and takes its next lane's n.
        // - The terminal lanes (lig == L - 1) are disabled throughout, as sources and as destinations, so
        //   nothing crosses an instance boundary (a padding lane at the wave's end has no source at all).
        // - The first lane of the chain, lig == L - 2, is thereby pinned: a DPP read from a disabled or missing
        //   lane leaves `old`, so it holds dp_N = 0 at every step and hands the same dp_{N-1} on each time.
        // - So the pipeline is idempotent: by induction the lanes lig >= L - 2 - t hold the dp that reaches them
        //   after step t, and every later step hands them the same bits again (the same operations on the same
        //   inputs).  After L - 2 steps lane 0 holds dp_1; dp_0 is read by nothing.
        // - Nothing may read pv before the last step: the lanes the wavefront has not reached hold throw-away
        //   values, possibly non-finite, which later steps overwrite.
        // (Per-step masks lig <= j, under which the finished lanes sat out, gave every lane the same bits at six
        // scalar instructions per step to rebuild the mask: profiles/walk_regions/README.md.)
        {
            auto step = [&]() {
                double n[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    n[i] = qfma(M[0][12 + i], pv[3], qfma(M[0][8 + i], pv[2], qfma(M[0][4 + i], pv[1], qfma(M[0][i], pv[0], e[i]))));
#pragma unroll
                for (int i = 0; i < 4; ++i) pv[i] = wave_from_next(pv[i], n[i]);
            };
            // dkk behind the walk, after its last step, in the walk's region: at one stage per lane the stage role
            // lig < N is the walk's mask (measured against a region of its own: profiles/walk_regions/README.md)
            auto update = [&]() {
                const double* dpk = pv;
                const double* B = st.B[0];
                const double* Rn = st.Rn[0];
                double rt[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    rt[i] = qfma(B[6 + i], dpk[3], qfma(B[4 + i], dpk[2], qfma(B[2 + i], dpk[1], qfma(B[i], dpk[0], gu[0][i]))));
                st.kk[0][0] = qfma(Rn[1], rt[1], qfma(Rn[0], rt[0], st.kk[0][0]));
                st.kk[0][1] = qfma(Rn[2], rt[1], qfma(Rn[1], rt[0], st.kk[0][1]));
            };
            if constexpr (NC > 0) {
                constexpr int L = lanes_per_instance(NC, 1);
                static_assert(lane_mask_stage(NC, 1) == lane_mask_lig_le(NC, 1, L - 2), "lig < N is the walk's mask");
                if (QSP_SOME_LANE(lanes_of<lane_mask_lig_le(NC, 1, L - 2)>())) {
#pragma clang loop unroll_count(QSP_WALK_UNROLL)
                    for (int j = L - 2; j >= 1; --j) step();
                    update();
                }
            } else if (QSP_SOME_LANE(c.lig <= c.L - 2)) {
#pragma clang loop unroll_count(1)
                for (int j = c.L - 2; j >= 1; --j) step();
                update();
            }
        }
    } else if constexpr (S == 2 && !FACTOR) {
        // corrector difference pass as a suffix scan of the lanes' backward maps, dp_N = 0: lane j's
        // map is slot 1's then slot 0's (identity past the horizon); U_j = D_j o D_{j+1} o ...
        const int k0 = 2 * c.lig;
        Aff d;
        {
            Aff m1;
            aff_delta(st.a[0], st.B[0], st.K[0], gx3[0], gu[0], d);
            aff_delta(st.a[1], st.B[1], st.K[1], gx3[1], gu[1], m1);
            if (k0 + 1 < c.N) aff_compose(d, m1);
            else if (!(k0 < c.N)) aff_identity(d);
        }
        for (int off = 1; off < c.L; off <<= 1) {
            const bool take = c.lig + off < c.L;
            Aff f;
            aff_read(d, take ? c.lane + off : c.lane, f);
            if (QSP_SOME_LANE(take)) aff_compose(d, f);
        }
        // dp_{2j+2}: the next lane's suffix map applied to dp_N = 0 (its constant); then each slot's
        // dkk from the dp reaching it, slot 1 first (ric_delta_step also steps dp to the slot)
        double pvs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double nx = wave_from_next(d.c[i]);
            pvs[i] = (c.lig + 1 < c.L) ? nx : 0.0;
        }
#pragma unroll
        for (int ls = 1; ls >= 0; --ls) {
            if (kof<S>(c, ls) < c.N) {
                double dkk[2];
                ric_delta_step(st.a[ls], st.B[ls], gx3[ls], gu[ls], st.K[ls], st.Rn[ls], pvs, dkk);
                st.kk[ls][0] += dkk[0];
                st.kk[ls][1] += dkk[1];
            }
        }
    } else if constexpr (S == 2 && FACTOR && ALT) {
        // factorisation as a suffix scan of the lanes' value-function elements: lane j combines its
        // two stages' elements (slot 0's, then slot 1's; the terminal element where k = N, none past
        // it), Hillis-Steele levels give E_{2j:N}, the next lane's result E_{2j+2:N} gives slot 1's
        // E_{2j+1:N}; then each slot forms K, Rn, kk from its successor's value function
        const int k0 = 2 * c.lig, k1 = k0 + 1;
        VElem e, e1;
        {
            const double Hx0[4] = {p.tau * p.W[0], p.tau * p.W[1], p.tau * p.W[2], hx3[0]};
            const double gxa[4] = {st.g[0][0], st.g[0][1], st.g[0][2], gx3[0]};
            if (k0 < c.N) velem_stage(st.a[0], st.B[0], st.bb[0], Hx0, hu[0], gxa, gu[0], e);
            else velem_terminal(p.We, st.g[0], e);
            const double Hx1[4] = {p.tau * p.W[0], p.tau * p.W[1], p.tau * p.W[2], hx3[1]};
            const double gxb[4] = {st.g[1][0], st.g[1][1], st.g[1][2], gx3[1]};
            if (k1 < c.N) velem_stage(st.a[1], st.B[1], st.bb[1], Hx1, hu[1], gxb, gu[1], e1);
            else velem_terminal(p.We, st.g[1], e1);
            if (k1 <= c.N) {
                VElem t = e1;
                velem_combine(e, t);
            }
        }
        for (int off = 1; off < c.L; off <<= 1) {
            const bool take = c.lig + off < c.L;
            VElem f;
            velem_read(e, take ? c.lane + off : c.lane, f);
            if (QSP_SOME_LANE(take)) velem_combine(e, f);
        }
        {
            VElem f;
            velem_read(e, c.lig + 1 < c.L ? c.lane + 1 : c.lane, f);
            if (k1 < c.N) {
                velem_combine(e1, f);
                double Pn[10], pn[4];
#pragma unroll
                for (int q = 0; q < 10; ++q) Pn[q] = f.J[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) pn[q] = -f.eta[q];
                const double gx[4] = {st.g[1][0], st.g[1][1], st.g[1][2], gx3[1]};
                const double Hx[4] = {p.tau * p.W[0], p.tau * p.W[1], p.tau * p.W[2], hx3[1]};
                ric_factor_step(st.a[1], st.B[1], st.bb[1], Hx, hu[1], gx, gu[1], Pn, pn, st.K[1], st.Rn[1], st.kk[1], false);
            }
            if (k0 < c.N) {
                double Pn[10], pn[4];
#pragma unroll
                for (int q = 0; q < 10; ++q) Pn[q] = e1.J[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) pn[q] = -e1.eta[q];
                const double gx[4] = {st.g[0][0], st.g[0][1], st.g[0][2], gx3[0]};
                const double Hx[4] = {p.tau * p.W[0], p.tau * p.W[1], p.tau * p.W[2], hx3[0]};
                ric_factor_step(st.a[0], st.B[0], st.bb[0], Hx, hu[0], gx, gu[0], Pn, pn, st.K[0], st.Rn[0], st.kk[0], false);
            }
        }
    } else if constexpr (S == 1 && FACTOR && ALT) {
        factor_walk_mfma<1, NC>(c, p, st, hx3, hu, gx3, gu);
    } else {   // the factorisation (both difference passes are taken above): matrix cores or lane walk
    static_assert(FACTOR, "the corrector's difference pass is a closed-loop walk (S = 1) or a scan (S = 2)");
    bool walked = false;
    if constexpr (S == 2 && FACTOR) {
        if (mfw_use(p, 2)) {   // uniform (two stages per lane: ALT is the factorisation scan)
            factor_walk_mfma<2>(c, p, st, hx3, hu, gx3, gu);
            walked = true;
        }
    }
    if (!walked)
    for (int j = c.L - 1; j >= 0; --j) {
        // Lanes above j already hold their final factors and sit the step out (exec
        // mask); lanes below j compute a throw-away step that their own turn overwrites.
        // Writing the factors in place this way needs no per-step selects.
        // The hand-over runs inside the same region: lane j-1 (active) reads lane j (active).
        if (QSP_SOME_LANE(c.lig <= j)) {
            double Pc[10], pvc[4];
#pragma unroll
            for (int i = 0; i < 10; ++i) Pc[i] = P[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) pvc[i] = pv[i];
#pragma unroll
            for (int ls = S - 1; ls >= 0; --ls) {
                if (j == c.L - 1 && ls >= lsN) continue;     // terminal / padding slots of the last lane
                const double gx[4] = {st.g[ls][0], st.g[ls][1], st.g[ls][2], gx3[ls]};
                const double Hx[4] = {p.tau * p.W[0], p.tau * p.W[1], p.tau * p.W[2], hx3[ls]};
                ric_factor_step(st.a[ls], st.B[ls], st.bb[ls], Hx, hu[ls], gx, gu[ls], Pc, pvc, st.K[ls],
                                st.Rn[ls], st.kk[ls], j > 0 || ls > 0);
            }
            // hand-over to lane j-1 (none after step 0: lane 0 reads a disabled lane there).  The
            // first step of a last lane without a stage (lsN == 0) leaves P at the terminal
            // diag(We) every lane already holds, so only p moves then.
            if (j > 0) {
                if (!(j == c.L - 1 && lsN == 0)) {
#pragma unroll
                    for (int i = 0; i < 10; ++i) P[i] = wave_from_next(P[i], Pc[i]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) pv[i] = wave_from_next(pv[i], pvc[i]);
            }
        }
    }
    }
    SEG_NEXT(FACTOR ? 2 : 6, t_rs);
    if constexpr (S == 1) {
        // forward in closed-loop form: dx_{k+1} = (A + B K) dx_k + (B kk + b), so a step is
        // one 4x4 affine map (16 FMA) instead of du = kk + K dx followed by the dynamics;
        // each lane keeps the dx of its own stage and forms du = kk + K dx afterwards, in
        // parallel.  A + B K is built once per factorisation (the corrector reuses it).
        if (FACTOR) {
            const double* a = st.a[0];
            const double* B = st.B[0];
            const double* K = st.K[0];
            const double Am[4][4] = {{1.0, 0.0, a[0], a[1]}, {0.0, 1.0, a[2], a[3]}, {0.0, 0.0, 1.0, a[4]},
                                     {0.0, 0.0, 0.0, a[5]}};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) M[0][4 * i + q] = qfma(B[2 * i + 1], K[4 + q], qfma(B[2 * i], K[q], Am[i][q]));
        }
        double cv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cv[i] = qfma(st.B[0][2 * i + 1], st.kk[0][1], qfma(st.B[0][2 * i], st.kk[0][0], st.bb[0][i]));
        double dx[4] = {dx0[0], dx0[1], dx0[2], dx0[3]};
        // The same pipeline as the difference walk, forwards, under the one exec mask 0 <= lig <= L - 2 for all
        // of its L - 2 steps: every enabled lane forms n = M dx + cv and takes its previous lane's n.
        // - The terminal lanes (lig == L - 1) are disabled throughout, as sources and as destinations.
        // - The first lane, lig == 0, is thereby pinned at dx0: its source is the previous instance's terminal
        //   lane, disabled, or missing (lane 0 of the wave), and such a DPP read leaves `old`.
        // - So the pipeline is idempotent: the lanes lig <= t hold the dx of their stage after step t, and every
        //   later step hands them the same bits again.  After L - 2 steps lane L - 2 holds dx_{N-1}, the last
        //   one read (a step L - 1 would move nothing: its only lane's source would be finished and disabled).
        // - Nothing may read dx before the last step: the lanes ahead of the wavefront hold throw-away values,
        //   possibly non-finite, which later steps overwrite.
        {
            auto step = [&]() {
                double n[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    n[i] = qfma(M[0][4 * i + 3], dx[3], qfma(M[0][4 * i + 2], dx[2], qfma(M[0][4 * i + 1], dx[1], qfma(M[0][4 * i], dx[0], cv[i]))));
#pragma unroll
                for (int i = 0; i < 4; ++i) dx[i] = wave_from_prev(dx[i], n[i]);
            };
            // du = kk + K dx and the out stores behind the walk, after its last step, in the walk's region (the
            // stage role lig < N is the walk's mask, as at the difference walk)
            auto store = [&]() {
                const double* dxk = dx;
                const double* K = st.K[0];
                st.f(out, 0, 0) = dxk[3];
                st.f(out, 0, 1) = qfma(K[3], dxk[3], qfma(K[2], dxk[2], qfma(K[1], dxk[1], qfma(K[0], dxk[0], st.kk[0][0]))));
                st.f(out, 0, 2) = qfma(K[7], dxk[3], qfma(K[6], dxk[2], qfma(K[5], dxk[1], qfma(K[4], dxk[0], st.kk[0][1]))));
            };
            if constexpr (NC > 0) {
                constexpr int L = lanes_per_instance(NC, 1);
                static_assert(lane_mask_stage(NC, 1) == lane_mask_walk_fwd(NC, 1, 0), "lig < N is the walk's mask");
                if (QSP_SOME_LANE(lanes_of<lane_mask_walk_fwd(NC, 1, 0)>())) {
#pragma clang loop unroll_count(QSP_WALK_UNROLL)
                    for (int j = 0; j < L - 2; ++j) step();
                    store();
                }
            } else if (QSP_SOME_LANE(c.lig <= c.L - 2)) {
#pragma clang loop unroll_count(1)
                for (int j = 0; j < c.L - 2; ++j) step();
                store();
            }
        }
        SEG_ADD(FACTOR ? 3 : 7, t_rs);
        return;
    }
    if constexpr (S == 2) {
        // forward pass as a prefix scan of the lanes' closed-loop maps (slot 0's, then slot 1's):
        // T_j = E_j o T_{j-1}; the state entering lane j is T_{j-1}(dx0) (dx0 at lane 0), then
        // slot 0 forms du = kk + K dx and steps the dynamics, slot 1 forms its du
        Aff e;
        {
            Aff m1;
            aff_forward(st.a[0], st.B[0], st.bb[0], st.K[0], st.kk[0], e);
            aff_forward(st.a[1], st.B[1], st.bb[1], st.K[1], st.kk[1], m1);
            aff_compose(m1, e);
            e = m1;
        }
        for (int off = 1; off < c.L; off <<= 1) {
            const bool take = c.lig >= off;
            Aff f;
            aff_read(e, take ? c.lane - off : c.lane, f);
            if (QSP_SOME_LANE(take)) aff_compose(e, f);
        }
        double dx[4];
        {
            double y[4];
            aff_apply(e, dx0, y);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double pr = wave_from_prev(y[i]);
                dx[i] = c.lig == 0 ? dx0[i] : pr;
            }
        }
#pragma unroll
        for (int ls = 0; ls < 2; ++ls) {
            double du[2];
            du[0] = qfma(st.K[ls][3], dx[3], qfma(st.K[ls][2], dx[2], qfma(st.K[ls][1], dx[1], qfma(st.K[ls][0], dx[0], st.kk[ls][0]))));
            du[1] = qfma(st.K[ls][7], dx[3], qfma(st.K[ls][6], dx[2], qfma(st.K[ls][5], dx[1], qfma(st.K[ls][4], dx[0], st.kk[ls][1]))));
            if (kof<S>(c, ls) < c.N) {
                st.f(out, ls, 0) = dx[3];
                st.f(out, ls, 1) = du[0];
                st.f(out, ls, 2) = du[1];
            }
            if (ls == 0) dyn_step(st.a[0], st.B[0], st.bb[0], du, dx);
        }
        return;
    }
}

// Mehrotra predictor-corrector IPM on the current linearisation.  Leaves the
// damped control step in LDS (F_DU) and the slacks/multipliers in F_T / F_LM.
// Returns the number of iterations taken by this lane's instance and, in `exit`, why it stopped
// (group-uniform): QP_EXIT_CONV the stop test was met; QP_EXIT_CAP the iteration cap (its last
// iterate is used, as HPIPM's at iter_max); QP_EXIT_STALL the step length stayed below
// qp_stall_alpha for qp_stall_iters iterations (locally infeasible linearisation, HPIPM's
// min-step exit; the last iterate is used as at the cap); QP_EXIT_DIVERGED mu left
// [0, qp_mu_max) (multipliers growing without bound, or non-finite): a QP failure (acados
// ACADOS_QP_FAILURE, status 4), stopped while its iterate is still finite.  A stopped instance's
// state is frozen while the rest of its wave iterates (no update with alpha = 0, which would turn
// an infinite direction into NaN).
//
// Stop test (HPIPM's four exit residuals, ocp_qp_ipm): complementarity mu < mu_stop, bound
// residual < res_stop, stationarity < qp_tol_stat, equality < qp_tol_eq.  The three linear
// residuals are those of the IPM iterate (z, pi, lam, t) with start z = 0, pi = 0, lam =
// mu0 / t: every Newton step solves them exactly and the update scales all of them by
// (1 - alpha), so each is its start value times prod(1 - alpha) (tracked, not recomputed:
// r0 = bound residual of the floored slacks, rg0 = max|g + C' lam|, rb0 = max(|dx0|, |b|)); the
// test r * prod < tol is applied as prod < min(tol / r) over the three.
template <int S, bool ALT = false, int NC = 0>
__device__ int qp_ipm(const Ctx& c, const SolveParams& p, Stage<S>& st, const double dx0[4], int& exit,
                      bool skip = false) {
    SEG_T(t_ipm);
    const double m = 2.0 * (3.0 * c.N - (p.s0_bound ? 0.0 : 1.0));
    // initial point.  r0 = largest bound residual of the infeasible start (t - d where the
    // slack had to be floored at t_min); every update scales all residuals by (1 - alpha)
    double r0 = 0.0, rg0 = 0.0, rb0 = 0.0;
#pragma unroll
    for (int ls = 0; ls < S; ++ls) {
        const int k = kof<S>(c, ls);
        double lo[3], hi[3];
        bnd_lohi(p, st, ls, lo, hi);
        double gl[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const bool act = bnd_act(p, c.N, k, j);
            const double tl = fmax(-lo[j], p.t_min), th = fmax(hi[j], p.t_min);
            if (act) r0 = fmax(r0, fmax(tl + lo[j], th - hi[j]));
            const double rl = rcp(tl), rh = rcp(th);
            st.t(ls, 2 * j) = act ? tl : 1.0;
            st.t(ls, 2 * j + 1) = act ? th : 1.0;
            st.rt(ls, 2 * j) = act ? rl : 1.0;
            st.rt(ls, 2 * j + 1) = act ? rh : 1.0;
            st.lm(ls, 2 * j) = act ? p.mu0 * rl : 0.0;
            st.lm(ls, 2 * j + 1) = act ? p.mu0 * rh : 0.0;
            gl[j] = act ? qfma(p.mu0, rh, -(p.mu0 * rl)) : 0.0;
        }
        // start-point stationarity g + C' lam (bounded components s, u_n, u_t) and equality
        // (defects; x0 on the first stage); the padding slots past the terminal stage hold zeros
        if (k <= c.N) {
            rg0 = fmax(rg0, fmax(fmax(fabs(st.g[ls][0]), fabs(st.g[ls][1])), fmax(fabs(st.g[ls][2]), fabs(st.g[ls][3] + gl[0]))));
            rg0 = fmax(rg0, fmax(fabs(st.g[ls][4] + gl[1]), fabs(st.g[ls][5] + gl[2])));
            rb0 = fmax(rb0, fmax(fmax(fabs(st.bb[ls][0]), fabs(st.bb[ls][1])), fmax(fabs(st.bb[ls][2]), fabs(st.bb[ls][3]))));
            if (k == 0) rb0 = fmax(rb0, fmax(fmax(fabs(dx0[0]), fabs(dx0[1])), fmax(fabs(dx0[2]), fabs(dx0[3]))));
        }
        st.du(ls, 0) = 0.0;
        st.du(ls, 1) = 0.0;
        // the forward walks never write the terminal / padding slots: define them, so no
        // stale LDS content (another block's data, possibly NaN bit patterns) is ever read
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            st.f(F_VA, ls, q) = 0.0;
            st.f(F_VN, ls, q) = 0.0;
        }
    }
    // the three linear residuals share the scale prod(1 - alpha): one threshold on it
    // (x / 0 = inf: a residual that starts at zero never binds)
    double rs_stop = p.res_stop / group_max(r0, c.gs);
    const double rs_g = p.qp_tol_stat / group_max(rg0, c.gs), rs_b = p.qp_tol_eq / group_max(rb0, c.gs);
    // a NaN start residual compares false here and leaves rs_stop as it was (the fmax accumulation
    // above drops NaN anyway); a NaN QP is caught by the divergence exit (NaN mu) or the non-finite
    // solution check after the loop, not by this threshold
    rs_stop = rs_g < rs_stop ? rs_g : rs_stop;
    rs_stop = rs_b < rs_stop ? rs_b : rs_stop;
    double rscale = 1.0;
    int nit = 0, stall = 0;
    bool conv = false, stalled = false, div = false;
    SEG_ADD(13, t_ipm);
    for (int it = 0;; ++it) {
        SEG_T(t_seg);
        double tl_sum = 0.0;
#pragma unroll
        for (int ls = 0; ls < S; ++ls)
#pragma unroll
            for (int q = 0; q < 6; ++q) tl_sum = qfma(st.t(ls, q), st.lm(ls, q), tl_sum);
        // The predictor's barrier terms go under the sum's shuffle levels: they do not depend on
        // mu, and the break below stands between the sum and their place in front of the
        // factorisation.  The pass in front of the break that ends the loop is computed for
        // nothing (registers only); a finished instance recomputes the terms of its frozen state.
        double hgv[S][6];
        const double mu = group_sum_over<3 * S>(tl_sum, c.gs, [&](int q) { barrier_term(p, c.N, st, q / 3, kof<S>(c, q / 3), q % 3, hgv[q / 3]); }) / m;
        ipm_exit_test(p, mu, rscale, rs_stop, stall, skip, div, conv, stalled);
        const bool done = conv || div || stalled;
        // the cap is tested after the last step too (conv reports it), then the loop ends
        if (it == p.qp_iters || __ballot(!done) == 0ull) break;
        nit += done ? 0 : 1;
#ifdef QSP_SEGSTAMP
        if ((threadIdx.x & 63) == 0) atomicAdd(&g_seg[31], 1ull);
#endif
        SEG_NEXT(0, t_seg);   // with the predictor's barrier terms (segment 1, theirs alone, is gone)
        // ---- predictor
        double M[S][16];   // closed-loop matrices A + B K (S = 1), shared by both forward walks
        riccati_solve<S, true, ALT, NC>(c, p, st, dx0, F_VA, M, hgv);
        SEG_T(t_seg2);
        // affine directions: computed once, kept in registers through the corrector
        double at[S][6], al[S][6];
        double num = 1.0, den = 1.0;
#pragma unroll
        for (int ls = 0; ls < S; ++ls) affine_dirs(p, c.N, st, ls, kof<S>(c, ls), at[ls], al[ls], num, den);
        const double aa = group_min(num / den, c.gs);
        double ma = 0.0;
#pragma unroll
        for (int ls = 0; ls < S; ++ls) ma = affine_mu_part(p, c.N, st, ls, kof<S>(c, ls), at[ls], al[ls], aa, ma);
        const double mua = group_sum_flat(ma, c.gs) / m;
        const double r = mua / mu;
        const double sg = fmax(r * r * r, p.sigma_min);
        const double smu = sg * mu;
        SEG_NEXT(4, t_seg2);
        // ---- corrector
#pragma unroll
        for (int ls = 0; ls < S; ++ls) corrector_terms(p, c.N, st, ls, kof<S>(c, ls), at[ls], al[ls], smu);
        SEG_ADD(5, t_seg2);
        riccati_solve<S, false, ALT, NC>(c, p, st, dx0, F_VN, M, hgv);
        SEG_T(t_seg3);
        double dt[S][6], dl[S][6];
        num = 1.0; den = p.frac;       // initial bound 1/frac
#pragma unroll
        for (int ls = 0; ls < S; ++ls) corrector_dirs(p, c.N, st, ls, kof<S>(c, ls), at[ls], al[ls], smu, dt[ls], dl[ls], num, den);
        double alpha = p.frac * group_min(num / den, c.gs);
        alpha = fmin(alpha, 1.0);
        // a finished instance sits the rest of the wave's loop out with its state frozen
        if (!done) {
            stall = alpha < p.qp_stall_alpha ? stall + 1 : 0;
            rscale *= 1.0 - alpha;
#pragma unroll
            for (int ls = 0; ls < S; ++ls) {
                apply_step(st, ls, dt[ls], dl[ls], alpha);
                damp_du(st, ls, alpha);
            }
        }
        SEG_ADD(8, t_seg3);
    }
    exit = ipm_exit_code(conv, div, stalled);
    return nit;
}

// State step of the damped QP solution (rollout of the affine dynamics), into LDS F_DX.
template <int S>
__device__ __forceinline__ void qp_rollout(const Ctx& c, Stage<S>& st, const double dx0[4]) {
    double dx[4] = {dx0[0], dx0[1], dx0[2], dx0[3]};
    for (int j = 0; j < c.L; ++j) {
        if (c.lig == j) {
#pragma unroll
            for (int ls = 0; ls < S; ++ls) {
                const int k = j * S + ls;
                if (k <= c.N) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) st.dxs(ls, i) = dx[i];
                }
                if (k < c.N) {
                    const double du[2] = {st.du(ls, 0), st.du(ls, 1)};
                    dyn_step(st.a[ls], st.B[ls], st.bb[ls], du, dx);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) dx[i] = wave_from_prev(dx[i]);
    }
}

// Dynamics multipliers by the adjoint recursion; writes PI (B x N x 4).
//   pi_{N-1} = We dx_N + g_N ; pi_{k-1} = Hx dx_k + gx_k + A_k' pi_k + (lam_hi - lam_lo)_s
template <int S>
__device__ __forceinline__ void qp_adjoint_store(const Ctx& c, const SolveParams& p, const Stage<S>& st,
                                                 double* PI, bool write, bool shift) {
    double pi[4] = {0, 0, 0, 0};
    for (int j = c.L - 1; j >= 0; --j) {
        if (c.lig == j) {
#pragma unroll
            for (int ls = S - 1; ls >= 0; --ls) {
                const int k = j * S + ls;
                if (k == c.N) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) pi[i] = qfma(p.We[i], st.dxs(ls, i), st.g[ls][i]);
                } else if (k < c.N) {
                    if (write && (!shift || k >= 1)) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) PI[(size_t)(shift ? k - 1 : k) * 4 + i] = pi[i];
                    }
                    if (write && shift && k == c.N - 1) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) PI[(size_t)k * 4 + i] = pi[i];
                    }
                    if (k >= 1) {
                        const double dxk[4] = {st.dxs(ls, 0), st.dxs(ls, 1), st.dxs(ls, 2), st.dxs(ls, 3)};
                        adjoint_step(p, st.a[ls], dxk, st.g[ls], st.lm(ls, 1) - st.lm(ls, 0), pi);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) pi[i] = wave_from_next(pi[i]);
    }
}

// The fixed-K SQP (nlp_mode 0) reads no multipliers between its iterations, so its QP kernels
// do not walk the adjoint recursion: every stage lane stores what the recursion takes from its
// own stage (the adjoint record, ADJ_REC doubles per stage 1..N, instance-major), every
// successful QP overwrites the record, and the epilogue walks the recursion once per solve from
// the record of the instance's last successful QP (adjoint_from_record).  The terms are those of
// adjoint_step in its order, so PI keeps its bits.
//   stage 1 <= k < N, at (k - 1) ADJ_REC: c_i = tau W_i dx_k,i + g_k,i (4), a_k (6), (lam_hi - lam_lo)_s
//   stage N, at (N - 1) ADJ_REC:          pi_{N-1} = We dx_N + g_N (4)

template <int S>
__device__ __forceinline__ void qp_adjoint_record(const Ctx& c, const SolveParams& p, const Stage<S>& st, double* rec) {
#pragma unroll
    for (int ls = 0; ls < S; ++ls) {
        const int k = kof<S>(c, ls);
        if (k < 1 || k > c.N) continue;
        double* r = rec + (size_t)(k - 1) * ADJ_REC;
        if (k == c.N) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = qfma(p.We[i], st.dxs(ls, i), st.g[ls][i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = qfma(p.tau * p.W[i], st.dxs(ls, i), st.g[ls][i]);
#pragma unroll
            for (int i = 0; i < 6; ++i) r[4 + i] = st.a[ls][i];
            r[10] = st.lm(ls, 1) - st.lm(ls, 0);
        }
    }
}

// PI (N x 4) of one instance from its adjoint record: qp_adjoint_store's recursion and its
// shifted / unshifted rows (shift: row k - 1 for k >= 1, the last row duplicated).
__device__ __forceinline__ void adjoint_from_record(int N, const double* rec, double* PI, bool shift) {
    double pi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pi[i] = rec[(size_t)(N - 1) * ADJ_REC + i];
    for (int k = N - 1; k >= 0; --k) {
        if (!shift || k >= 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) PI[(size_t)(shift ? k - 1 : k) * 4 + i] = pi[i];
        }
        if (shift && k == N - 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) PI[(size_t)k * 4 + i] = pi[i];
        }
        if (k >= 1) {
            const double* r = rec + (size_t)(k - 1) * ADJ_REC;
            double np[4];
            np[0] = r[0] + pi[0];
            np[1] = r[1] + pi[1];
            np[2] = r[2] + (qfma(r[6], pi[1], r[4] * pi[0]) + pi[2]);
            np[3] = r[3] + qfma(r[9], pi[3], qfma(r[8], pi[2], qfma(r[7], pi[1], r[5] * pi[0])));
            np[3] += r[10];
#pragma unroll
            for (int i = 0; i < 4; ++i) pi[i] = np[i];
        }
    }
}

// ------------------------------------------------------------------ kernels
// One solve = prologue, K x (linearize, qp), epilogue; all on one stream.
// Workspace (SolveArgs::w*): SQP iterate X/U, wrapped x0, stage data in SoA (LinField, qsp_kernels.h).

__device__ __forceinline__ const ShapeDev& shape_of(const SolveArgs& A, int i) {
    const int id = A.shape_id ? A.shape_id[i] : 0;
    return A.shapes[shape_clamp(id, A.n_shapes)];
}

// NLP multipliers and merit weights at the start of a solve (oracle sqp_solve: PI from the
// initial guess, LAM and the weights zero).
__device__ __forceinline__ void nlp_init(const SolveArgs& A, int i, bool use_pi) {
    const int N = A.p.N;
    const size_t tot = (size_t)A.B * (N + 1);
    for (int k = 0; k <= N; ++k) {
        const size_t si = (size_t)i * (N + 1) + k;
        for (int q = 0; q < 4; ++q)
            A.wnlp[(W_PI + q) * tot + si] = (use_pi && A.PI_in && k < N) ? A.PI_in[((size_t)i * N + k) * 4 + q] : 0.0;
        for (int q = W_LAM; q < W_COUNT; ++q) A.wnlp[q * tot + si] = 0.0;
    }
    A.wdone[i] = 0;
    if (A.wres)
        for (int q = 0; q < 4; ++q) A.wres[(size_t)i * 4 + q] = 0.0;
}

// An instance whose s_0 makes every QP infeasible (s0_infeasible, qsp_ipm.hpp) does not iterate
// (wdone = 3: status QSP_STATUS_QP_FAIL -- QSP_STATUS_NAN where s_0 or the rest of the iterate is not
// finite, epilogue_kernel --, sqp_iter 0, the initial guess returned), as the oracle's sqp_solve.
// (Called after nlp_init, which clears wdone.)
__device__ __forceinline__ void s0_feasible(const SolveArgs& A, int i, double s0) {
    if (A.wdone && s0_infeasible(A.p, s0)) {
        A.wdone[i] = 3;
        A.sqp_iter[i] = 0;
    }
}

// NMPC_controller.solve prologue (NMPC_controller.m:332-384) or acados-level init copy.
__global__ void prologue_kernel(SolveArgs A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.B) return;
    const SolveParams& p = A.p;
    const int N = p.N;
    const ShapeDev& sh = shape_of(A, i);
    double x0[4];
    for (int c = 0; c < 4; ++c) x0[c] = A.x0[(size_t)i * 4 + c];
    double* X = A.wX + (size_t)i * (N + 1) * 4;
    double* U = A.wU + (size_t)i * N * 2;
    A.qp_iter[i] = 0;
    if (A.qp_capped) A.qp_capped[i] = 0;
    if (A.qp_stalled) A.qp_stalled[i] = 0;
    if (A.wdone) A.wdone[i] = 0;
    if (A.wnit) A.wnit[i] = 0;
    if (A.wadjv) A.wadjv[i] = 0;   // no successful QP yet: PI_out keeps what it holds (the warm start's)
    if (!(A.flags & QSP_FLAG_CONTROLLER)) {
        for (int q = 0; q < (N + 1) * 4; ++q) X[q] = A.X_in[(size_t)i * (N + 1) * 4 + q];
        for (int q = 0; q < N * 2; ++q) U[q] = A.U_in[(size_t)i * N * 2 + q];
        for (int c = 0; c < 4; ++c) A.wx0[(size_t)i * 4 + c] = x0[c];
        if (p.nlp_mode == 1) nlp_init(A, i, true);
        s0_feasible(A, i, x0[3]);
        return;
    }
    const bool cold = (A.warm_valid == nullptr || A.warm_valid[i] == 0);
    controller_guess(sh, p, cold, A.U_in + (size_t)i * N * 2, x0, U, X);    // :332, :351-380
    for (int c = 0; c < 4; ++c) A.wx0[(size_t)i * 4 + c] = x0[c];
    if (p.nlp_mode == 1) nlp_init(A, i, !cold);                             // :351-355 (PI = 0 cold)
    s0_feasible(A, i, x0[3]);
}

// The QP of one SQP iteration in the register/LDS-resident lane-group layout:
// load stage data, Mehrotra IPM, roll out the damped step, update the SQP iterate.
// Dynamics multipliers of the QP solution, one per stage lane (S = 1): lane k < N
// returns pi_k (same adjoint recursion as qp_adjoint_store).
__device__ __forceinline__ void qp_adjoint_lane(const Ctx& c, const SolveParams& p, const Stage<1>& st,
                                                double piq[4]) {
    double pi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i) piq[i] = 0.0;
    for (int j = c.L - 1; j >= 0; --j) {
        if (c.lig == j) {
            if (j == c.N) {
#pragma unroll
                for (int i = 0; i < 4; ++i) pi[i] = qfma(p.We[i], st.dxs(0, i), st.g[0][i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) piq[i] = pi[i];
                if (j >= 1) {
                    const double dxk[4] = {st.dxs(0, 0), st.dxs(0, 1), st.dxs(0, 2), st.dxs(0, 3)};
                    adjoint_step(p, st.a[0], dxk, st.g[0], st.lm(0, 1) - st.lm(0, 0), pi);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) pi[i] = wave_from_next(pi[i]);
    }
}

// ------------------------------------------------------------------ nlp_mode 1
// acados 'SQP' + 'merit_backtracking' (NMPC_controller.m:271-276), restated in the
// oracle's sqp_solve.  One SQP iteration = linearize, qp_step<1, true> (KKT test of the
// current iterate -> converged instances freeze; QP; its solution into wqp), and
// merit_ls_kernel (merit weights from the QP multipliers, Armijo backtracking on the l1
// merit function, damped multiplier update).  One stage per lane: lane k of a group owns
// stage k, every per-stage term is lane-parallel, horizon sums/maxima are group reductions.
// Workspaces: NlpField, QpField (qsp_kernels.h), SoA over (instance, stage) like wlin.

// KKT residuals of the NLP at the current iterate against tol_* (max norms over the
// horizon); `nlp` points at this lane's stage in the W_* SoA (stride tot).  res (the instance's
// 4 doubles, or nullptr): the residuals are recorded there (acados' res_stat/eq/ineq/comp
// statistics of the last test, qsp_get_residuals).
__device__ bool nlp_converged(const Ctx& c, const SolveParams& p, const Stage<1>& st, const double* nlp, size_t tot,
                              double* res) {
    const int N = p.N;
    const int k = c.lig;
    double PIk[4], LAMk[6];
#pragma unroll
    for (int q = 0; q < 4; ++q) PIk[q] = nlp[(W_PI + q) * tot];
#pragma unroll
    for (int q = 0; q < 6; ++q) LAMk[q] = nlp[(W_LAM + q) * tot];
    double PIp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) PIp[q] = wave_from_prev(PIk[q]);   // pi_{k-1}
    double rs = 0.0, re = 0.0, ri = 0.0, rc = 0.0;
    const double v[3] = {st.v(0, 0), st.v(0, 1), st.v(0, 2)};
    kkt_stage(p, k, st.a[0], st.B[0], st.g[0], st.bb[0], v, PIk, PIp, LAMk, rs, rs, rs, re, ri, rc);   // one stationarity maximum
    rs = group_max(rs, c.gs);
    re = group_max(re, c.gs);
    ri = group_max(ri, c.gs);
    rc = group_max(rc, c.gs);
    if (res && c.real && c.lig == 0) {
        res[0] = rs;
        res[1] = re;
        res[2] = ri;
        res[3] = rc;
    }
    return rs < p.tol_stat && re < p.tol_eq && ri < p.tol_ineq && rc < p.tol_comp;
}

// The SQP's reaction to a QP's exit (both SQP kernels): counts of capped and stalled QPs; a
// diverged QP (status 4, acados ACADOS_QP_FAILURE) or a non-finite solution (status 1) stops the
// instance's SQP with its last iterate, as the oracle's sqp_solve does.  Returns that failure.
template <int S>
__device__ __forceinline__ bool qp_outcome(const SolveArgs& A, const Ctx& c, const Stage<S>& st, int iv, int it,
                                           int exit, bool skip) {
    const int N = c.N;
    if (c.real && c.lig == 0 && !skip) {
        if (A.qp_capped && exit == QP_EXIT_CAP) A.qp_capped[iv] += 1;
        if (A.qp_stalled && exit == QP_EXIT_STALL) A.qp_stalled[iv] += 1;
    }
    if (!A.wdone) return false;
    double bad = 0.0;
#pragma unroll
    for (int ls = 0; ls < S; ++ls) {
        const int k = kof<S>(c, ls);
#pragma unroll
        for (int q = 0; q < 4; ++q) bad = (k > N || isfinite(st.dxs(ls, q))) ? bad : 1.0;
        bad = (k >= N || (isfinite(st.du(ls, 0)) && isfinite(st.du(ls, 1)))) ? bad : 1.0;
    }
    const double badg = group_max(bad, c.gs);   // every lane takes part in the DPP scan
    const bool div = exit == QP_EXIT_DIVERGED;
    const bool failed = !skip && (div || badg > 0.0);
    if (failed && c.real && c.lig == 0) {
        A.wdone[iv] = div ? 4 : 2;
        A.sqp_iter[iv] = it;
    }
    return failed;
}

// ---- pieces the SQP kernels (qp_step_kernel, sqp_loop_kernel) share as functions.  The fused kernel's
// bit identity to the per-iteration launches rests on both computing the same.  The linearisation's
// stage load and dx0 are still written out in both, and the stage load a third time in the twin's
// load_stage: as one function it costs the SQP kernels up to 15 VGPRs (profiles/ipm_shared/README.md),
// so the three must be edited together.  Written out in the kernels and in the twin besides, for the
// reasons measured there: qp_ipm's start point, its t.lm sum and centring scalar (twin: qp_ipm), and
// merit_ls_kernel's directional-derivative term (twin: merit_ls).  Everything else per-lane around the
// solve -- prologue, status, shift, cost, staging, the closed loop's steps -- is one function in
// qsp_math.hpp or qsp_ipm.hpp that both sides call (profiles/wrapper_shared/README.md).
// debug (QSP_FLAG_POISON): this thread's LDS column filled with NaN
template <int S>
__device__ __forceinline__ void poison_lds(double* col) {
    for (int f = 0; f < F_COUNT * S + mfw_extra(S); ++f) col[f * BLOCK] = __builtin_nan("");
}

// the bounded components (s_k, u_n, u_t) of slot ls's stage into LDS (kc, ku: the stage clamped to N, N - 1)
template <int S>
__device__ __forceinline__ void load_bounded(const Stage<S>& st, int ls, int kc, int ku, const double* X, const double* U) {
    st.v(ls, 0) = X[4 * kc + 3];
    st.v(ls, 1) = U[2 * ku];
    st.v(ls, 2) = U[2 * ku + 1];
}

// the full Gauss-Newton step: X += dx, U += du, and the instance's IPM iteration count
template <int S>
__device__ __forceinline__ void iterate_update(const SolveArgs& A, const Ctx& c, const Stage<S>& st, int iv, int nit,
                                               double* X, double* U) {
    const int N = c.N;
#pragma unroll
    for (int ls = 0; ls < S; ++ls) {
        const int k = kof<S>(c, ls);
        if (k <= N)
            for (int q = 0; q < 4; ++q) X[4 * k + q] += st.dxs(ls, q);
        if (k < N) {
            U[2 * k] += st.du(ls, 0);
            U[2 * k + 1] += st.du(ls, 1);
        }
        if (k == 0) A.qp_iter[iv] += nit;
    }
}

// NC: the horizon compiled in (0: read from p.N; see ctx_of and QSP_FIXED_HORIZONS)
template <int S, bool MERIT = false, bool LIN = false, bool ALT = false, int NC = 0>
__global__ void __launch_bounds__(BLOCK, QSP_MIN_WAVES) qp_step_kernel(SolveArgs A, int it) {
    SEG_T(t_k);
    extern __shared__ double smem[];
    const SolveParams& p = A.p;
    const Ctx c = ctx_of<S, NC>(threadIdx.x & 63, p.N, A.nI);
    // instances are packed into waves in the order of their previous IPM iteration count
    // (sort_by_iters_kernel), so the instances sharing a wave finish together
    const int slot = A.i0 + (c.real ? c.inst : A.nI - 1);
    const int iv = A.wperm ? A.wperm[slot] : slot;
    const int N = c.N;
    const size_t tot = (size_t)A.B * (N + 1);
    Stage<S> st;
    st.lds = smem + threadIdx.x;
    if (A.flags & QSP_FLAG_POISON) {
        for (int f = 0; f < F_COUNT * S + mfw_extra(S); ++f) st.lds[f * BLOCK] = __builtin_nan("");
    }
    double* X = A.wX + (size_t)iv * (N + 1) * 4;
    double* U = A.wU + (size_t)iv * N * 2;
    // frozen instances (converged in nlp_mode 1, or a failed QP earlier) are not iterated
    const bool was_done = A.wdone && A.wdone[iv] != 0;
    const bool lin_live = c.real && !was_done;   // fused linearisation only where it is used
#pragma unroll
    for (int ls = 0; ls < S; ++ls) {
        const int k = kof<S>(c, ls);
        const int kc = k <= N ? k : N;
        const int ku = k < N ? k : N - 1;
        if constexpr (LIN) {
            // the SQP iteration's linearisation, one stage per slot (RK4 + sensitivities): the
            // stage data stays in registers instead of a 24-double HBM round trip
            if (kc < N && lin_live) {
                const double xk[4] = {X[4 * kc], X[4 * kc + 1], X[4 * kc + 2], X[4 * kc + 3]};
                const double uk[2] = {U[2 * kc], U[2 * kc + 1]};
#ifdef QSP_SEGSTAMP
                {   // (diagnostic build: the iterate's loads complete before the stamp)
                    double w = xk[0] + xk[1] + xk[2] + xk[3] + uk[0] + uk[1];
                    asm volatile("" : "+v"(w));
                    SEG_NEXT(14, t_k);
                }
#endif
                Lin Ln;
                rk4<true>(shape_of(A, iv), p.Ts, xk, uk, Ln);
#ifdef QSP_SEGSTAMP
                {
                    double w = Ln.a[0] + Ln.B[0] + Ln.xn[0];
                    asm volatile("" : "+v"(w));
                    SEG_NEXT(15, t_k);
                }
#endif
                const double* yr = A.yref + ((size_t)iv * N + kc) * 6;
#pragma unroll
                for (int q = 0; q < 6; ++q) st.a[ls][q] = Ln.a[q];
#pragma unroll
                for (int q = 0; q < 8; ++q) st.B[ls][q] = Ln.B[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) st.bb[ls][q] = Ln.xn[q] - X[4 * (kc + 1) + q];
#pragma unroll
                for (int q = 0; q < 4; ++q) st.g[ls][q] = p.tau * p.W[q] * (xk[q] - yr[q]);
#pragma unroll
                for (int q = 0; q < 2; ++q) st.g[ls][4 + q] = p.tau * p.W[4 + q] * (uk[q] - yr[4 + q]);
            } else {   // terminal stage (or an instance that does not iterate): no dynamics
                const double* ye = A.yref_e + (size_t)iv * 4;
#pragma unroll
                for (int q = 0; q < 6; ++q) st.a[ls][q] = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) st.B[ls][q] = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) st.bb[ls][q] = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) st.g[ls][q] = p.We[q] * (X[4 * N + q] - ye[q]);
                st.g[ls][4] = 0.0;
                st.g[ls][5] = 0.0;
            }
        } else {
            const double* in = A.wlin + (size_t)iv * (N + 1) + kc;
#pragma unroll
            for (int q = 0; q < 6; ++q) st.a[ls][q] = in[(L_A + q) * tot];
#pragma unroll
            for (int q = 0; q < 8; ++q) st.B[ls][q] = in[(L_B + q) * tot];
#pragma unroll
            for (int q = 0; q < 4; ++q) st.bb[ls][q] = in[(L_BB + q) * tot];
#pragma unroll
            for (int q = 0; q < 6; ++q) st.g[ls][q] = in[(L_G + q) * tot];
        }
        load_bounded<S>(st, ls, kc, ku, X, U);
    }
    if constexpr (MERIT && LIN) {
        // the line search (merit_ls_kernel) evaluates the defect and gradient at the same point
        if (lin_live && c.lig <= N) {
            double* out = A.wlin + (size_t)iv * (N + 1) + c.lig;
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(L_BB + q) * tot] = st.bb[0][q];
#pragma unroll
            for (int q = 0; q < 6; ++q) out[(L_G + q) * tot] = st.g[0][q];
        }
    }
    double dx0[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) dx0[q] = A.wx0[(size_t)iv * 4 + q] - X[q];   // used by lane lig == 0
    // padding lanes (no instance) must not hold their wave in the IPM loop: they mirror
    // instance B-1 with group reductions over foreign lanes and need not converge
    bool skip = was_done || !c.real;
    if constexpr (MERIT) {
        static_assert(S == 1, "nlp_mode 1 uses one stage per lane");
        // nlp_mode 1: KKT test of the current iterate; converged instances freeze
        const bool conv = !was_done && nlp_converged(c, p, st, A.wnlp + (size_t)iv * (N + 1) + c.lig, tot,
                                                     A.wres ? A.wres + (size_t)iv * 4 : nullptr);
        skip = was_done || conv || !c.real;
        if (conv && c.real && c.lig == 0) {
            A.wdone[iv] = 1;
            A.sqp_iter[iv] = it;
        }
    }
    int exit;
    SEG_NEXT(10, t_k);
    const int nit = qp_ipm<S, ALT, NC>(c, p, st, dx0, exit, skip);
    SEG_NEXT(11, t_k);
    qp_rollout<S>(c, st, dx0);
    const bool failed = qp_outcome<S>(A, c, st, iv, it, exit, skip);
    if (A.wnit && c.real && c.lig == 0) {
        // wave-packing record and key of this instance for the next launch
        // (sort_by_iters_kernel); an instance that did not iterate keeps its record
        const int old = A.wnit[iv];
        const int rec = (MERIT || !(skip || failed)) ? pack_record(old, nit) : old;
        A.wnit[iv] = rec;
        if (A.whist) atomicAdd(&A.whist[(it & 1) * PACK_KEYS_MAX + pack_key(rec, pack_maxkey(p.qp_iters))], 1);
    }
    if constexpr (MERIT) {
        // QP solution (step, dynamics and bound multipliers) for the line-search kernel
        double piq[4];
        qp_adjoint_lane(c, p, st, piq);
        if (c.real && !skip && !failed) {
            const size_t si = (size_t)iv * (N + 1) + c.lig;
            double* w = A.wqp + si;
#pragma unroll
            for (int q = 0; q < 4; ++q) w[(Q_DX + q) * tot] = st.dxs(0, q);
#pragma unroll
            for (int q = 0; q < 2; ++q) w[(Q_DU + q) * tot] = c.lig < N ? st.du(0, q) : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) w[(Q_PI + q) * tot] = piq[q];
#pragma unroll
            for (int q = 0; q < 6; ++q) w[(Q_LAM + q) * tot] = c.lig < N ? st.lm(0, q) : 0.0;
        }
        if (c.real && c.lig == 0) A.qp_iter[iv] += nit;
        return;
    }
    const bool last = it + 1 >= p.sqp_iters;
    if (A.qp_dx) {
        // QP-level interface (qsp_qp_solve): report the QP solution itself
        if (last) qp_adjoint_store<S>(c, p, st, A.PI_out + (size_t)iv * N * 4, c.real, false);
        if (!c.real) return;
#pragma unroll
        for (int ls = 0; ls < S; ++ls) {
            const int k = kof<S>(c, ls);
            if (k <= N)
                for (int q = 0; q < 4; ++q) A.qp_dx[((size_t)iv * (N + 1) + k) * 4 + q] = st.dxs(ls, q);
            if (k < N) {
                for (int q = 0; q < 2; ++q) A.qp_du[((size_t)iv * N + k) * 2 + q] = st.du(ls, q);
                for (int q = 0; q < 6; ++q) A.qp_lam[((size_t)iv * N + k) * 6 + q] = st.lm(ls, q);
            }
            if (k == 0) A.qp_iter[iv] = nit;
            if (k == 0 && A.qp_capped) A.qp_capped[iv] = qp_exit_status(exit);   // (qsp_qp_solve)
        }
        return;
    }
    if (!c.real || skip || failed) return;
    SEG_NEXT(12, t_k);
    // adjoint record of every successful QP (the epilogue forms the multipliers of the last
    // one, also for an instance that stops early: a failed QP leaves the record as it was)
    qp_adjoint_record<S>(c, p, st, A.wadj + (size_t)iv * N * ADJ_REC);
    if (c.lig == 0) A.wadjv[iv] = 1;
    SEG_NEXT(16, t_k);
    iterate_update<S>(A, c, st, iv, nit, X, U);
    SEG_ADD(12, t_k);
}

// Small batches (fewer waves than the chip's 2 048 wave slots), nlp_mode 0: the whole SQP loop
// in one launch.  Every wave keeps its instances for all K iterations, so a solve costs the
// slowest wave's own sum of IPM iterations instead of the sum over iterations of the slowest
// wave of the batch (no packing sort, no grid-wide boundary between SQP iterations).  The
// per-iteration arithmetic is qp_step_kernel<S, false, true>'s (same helpers, same order), so
// the results are bit-identical to the per-iteration launches (tests/test_gpu_fullsize.py).
template <int S, bool ALT = false>
__global__ void __launch_bounds__(BLOCK, QSP_MIN_WAVES) sqp_loop_kernel(SolveArgs A) {
    extern __shared__ double smem[];
    const SolveParams& p = A.p;
    const int N = p.N;
    if (A.flags & QSP_FLAG_POISON) poison_lds<S>(smem + threadIdx.x);
    bool stopped = false;   // group-uniform: a failed QP stops the instance's SQP
    for (int it = 0; it < p.sqp_iters; ++it) {
        if (it > 0) __syncthreads();   // the neighbour lanes' X, U stores of the last iteration
        // debug: re-poisoned at every SQP iteration, so a read of a word the current iteration
        // did not write shows up (the last iteration's finite values would hide it)
        if (it > 0 && (A.flags & QSP_FLAG_POISON)) poison_lds<S>(smem + threadIdx.x);
        // lane geometry and addresses re-derived every iteration from an opaque lane id: hoisted
        // out of the loop they would stay live through the interior point (register budget)
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const Ctx c = ctx_of<S>(lane, N, A.nI);
        const int iv = A.i0 + (c.real ? c.inst : A.nI - 1);
        double* X = A.wX + (size_t)iv * (N + 1) * 4;
        double* U = A.wU + (size_t)iv * N * 2;
        if (it == 0) stopped = A.wdone[iv] != 0;
        // a fresh register block per iteration: the factor walk writes K, Rn, kk in place under
        // a lane mask, which would otherwise keep the last iteration's values live
        Stage<S> st;
        st.lds = smem + threadIdx.x;
        const bool lin_live = c.real && !stopped;
#pragma unroll
        for (int ls = 0; ls < S; ++ls) {
            const int k = kof<S>(c, ls);
            const int kc = k <= N ? k : N;
            const int ku = k < N ? k : N - 1;
            if (kc < N && lin_live) {
                const double xk[4] = {X[4 * kc], X[4 * kc + 1], X[4 * kc + 2], X[4 * kc + 3]};
                const double uk[2] = {U[2 * kc], U[2 * kc + 1]};
                Lin Ln;
                rk4<true>(shape_of(A, iv), p.Ts, xk, uk, Ln);
                const double* yr = A.yref + ((size_t)iv * N + kc) * 6;
#pragma unroll
                for (int q = 0; q < 6; ++q) st.a[ls][q] = Ln.a[q];
#pragma unroll
                for (int q = 0; q < 8; ++q) st.B[ls][q] = Ln.B[q];
#pragma unroll
                for (int q = 0; q < 4; ++q) st.bb[ls][q] = Ln.xn[q] - X[4 * (kc + 1) + q];
#pragma unroll
                for (int q = 0; q < 4; ++q) st.g[ls][q] = p.tau * p.W[q] * (xk[q] - yr[q]);
#pragma unroll
                for (int q = 0; q < 2; ++q) st.g[ls][4 + q] = p.tau * p.W[4 + q] * (uk[q] - yr[4 + q]);
            } else {
                const double* ye = A.yref_e + (size_t)iv * 4;
#pragma unroll
                for (int q = 0; q < 6; ++q) st.a[ls][q] = 0.0;
#pragma unroll
                for (int q = 0; q < 8; ++q) st.B[ls][q] = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) st.bb[ls][q] = 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) st.g[ls][q] = p.We[q] * (X[4 * N + q] - ye[q]);
                st.g[ls][4] = 0.0;
                st.g[ls][5] = 0.0;
            }
            load_bounded<S>(st, ls, kc, ku, X, U);
        }
        double dx0[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) dx0[q] = A.wx0[(size_t)iv * 4 + q] - X[q];
        const bool skip = stopped || !c.real;
        int exit;
        const int nit = qp_ipm<S, ALT>(c, p, st, dx0, exit, skip);
        qp_rollout<S>(c, st, dx0);
        const bool failed = qp_outcome<S>(A, c, st, iv, it, exit, skip);
        if (c.real && !skip && !failed) {
            qp_adjoint_record<S>(c, p, st, A.wadj + (size_t)iv * N * ADJ_REC);
            if (c.lig == 0) A.wadjv[iv] = 1;
            iterate_update<S>(A, c, st, iv, nit, X, U);
        }
        stopped = stopped || failed;
    }
}

// Counting sort of the instances by their packing key (pack_key) in one pass over the
// instances: the histogram of the keys was accumulated by the QP launch itself (whist,
// parity q); every block forms the exclusive prefix of the histogram (a block-wide scan),
// places its instances at the key's prefix plus a block offset taken from the running
// counters, and block 0 clears the other parity's histogram and counters for the next
// launch.  The order inside a key is arbitrary and does not affect any result (instances
// are independent).  Sorts the instance range [i0, i0 + B) into perm[i0 ...] (one part of a
// split SQP loop, with the part's own whist).
__global__ void __launch_bounds__(256) sort_by_iters_kernel(int i0, int B, int maxkey, const int32_t* nit,
                                                            int32_t* perm, int32_t* whist, int q) {
    constexpr int KPT = PACK_KEYS_MAX / 256;   // keys per thread in the prefix scan
    __shared__ int pre[PACK_KEYS_MAX], lcount[PACK_KEYS_MAX], part[256];
    const int tid = threadIdx.x;
    const int nkeys = (maxkey + 1) * (maxkey + 1);
    const int32_t* hist = whist + q * PACK_KEYS_MAX;
    int32_t* run = whist + (2 + q) * PACK_KEYS_MAX;
    int h[KPT], sum = 0;
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
        const int k = tid * KPT + r;
        h[r] = k < nkeys ? hist[k] : 0;
        sum += h[r];
        lcount[k] = 0;
    }
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive scan of the per-thread sums
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int acc = part[tid] - sum;
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
        pre[tid * KPT + r] = acc;
        acc += h[r];
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + tid;
    int key = 0, pos = 0;
    if (i < B) {
        key = pack_key(nit[i0 + i], maxkey);
        pos = atomicAdd(&lcount[key], 1);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < KPT; ++r) {
        const int k = tid * KPT + r;
        if (lcount[k] > 0) pre[k] += atomicAdd(&run[k], lcount[k]);
    }
    __syncthreads();
    if (i < B) perm[i0 + pre[key] + pos] = i0 + i;
    if (blockIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            whist[(1 - q) * PACK_KEYS_MAX + tid * KPT + r] = 0;
            whist[(3 - q) * PACK_KEYS_MAX + tid * KPT + r] = 0;
        }
    }
}

__global__ void iota_kernel(int B, int32_t* perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) perm[i] = i;
}

// nlp_mode 1 line search and update (one stage per lane, no LDS): merit weights
// nu = max(|pi|, (nu + |pi|)/2), eta likewise from the QP bound multipliers; phi(0) and
// its directional derivative; alpha <- ls_alpha_red * alpha until
// phi(alpha) <= phi(0) + ls_eps alpha dphi or alpha would drop below ls_alpha_min (then
// the last alpha tried is taken); X, U, PI, LAM updated with that alpha.
__global__ void __launch_bounds__(64) merit_ls_kernel(SolveArgs A) {
    const SolveParams& p = A.p;
    const Ctx c = ctx_of<1>(threadIdx.x & 63, p.N, A.nI);
    // the QP launch's wave packing (instances ordered by their predicted IPM count) also groups
    // the line searches: a wave backtracks until the last of its instances accepts a step
    const int slot = A.i0 + (c.real ? c.inst : A.nI - 1);
    const int iv = A.wperm ? A.wperm[slot] : slot;
    const int N = p.N;
    const int k = c.lig <= N ? c.lig : N;
    const bool stg = k < N;
    const int ku = stg ? k : N - 1;
    const size_t tot = (size_t)A.B * (N + 1);
    const size_t si = (size_t)iv * (N + 1) + k;
    // converged instances (this or an earlier iteration) keep their iterate; the QP kernel
    // wrote no step for them
    const bool skip = !c.real || A.wdone[iv] != 0;
    const ShapeDev& sh = shape_of(A, iv);
    double* X = A.wX + (size_t)iv * (N + 1) * 4;
    double* U = A.wU + (size_t)iv * N * 2;
    // what the backtracking loop reads stays in registers; the multipliers are read again
    // for the update after it (fewer live registers: more waves per SIMD)
    double xk[4], uk[2], dxk[4], duk[2], bb[4], g[6];
    double NUk[4], ETAk[6];
#pragma unroll
    for (int q = 0; q < 4; ++q) xk[q] = X[4 * k + q];
    uk[0] = U[2 * ku];
    uk[1] = U[2 * ku + 1];
    const double* w = A.wqp + si;
    const double* in = A.wlin + si;
    const double* nl = A.wnlp + si;
#pragma unroll
    for (int q = 0; q < 4; ++q) dxk[q] = skip ? 0.0 : w[(Q_DX + q) * tot];
#pragma unroll
    for (int q = 0; q < 2; ++q) duk[q] = (skip || !stg) ? 0.0 : w[(Q_DU + q) * tot];
#pragma unroll
    for (int q = 0; q < 4; ++q) bb[q] = in[(L_BB + q) * tot];
#pragma unroll
    for (int q = 0; q < 6; ++q) g[q] = in[(L_G + q) * tot];
#pragma unroll
    for (int q = 0; q < 4; ++q) NUk[q] = nl[(W_NU + q) * tot];
#pragma unroll
    for (int q = 0; q < 6; ++q) ETAk[q] = nl[(W_ETA + q) * tot];
    if (stg) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            NUk[q] = merit_weight(NUk[q], skip ? 0.0 : fabs(w[(Q_PI + q) * tot]));
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            ETAk[q] = merit_weight(ETAk[q], skip ? 0.0 : fabs(w[(Q_LAM + q) * tot]));
        }
    }
    const double* yr = A.yref + ((size_t)iv * N + ku) * 6;
    const double* ye = A.yref_e + (size_t)iv * 4;
    double dph = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) dph = qfma(g[i], dxk[i], dph);
    if (stg) {
        dph = qfma(g[5], duk[1], qfma(g[4], duk[0], dph));
#pragma unroll
        for (int i = 0; i < 4; ++i) dph = qfma(-NUk[i], fabs(bb[i]), dph);
        const double v[3] = {xk[3], uk[0], uk[1]};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (j == 0 && k == 0 && !p.s0_bound) continue;
            const double lo = p.lh[j] - v[j], hi = p.uh[j] - v[j];
            if (lo > 0.0) dph = qfma(-ETAk[2 * j], lo, dph);
            if (hi < 0.0) dph = qfma(ETAk[2 * j + 1], hi, dph);
        }
    }
    const double phi0 = group_sum(merit_stage(p, k, xk, uk, yr, ye, bb, NUk, ETAk), c.gs);
    const double dphi = group_sum(dph, c.gs);
    double alpha = 1.0;
    bool fin = skip;
    while (__ballot(!fin) != 0ull) {
        double xt[4], ut[2], xnx[4], def[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) xt[q] = qfma(alpha, dxk[q], xk[q]);
        ut[0] = qfma(alpha, duk[0], uk[0]);
        ut[1] = qfma(alpha, duk[1], uk[1]);
#pragma unroll
        for (int q = 0; q < 4; ++q) xnx[q] = wave_from_next(xt[q]);   // x_{k+1} + alpha dx_{k+1}
        if (stg) {
            Lin Lt;
            rk4<false>(sh, p.Ts, xt, ut, Lt);
#pragma unroll
            for (int q = 0; q < 4; ++q) def[q] = Lt.xn[q] - xnx[q];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) def[q] = 0.0;
        }
        const double phi = group_sum(merit_stage(p, k, xt, ut, yr, ye, def, NUk, ETAk), c.gs);
        if (!fin) {
            if (phi <= qfma(p.ls_eps * alpha, dphi, phi0)) {
                fin = true;
            } else {
                const double an = alpha * p.ls_alpha_red;
                if (an < p.ls_alpha_min) fin = true;      // accept the last step tried
                else alpha = an;
            }
        }
    }
    if (skip) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) X[4 * k + q] = qfma(alpha, dxk[q], xk[q]);
    if (stg) {
        U[2 * k] = qfma(alpha, duk[0], uk[0]);
        U[2 * k + 1] = qfma(alpha, duk[1], uk[1]);
        double* nw = A.wnlp + si;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            nw[(W_PI + q) * tot] = damp_update(alpha, w[(Q_PI + q) * tot], nw[(W_PI + q) * tot]);
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            nw[(W_LAM + q) * tot] = damp_update(alpha, w[(Q_LAM + q) * tot], nw[(W_LAM + q) * tot]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) nw[(W_NU + q) * tot] = NUk[q];
#pragma unroll
        for (int q = 0; q < 6; ++q) nw[(W_ETA + q) * tot] = ETAk[q];
    }
}

// status, cost, u0 and the (optionally shifted, NMPC_controller.m:397-399) outputs.
static_assert(QSP_STATUS_SUCCESS == ST_SUCCESS && QSP_STATUS_NAN == ST_NAN && QSP_STATUS_MAXITER == ST_MAXITER &&
              QSP_STATUS_QP_FAIL == ST_QP_FAIL, "solve_status (qsp_ipm.hpp) returns the public QSP_STATUS_*");
__global__ void epilogue_kernel(SolveArgs A) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.B) return;
    const SolveParams& p = A.p;
    const int N = p.N;
    const double* X = A.wX + (size_t)i * (N + 1) * 4;
    const double* U = A.wU + (size_t)i * N * 2;
    const double* yref = A.yref + (size_t)i * N * 6;
    const double* ye = A.yref_e + (size_t)i * 4;
    A.cost[i] = solve_cost(p, X, U, yref, ye);
    // x0 is part of the returned iterate; the SQP's record wdone: solve_status (qsp_ipm.hpp)
    const bool bad = iterate_nonfinite(N, X, U, A.wx0 + (size_t)i * 4);
    A.status[i] = solve_status(p, bad, A.wdone ? A.wdone[i] : 0, A.sqp_iter[i]);
    A.u0[(size_t)i * 2] = U[0];
    A.u0[(size_t)i * 2 + 1] = U[1];
    const int sh = (A.flags & QSP_FLAG_SHIFT) ? 1 : 0;
    shift_rows<4>(N + 1, sh, X, 4, 1, A.X_out + (size_t)i * (N + 1) * 4);
    shift_rows<2>(N, sh, U, 2, 1, A.U_out + (size_t)i * N * 2);
    if (p.nlp_mode == 1) {
        // dynamics multipliers of the NLP iterate (shifted like X/U in controller mode)
        const size_t tot = (size_t)A.B * (N + 1);
        shift_rows<4>(N, sh, A.wnlp + W_PI * tot + (size_t)i * (N + 1), 1, tot, A.PI_out + (size_t)i * N * 4);
    }
    if (p.nlp_mode == 0 && A.wadjv && A.wadjv[i] != 0) {
        // dynamics multipliers of the last successful QP, once per solve; an instance without
        // one (stage-0 bound, a failure at the first QP) keeps what PI_out held
        adjoint_from_record(N, A.wadj + (size_t)i * N * ADJ_REC, A.PI_out + (size_t)i * N * 4, sh != 0);
    }
    if (A.warm_valid && (A.flags & QSP_FLAG_CONTROLLER)) A.warm_valid[i] = 1;
}

// ------------------------------------------------------------------ launchers
// The QP kernels take more than 64 KB of dynamic LDS, which a kernel must be allowed once per
// device (one bit per device in `done`; handles on several devices may share a process).
static hipError_t lds_attr_once(const void* kernel, int bytes, std::atomic<uint64_t>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_acq_rel);
    return e;
}

// The QP kernels' grid: one workgroup per wave of instances, with the stage count's dynamic LDS
// (allowed once per kernel and device).  extra: the kernel's arguments after SolveArgs.
template <auto KERNEL, int S, class... Extra>
static hipError_t launch_qp_waves(const SolveArgs& a, hipStream_t stream, Extra... extra) {
    static std::atomic<uint64_t> attr{0};   // one per KERNEL
    const hipError_t e = lds_attr_once((const void*)KERNEL, lds_bytes(S), attr);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)waves_for(a.nI, a.p.N, S)), dim3(BLOCK), lds_bytes(S), stream, a, extra...);
    return hipGetLastError();
}

// The kernel variant of a handle.  ALT is the alternative factorisation of the stage count: at one
// stage per lane the walk on the matrix cores (mfw_use), at two the associative scan
// (SolveParams::factor_scan); two stages per lane take the matrix cores inside the kernel (mfw_use).
// Which factorisation that is: factor_walk_of (qsp_layout.h), the rule the twin follows too.  Every launcher
// selects through factor_alt / with_variant.
static_assert(QSP_WALK_LANE == WALK_LANE && QSP_WALK_MFMA == WALK_MFMA && QSP_WALK_SCAN == WALK_SCAN, "QSP_WALK_*");
int factor_walk_kind(const SolveParams& p, int S) { return factor_walk_of(p.N, S, p.mfma_walk, p.factor_scan); }
static bool factor_alt(const SolveParams& p, int S) { return factor_walk_kind(p, S) == (S == 1 ? WALK_MFMA : WALK_SCAN); }

// f(S, ALT) with the handle's variant as compile-time constants
template <class F>
static hipError_t with_variant(const SolveParams& p, int S, F&& f) {
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    const bool alt = factor_alt(p, S);
    switch (S) {
        case 1: return alt ? f(one{}, std::true_type{}) : f(one{}, std::false_type{});
        case 2: return alt ? f(two{}, std::true_type{}) : f(two{}, std::false_type{});
        default: return hipErrorInvalidValue;
    }
}

// sqp_loop_kernel keeps more state live across its SQP loop than qp_step_kernel and runs at
// 1 wave/SIMD (256 VGPRs + AGPRs), so it pays only while its waves fit the SIMDs (4 per CU:
// 1 024 on a whole MI355X) in one round.  Measured (scripts/fused_sweep.sh, N = 20, K = 50,
// S = 1, solves/s per-iteration launches -> fused): B = 1 024 58.7k -> 76.5k; 2 048 115k ->
// 123k; 3 072 (1 024 waves) 173k -> 224k; 4 096 (1 366 waves, two rounds) 227k -> 169k.
int sqp_fused_auto(int B, int N, int S, int nlp_mode, int cus) {
    const long waves = waves_for(B, N, S);
    return (nlp_mode == 0 && (S == 1 || S == 2) && waves <= 4L * cus) ? 1 : 0;
}

// The horizons qp_step_kernel is also compiled for, one X(N) each (one stage per lane on the matrix
// cores, with and without the linearisation).  A handle's horizon is fixed at its creation, so at
// these the kernel need not carry N as data (ctx_of); every other horizon, variant and kernel takes the
// runtime-horizon code.  Results are the same bits either way; QSP_FIXED_HORIZON=0 forces the latter.
#define QSP_FIXED_HORIZONS(X) X(20)

// lin: the SQP iteration's linearisation runs inside the QP kernel (nlp_mode 0); without it the
// kernel reads the stage data the workspace holds (qsp_qp_solve).
// The compiled horizon the per-iteration QP launches of a handle take (0: the runtime-horizon kernel):
// p.N where QSP_FIXED_HORIZONS lists it, on the one-stage matrix-core variant, unless the switch forbids it.
int qp_fixed_horizon(const SolveParams& p, int S, uint32_t flags) {
    if (S != 1 || !factor_alt(p, 1) || (flags & QSP_FLAG_RUNTIME_N)) return 0;
#define QSP_FIXED_IS(n) if (p.N == n) return n;
    QSP_FIXED_HORIZONS(QSP_FIXED_IS)
#undef QSP_FIXED_IS
    return 0;
}

static hipError_t launch_qp_fixed(const SolveArgs& a, int it, hipStream_t stream, bool lin);
static hipError_t launch_qp_any(const SolveArgs& a, int S, int it, hipStream_t stream, bool lin) {
    if (qp_fixed_horizon(a.p, S, a.flags)) return launch_qp_fixed(a, it, stream, lin);   // the kernel compiled for it (same bits)
    return with_variant(a.p, S, [&](auto s, auto alt) {
        return lin ? launch_qp_waves<qp_step_kernel<s(), false, true, alt()>, s()>(a, stream, it)
                   : launch_qp_waves<qp_step_kernel<s(), false, false, alt()>, s()>(a, stream, it);
    });
}

#ifdef QSP_SEGSTAMP
// diagnostic build: read (and optionally clear) the segment cycle sums
extern "C" int qsp_debug_segments(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_seg), sizeof(g_seg)) != hipSuccess) return -2;
    if (reset) {
        static const unsigned long long zero[32] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_seg), zero, sizeof(zero)) != hipSuccess) return -2;
    }
    return 0;
}
#endif

// nlp_mode 1 (one stage per lane): the QP with the KKT test, then the line search
static hipError_t launch_sqp_merit(const SolveArgs& a, int it, hipStream_t stream) {
    const hipError_t e = factor_alt(a.p, 1) ? launch_qp_waves<qp_step_kernel<1, true, true, true>, 1>(a, stream, it)
                                            : launch_qp_waves<qp_step_kernel<1, true, true, false>, 1>(a, stream, it);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(merit_ls_kernel, dim3((unsigned)waves_for(a.nI, a.p.N, 1)), dim3(WAVE), 0, stream, a);   // one wave per workgroup
    return hipGetLastError();
}

// Two parts once the batch fills the wave slots of the device (2 waves/SIMD) at least once;
// below that the waves of one launch already run side by side and splitting only adds launches.
// Measured (scripts/parts_sweep.sh, N = 20, K = 50, solves/s one part -> two parts): B = 4 096
// (1 366 waves) 226k -> 218k; B = 8 192 323k -> 361k; B = 16 384 423k -> 505k; B = 32 768
// 473k -> 509k; B = 65 536 491k -> 512k; N = 50, B = 16 384 (S = 2) 69.7k -> 74.8k; merit
// SQP (max_iter 30) B = 65 536 619k -> 672k, and at N = 10 1.42M -> 1.65M.
int sqp_parts_auto(int B, int N, int S, int cus) {
    const long waves = waves_for(B, N, S);
    return waves >= 8L * cus ? 2 : 1;   // 2 waves/SIMD x 4 SIMDs per CU: 2 048 slots on a whole MI355X
}

// One part's SQP loop on `stream`: (packing sort, QP [+ line search]) x sqp_iters over the
// instance range of `as`.  mark(): kernel-boundary events (single-part loop only).
template <class Mark>
static hipError_t sqp_iteration(const SolveArgs& as, int S, bool sorted, int it, hipStream_t stream, Mark&& mark) {
    hipError_t e = hipSuccess;
    if (sorted && it > 0) {
        hipLaunchKernelGGL(sort_by_iters_kernel, dim3((as.nI + 255) / 256), dim3(256), 0, stream, as.i0, as.nI,
                           pack_maxkey(as.p.qp_iters), as.wnit, as.wperm, as.whist, (it - 1) & 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = mark();
    if (e == hipSuccess)
        e = as.p.nlp_mode == 1 ? launch_sqp_merit(as, it, stream) : launch_qp_any(as, S, it, stream, true);
    if (e == hipSuccess) e = mark();
    return e;
}

hipError_t launch_sqp(const SolveArgs& a, int S, hipStream_t stream, hipEvent_t* ev, const SqpStreams* split) {
    if (a.p.nlp_mode == 0 && (!a.wadj || !a.wadjv)) return hipErrorInvalidValue;   // the QP kernels' adjoint record
    const int G = instances_per_wave(a.p.N, S);
    // parts of whole waves (the last part takes the remainder); at least one wave each
    int P = split ? split->parts : 1;
    if (P > SQP_MAX_PARTS) P = SQP_MAX_PARTS;
    const int wtot = (int)waves_for(a.B, a.p.N, S);
    if (P > wtot) P = wtot;
    for (int q = 1; q < P; ++q)
        if (!split->aux[q - 1] || !split->join[q - 1] || !split->fork) P = 1;
    const bool fused = split && split->fused && a.p.nlp_mode == 0 && a.wdone && (S == 1 || S == 2);
    if (fused) P = 1;
    const bool two = P > 1;
    const int K = a.p.sqp_iters;
    int ne = 0;
    auto mark = [&]() { return ev ? hipEventRecord(ev[ne++], stream) : hipSuccess; };
    auto nomark = []() { return hipSuccess; };
    const unsigned gb = (unsigned)((a.B + 127) / 128);
    hipError_t e = mark();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(prologue_kernel, dim3(gb), dim3(128), 0, stream, a);
    e = hipGetLastError();
    const bool sorted = !fused && a.wperm && a.wnit && a.whist;
    SolveArgs as = a;
    as.i0 = 0;
    as.nI = a.B;
    if (!sorted) {   // identity order: the QP kernels must not read an unsorted permutation
        as.whist = nullptr;
        as.wperm = nullptr;
    }
    if (e == hipSuccess && sorted) {
        hipLaunchKernelGGL(iota_kernel, dim3(gb), dim3(128), 0, stream, a.B, a.wperm);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemsetAsync(a.whist, 0, P * WHIST_PER_PART * sizeof(int32_t), stream);
    }
    if (e == hipSuccess) e = mark();
    if (fused) {
        if (e == hipSuccess)
            e = with_variant(as.p, S, [&](auto s, auto alt) {
                return launch_qp_waves<sqp_loop_kernel<s(), alt()>, s()>(as, stream);
            });
        ne = 2 * K + 1;
        if (e == hipSuccess) e = mark();
    } else if (!two) {
        for (int it = 0; it < K && e == hipSuccess; ++it) e = sqp_iteration(as, S, sorted, it, stream, mark);
    } else {
        // fork: the other parts wait for the prologue, then every part iterates independently
        SolveArgs ap[SQP_MAX_PARTS];
        hipStream_t sp[SQP_MAX_PARTS];
        for (int q = 0; q < P; ++q) {
            const int w0 = (int)((long)wtot * q / P), w1 = (int)((long)wtot * (q + 1) / P);
            ap[q] = as;
            ap[q].i0 = w0 * G;
            ap[q].nI = (q + 1 < P ? w1 * G : a.B) - w0 * G;
            if (sorted) ap[q].whist = a.whist + q * WHIST_PER_PART;
            sp[q] = q == 0 ? stream : split->aux[q - 1];
        }
        if (e == hipSuccess) e = hipEventRecord(split->fork, stream);
        for (int q = 1; q < P && e == hipSuccess; ++q) e = hipStreamWaitEvent(sp[q], split->fork, 0);
        for (int it = 0; it < K && e == hipSuccess; ++it)
            for (int q = 0; q < P && e == hipSuccess; ++q) e = sqp_iteration(ap[q], S, sorted, it, sp[q], nomark);
        for (int q = 1; q < P && e == hipSuccess; ++q) {
            e = hipEventRecord(split->join[q - 1], sp[q]);
            if (e == hipSuccess) e = hipStreamWaitEvent(stream, split->join[q - 1], 0);
        }
        ne = 2 * K + 1;
        if (e == hipSuccess) e = mark();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(epilogue_kernel, dim3(gb), dim3(128), 0, stream, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = mark();
    return e;
}

// One QP (qsp_qp_solve): the workspace already holds the stage data.
hipError_t launch_qp(const SolveArgs& a, int S, hipStream_t stream) {
    SolveArgs as = a;
    as.i0 = 0;
    as.nI = a.B;
    return launch_qp_any(as, S, a.p.sqp_iters - 1, stream, false);
}

// The kernels compiled for a horizon (a.p.N == qp_fixed_horizon(...) != 0).  Defined last, so these
// instantiations follow every other kernel in the code object and the others keep the places they have
// without them.
static hipError_t launch_qp_fixed(const SolveArgs& a, int it, hipStream_t stream, bool lin) {
    switch (a.p.N) {
#define QSP_FIXED_CASE(n)                                                                            \
    case n:                                                                                          \
        static_assert(mfw_fits(n, 1), "a compiled horizon takes the one-stage matrix-core variant"); \
        return lin ? launch_qp_waves<qp_step_kernel<1, false, true, true, n>, 1>(a, stream, it)      \
                   : launch_qp_waves<qp_step_kernel<1, false, false, true, n>, 1>(a, stream, it);
        QSP_FIXED_HORIZONS(QSP_FIXED_CASE)
#undef QSP_FIXED_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace qsp
