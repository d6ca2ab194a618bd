/* qsp_layout.h — the QP kernels' layout rules, in one place: how instances map onto wavefronts,
 * how many stages a lane holds, the LDS fields of a lane, which horizons factorise on the
 * matrix cores and which factorisation a handle takes.  Plain integer arithmetic that compiles as C99 and
 * as HIP C++ (host and device) -- with one exception, mfma_walk_default at the end: a host-only read of an
 * environment variable (hence <stdlib.h>), here because the library and the twin must read it alike:
 * qsp_solver.hip and qsp_capi.hip include it, and so does the CPU twin that checks the kernels bit
 * for bit (test infrastructure may read a product header; the product never reads the twin).  The
 * twin reads four more on the same terms, C++ only: qsp_fp.hpp, qsp_math.hpp, qsp_riccati.hpp and
 * qsp_ipm.hpp, the lane-local arithmetic. */
#ifndef QSP_LAYOUT_H
#define QSP_LAYOUT_H
#include <stdlib.h>

#ifdef __HIPCC__
#define QSP_LAYOUT_FN __host__ __device__ constexpr
#else
#define QSP_LAYOUT_FN static inline
#endif

#ifdef __cplusplus
namespace qsp {
#endif

/* ------------------------------------------------------------------ instances on wavefronts
 * One instance owns L = ceil((N + 1) / S) consecutive lanes of a wavefront (S stages per lane);
 * a wavefront holds G = 64 / L whole instances and every QP workgroup is one wavefront. */
enum { WAVE = 64 };
QSP_LAYOUT_FN int lanes_per_instance(int N, int S) { return (N + S) / S; }
QSP_LAYOUT_FN int instances_per_wave(int N, int S) { return WAVE / lanes_per_instance(N, S); }
QSP_LAYOUT_FN long waves_for(long nI, int N, int S) {
    return (nI + instances_per_wave(N, S) - 1) / instances_per_wave(N, S);
}

/* Stages per lane of a handle: the explicit request, else one for nlp_mode 1 (its kernels exist at
 * one stage per lane only), else by the horizon.  One stage per lane keeps the QP kernel at
 * 2 waves/SIMD with its closed-loop walks and wins while a wavefront still holds two or more
 * instances; once one stage per lane leaves a single instance per wave (N + 1 > 32), two stages
 * per lane (1 wave/SIMD, 2-3 instances per wave) win.  scripts/layout_sweep.sh, round 1 (one-wave
 * workgroups): N = 10 1.32M vs 1.17M, N = 20 493k vs 422k, N = 50 (B = 16 384) 62.6k vs 70.0k
 * solves/s for S = 1 vs 2. */
QSP_LAYOUT_FN int stages_per_lane(int N, int nlp_mode, int requested) {
    return requested > 0 ? requested : (nlp_mode == 1 || N + 1 <= 32 ? 1 : 2);
}

/* ------------------------------------------------------------------ a lane's LDS column
 * Registers hold what the horizon recursions read on every step (stage model, gradient, Riccati
 * factors); LDS holds what only the stage-parallel phases touch (iterate, slacks/multipliers,
 * barrier terms, QP solution pieces): per stage slot the fields below, WAVE doubles each. */
enum LdsField {
    F_T = 0,      /* 6  slacks        s_lo s_hi un_lo un_hi ut_lo ut_hi */
    F_LM = 6,     /* 6  multipliers */
    F_V = 12,     /* 3  bounded components of the SQP iterate (s_k, u_n, u_t) */
    F_DU = 15,    /* 2  damped QP control step */
    F_RT = 17,    /* 6  1 / slack, refreshed whenever the slacks change */
    F_VA = 23,    /* 3  affine-predictor bounded components (ds, dun, dut) */
    F_VN = 26,    /* 3  corrector bounded components */
    F_DX = 23,    /* 4  final QP state step (written after the IPM: aliases F_VA / F_VN) */
    F_HG = 29,    /* 6  the corrector's barrier gradient additions (3..5); 0..2 unused (the predictor's
                   *    barrier terms go to the factorisation in registers) */
    F_COUNT = 35
};

/* ------------------------------------------------------------------ the matrix-core factor walk
 * Its stage records overlay F_VA .. F_HG of every slot (free while the predictor factorises) and
 * mfw_extra(S) more fields at the end of the workgroup's LDS (factor_walk_mfma in qsp_solver.hip).
 * A record, row-major in the order the block lanes read it: */
enum MfwSlot { R_G = 0, R_A = 12, R_GX = 18, R_HX3 = 22, R_HU = 23, R_GU = 25, MFW_REC = 27 };
enum MfwOut { O_K = 0, O_Z = 8, O_COUNT = 16 };   /* K (2 x 4), rows 0, 1 of Z = [R~ | r~ | .] */
/* Where the block lane of matrix row r, column cc stores its element of K and of Z in its stage's record.
 * Rows 0, 1 hold the outputs and store them to their slots.  Rows 2, 3 hold nothing the stage lane collects;
 * at one stage per lane they store too, so that the step's stores run on the whole wave without a change of
 * the exec mask, to dump slots O_COUNT .. O_COUNT + 7: operand slots of the same record, which the walk read
 * one step ahead and reads never again, and which the record's next publish rewrites with the rest of it. */
QSP_LAYOUT_FN int mfw_store_k(int r, int cc) { return r < 2 ? O_K + 4 * r + cc : O_COUNT + 4 * (r - 2) + cc; }
QSP_LAYOUT_FN int mfw_store_z(int r, int cc) { return r < 2 ? O_Z + 4 * r + cc : O_COUNT + 4 * (r - 2) + cc; }
/* the operand constants (A's ones and zeros, the zero column of [B | b | 0], Hx's fixed diagonal),
 * at the end of the region */
enum MfwConst { C_ONE = 0, C_ZERO = 1, C_HX = 2, C_COUNT = 5 };

/* One stage per lane: two extra fields, 18 944 bytes per workgroup, so eight one-wave workgroups and
 * a packing-sort workgroup still share a CU's LDS.  Two stages per lane: four, 37 888 bytes per
 * workgroup -- three (1 728 doubles of records) are too few for the stride padding between
 * the instances' records at N = 30, 31 (1 757 doubles) and N = 62, 63 (1 739), and for the five
 * constants behind the 64 records of one instance at N = 126, 127 (1 733). */
QSP_LAYOUT_FN int mfw_extra(int S) { return S == 1 ? 2 : 4; }
QSP_LAYOUT_FN int lds_doubles(int S) { return (F_COUNT * S + mfw_extra(S)) * WAVE; }
/* LDS doubles the stage records may occupy: F_VA .. F_HG of every slot plus the extra fields. */
QSP_LAYOUT_FN int mfw_region(int S) { return ((F_COUNT - F_VA) * S + mfw_extra(S)) * WAVE; }
/* The records of a wave's instances do not fit at once: the walk runs in two phases, stages
 * H .. N - 1 with the terminal record, then 0 .. H - 1; CM records per instance and phase. */
QSP_LAYOUT_FN int mfw_split(int N) { return (N + 1) / 2; }
QSP_LAYOUT_FN int mfw_records(int N) { return N + 1 - mfw_split(N); }
/* The instances' record regions start IS doubles apart, IS >= CM records: a stride whose multiples
 * put the instances' reads of one operand (at most six consecutive doubles per half wave) on
 * disjoint LDS banks (32 doubles): 9 ... 11 or 21 ... 23 mod 32 for three instances, 8 or 24 for
 * four, 6 ... 26 for two. */
QSP_LAYOUT_FN int mfw_stride(int CM, int G) {
    int is = CM * MFW_REC;
    for (;; ++is) {
        const int m = is & 31;
        if (G <= 1 || (G == 2 && m >= 6 && m <= 26) || (G == 3 && ((m >= 9 && m <= 11) || (m >= 21 && m <= 23))) ||
            (G >= 4 && (m == 8 || m == 24)))
            return is;
    }
}
/* Which horizons factorise on the matrix cores: one instance per 16-lane block (G <= 4: at one
 * stage per lane N >= 12, at two N >= 24) and the records of a phase in the region.  That is
 * N = 12 .. 31 at one stage per lane and N = 24 .. 127 at two, narrowly: one stage per lane at
 * N = 20 fills 896 of 896 doubles, two at N = 30, 31 use 1757 of 1792 (tests/test_twin.py pins
 * the table). */
QSP_LAYOUT_FN int mfw_fits(int N, int S) {
    const int G = instances_per_wave(N, S), CM = mfw_records(N);
    return G <= 4 && (G - 1) * mfw_stride(CM, G) + CM * MFW_REC + C_COUNT <= mfw_region(S) && (S == 2 || N <= 31);
}
/* The factorisation a handle's QP kernels take, in the public QSP_WALK_* coding (qsp_nmpc.h): at two
 * stages per lane the associative scan where factor_scan asks for it, else the matrix cores where
 * mfma_walk allows them and the records fit, else the lane walk.  The kernels' launchers select by it
 * (factor_alt, qsp_solver.hip) and the twin emulates what it names. */
enum FactorWalk { WALK_LANE = 0, WALK_MFMA = 1, WALK_SCAN = 2 };
QSP_LAYOUT_FN int factor_walk_of(int N, int S, int mfma_walk, int factor_scan) {
    return (S != 1 && S != 2) ? WALK_LANE : (S == 2 && factor_scan) ? WALK_SCAN
         : (mfma_walk && mfw_fits(N, S)) ? WALK_MFMA : WALK_LANE;
}
/* ------------------------------------------------------------------ lane masks
 * Which lanes of a wavefront pass each geometric test of the QP kernels, as a 64-bit mask (bit l: lane l).
 * Where the horizon is compiled in, the kernel takes these constants as scalar exec masks instead of
 * comparing per lane.  Every mask restates today's per-lane expression with lig = lane - (lane / L) L, on
 * the padding lanes behind the last whole instance (lane / L == G) as well: they get what the
 * expression gives them.  tests/test_lane_masks.py compares each with its predicate on all 64 lanes. */
typedef unsigned long long lane_mask_t;
/* lo <= lig <= hi */
QSP_LAYOUT_FN lane_mask_t lane_mask_lig_in(int N, int S, int lo, int hi) {
    lane_mask_t m = 0;
    for (int l = 0; l < WAVE; ++l) {
        const int lig = l % lanes_per_instance(N, S);
        if (lig >= lo && lig <= hi) m |= 1ull << l;
    }
    return m;
}
QSP_LAYOUT_FN lane_mask_t lane_mask_lig_eq(int N, int S, int j) { return lane_mask_lig_in(N, S, j, j); }
/* the backward lane walks' step j: lig <= j */
QSP_LAYOUT_FN lane_mask_t lane_mask_lig_le(int N, int S, int j) { return lane_mask_lig_in(N, S, 0, j); }
/* the forward lane walks' step j: j <= lig < L - 1 */
QSP_LAYOUT_FN lane_mask_t lane_mask_walk_fwd(int N, int S, int j) {
    return lane_mask_lig_in(N, S, j, lanes_per_instance(N, S) - 2);
}
/* From one step of a walk to the next the lanes with lig == j leave: mask(j -+ 1) = mask(j) & ~eq(j), and
 * eq(j) = eq(0) << j for j <= L - 1 (a group's bit stays inside the group; the padding lanes' falls off the
 * wave where they have no such lane) -- two scalar operations per step, none where j is a constant. */
QSP_LAYOUT_FN lane_mask_t lane_mask_leave(lane_mask_t m, lane_mask_t first, int j) { return m & ~(first << j); }
/* the sum tree's level off: lig + off < L */
QSP_LAYOUT_FN lane_mask_t lane_mask_tree(int N, int S, int off) {
    return lane_mask_lig_in(N, S, 0, lanes_per_instance(N, S) - 1 - off);
}
/* stage roles at one stage per lane: lig == 0; lig < N (a stage with a control) */
QSP_LAYOUT_FN lane_mask_t lane_mask_first(int N, int S) { return lane_mask_lig_eq(N, S, 0); }
QSP_LAYOUT_FN lane_mask_t lane_mask_stage(int N, int S) { return lane_mask_lig_in(N, S, 0, N - 1); }
/* the lanes of the wave's whole instances: lane / L < G */
QSP_LAYOUT_FN lane_mask_t lane_mask_instances(int N, int S) {
    const int n = instances_per_wave(N, S) * lanes_per_instance(N, S);
    return n >= WAVE ? ~0ull : (1ull << n) - 1;
}
/* GroupScan's flags (qsp_solver.hip), i = 0 .. 5: the row shifts by 1, 2, 4, 8 and the row broadcasts of
 * lanes 15 and 31, each taken where the source lane lies in the same group */
enum { SCAN_FLAGS = 6 };
QSP_LAYOUT_FN lane_mask_t lane_mask_scan(int N, int S, int i) {
    lane_mask_t m = 0;
    for (int l = 0; l < WAVE; ++l) {
        const int lig = l % lanes_per_instance(N, S), col = l & 15, row = l >> 4;
        const int take = i < 4 ? (col >= (1 << i) && lig >= (1 << i))
                       : i == 4 ? ((row & 1) && lig > col) : (row >= 2 && lig >= l - 31);
        if (take) m |= 1ull << l;
    }
    return m;
}
/* the factor walk's phase ph at one stage per lane: the stage lanes that publish a record (stages kb .. ke
 * of the whole instances), and those that collect factors from it (the stages k < N among them) */
QSP_LAYOUT_FN lane_mask_t lane_mask_mfw_publish(int N, int ph) {
    const int H = mfw_split(N);
    return lane_mask_lig_in(N, 1, ph == 0 ? H : 0, ph == 0 ? N : H - 1) & lane_mask_instances(N, 1);
}
QSP_LAYOUT_FN lane_mask_t lane_mask_mfw_collect(int N, int ph) {
    return lane_mask_mfw_publish(N, ph) & lane_mask_stage(N, 1);
}
/* the factor walk's block lanes: lane l holds element (r, cc) = (l >> 4, l & 3) of its block's 4 x 4 operands.
 * Roles by matrix row and column (rows, cols: bit sets of the rows and the columns that take the role), the
 * diagonal r == cc and the upper triangle r <= cc */
QSP_LAYOUT_FN lane_mask_t lane_mask_mfw_role(int rows, int cols) {
    lane_mask_t m = 0;
    for (int l = 0; l < WAVE; ++l)
        if (((rows >> (l >> 4)) & 1) && ((cols >> (l & 3)) & 1)) m |= 1ull << l;
    return m;
}
QSP_LAYOUT_FN lane_mask_t lane_mask_mfw_diag(void) {
    return lane_mask_mfw_role(1, 1) | lane_mask_mfw_role(2, 2) | lane_mask_mfw_role(4, 4) | lane_mask_mfw_role(8, 8);
}
QSP_LAYOUT_FN lane_mask_t lane_mask_mfw_upper(void) {
    return lane_mask_mfw_role(1, 0xf) | lane_mask_mfw_role(2, 0xe) | lane_mask_mfw_role(4, 0xc) | lane_mask_mfw_role(8, 8);
}

/* SolveParams::mfma_walk of a new handle (host): on, unless the developer switch QSP_MFMA_WALK=0
 * selects the lane walk wherever the matrix cores would factorise (an A/B that rounds differently) */
static inline int mfma_walk_default(void) {
    const char *mw = getenv("QSP_MFMA_WALK");
    return !(mw && mw[0] == '0');
}

#ifdef __cplusplus
}  /* namespace qsp */
#endif
#endif
