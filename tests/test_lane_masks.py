"""The lane masks of a compiled horizon (lane_mask_* in qsp_layout.h), read from the header itself by a small
C++ program, in the manner of test_walk_store_slots.py.  The kernel compiled for a horizon takes these 64-bit
constants where the runtime-horizon kernel tests each lane; so every mask must equal the plain per-lane
predicate, written out here once more from the lane's geometry (grp = lane / L, lig = lane - grp L), on all 64
lanes -- the padding lanes behind the last whole instance included, which get what the expression gives them --
for N = 20, every horizon in QSP_FIXED_HORIZONS and the neighbouring layouts (four, three and two instances per
wave, with and without padding lanes), every walk step j and every tree level.  The rule that advances a walk's
mask from one step to the next (lane_mask_leave: the lanes lig == j, the lig == 0 mask shifted by j, leave) is checked over the steps the
walks take."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uclv_qs_pushing_matlab_amd", "csrc")

PROG = r"""
#include <cstdio>
#include "qsp_layout.h"
using namespace qsp;
static int bad = 0;
template <class F>
static void check(const char* what, int N, int a, lane_mask_t m, F pred) {
    for (int lane = 0; lane < 64; ++lane) {
        const bool want = pred(lane), got = (m >> lane) & 1;
        if (want != got) {
            std::printf("MISMATCH %s N %d arg %d lane %d: mask %d predicate %d\n", what, N, a, lane, (int)got, (int)want);
            ++bad;
        }
    }
}
static void horizon(int N) {
    const int S = 1, L = lanes_per_instance(N, S), G = WAVE / L, H = mfw_split(N);
    auto grp = [=](int lane) { return lane / L; };
    auto lig = [=](int lane) { return lane - lane / L * L; };
    for (int j = 0; j < L; ++j) {
        check("lig <= j", N, j, lane_mask_lig_le(N, S, j), [=](int l) { return lig(l) <= j; });
        check("lig == j", N, j, lane_mask_lig_eq(N, S, j), [=](int l) { return lig(l) == j; });
        check("j <= lig < L-1", N, j, lane_mask_walk_fwd(N, S, j), [=](int l) { return lig(l) >= j && lig(l) < L - 1; });
    }
    for (int off = 1; off < 64; off <<= 1)
        check("lig + off < L", N, off, lane_mask_tree(N, S, off), [=](int l) { return lig(l) + off < L; });
    check("lig == 0", N, 0, lane_mask_first(N, S), [=](int l) { return lig(l) == 0; });
    check("lig < N", N, 0, lane_mask_stage(N, S), [=](int l) { return lig(l) < N; });
    check("grp < G", N, 0, lane_mask_instances(N, S), [=](int l) { return grp(l) < G; });
    for (int i = 0; i < SCAN_FLAGS; ++i)
        check("scan flag", N, i, lane_mask_scan(N, S, i), [=](int lane) {
            const int base = grp(lane) * L, lg = lane - base, col = lane & 15, row = lane >> 4;   // GroupScan::init
            const bool f[6] = {col >= 1 && lg >= 1, col >= 2 && lg >= 2, col >= 4 && lg >= 4, col >= 8 && lg >= 8,
                               (row & 1) && lg > col, row >= 2 && lg >= lane - 31};
            return f[i];
        });
    for (int ph = 0; ph < 2; ++ph) {
        const int kb = ph == 0 ? H : 0, ke = ph == 0 ? N : H - 1;
        check("publish", N, ph, lane_mask_mfw_publish(N, ph), [=](int l) { return grp(l) < G && lig(l) >= kb && lig(l) <= ke; });
        check("collect", N, ph, lane_mask_mfw_collect(N, ph),
              [=](int l) { return grp(l) < G && lig(l) >= kb && lig(l) <= ke && lig(l) < N; });
    }
    // the scalar rule, over the steps the walks take: backward j = L-2 .. 1 from lig <= L-2, forward
    // j = 0 .. L-2 from 0 <= lig < L-1
    const lane_mask_t first = lane_mask_first(N, S);
    lane_mask_t act = lane_mask_lig_le(N, S, L - 2);
    for (int j = L - 2; j >= 1; --j) {
        if (act != lane_mask_lig_le(N, S, j)) { std::printf("MISMATCH backward rule N %d step %d\n", N, j); ++bad; }
        act = lane_mask_leave(act, first, j);
    }
    if (act != first) { std::printf("MISMATCH backward rule N %d: lanes left after the last step\n", N); ++bad; }
    act = lane_mask_walk_fwd(N, S, 0);
    for (int j = 0; j < L - 1; ++j) {
        if (act != lane_mask_walk_fwd(N, S, j)) { std::printf("MISMATCH forward rule N %d step %d\n", N, j); ++bad; }
        act = lane_mask_leave(act, first, j);
    }
    if (act != 0) { std::printf("MISMATCH forward rule N %d: lanes left after the last step\n", N); ++bad; }
    std::printf("HORIZON %d L %d G %d\n", N, L, G);
}
// the factor walk's block lanes: element (r, cc) = (lane >> 4, lane & 3), every set of rows and of columns
static void roles() {
    for (int rows = 0; rows < 16; ++rows)
        for (int cols = 0; cols < 16; ++cols)
            check("rows x cols", rows, cols, lane_mask_mfw_role(rows, cols),
                  [=](int l) { return ((rows >> (l >> 4)) & 1) && ((cols >> (l & 3)) & 1); });
    check("r == cc", 0, 0, lane_mask_mfw_diag(), [](int l) { return (l >> 4) == (l & 3); });
    check("r <= cc", 0, 0, lane_mask_mfw_upper(), [](int l) { return (l >> 4) <= (l & 3); });
}
int main(int argc, char** argv) {
    roles();
    for (int i = 1; i < argc; ++i) horizon(std::atoi(argv[i]));
    return bad != 0;
}
"""


def fixed_horizons():
    with open(os.path.join(CSRC, "qsp_solver.hip")) as fh:
        m = re.search(r"^#define QSP_FIXED_HORIZONS\(X\)(.*)$", fh.read(), re.M)
    return [int(v) for v in re.findall(r"X\((\d+)\)", m.group(1))]


def test_fixed_horizons_are_read():
    assert 20 in fixed_horizons()


def test_masks_equal_the_per_lane_predicates(tmp_path):
    src, exe = tmp_path / "masks.cpp", tmp_path / "masks"
    src.write_text(PROG)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    # the compiled horizons; the one-stage-per-lane layouts at their edges: L = 13 (G = 4, 12 padding lanes),
    # 16 (G = 4, none), 17 and 21 (G = 3), 22 and 32 (G = 2, 20 padding lanes and none)
    horizons = sorted({20, *fixed_horizons(), 12, 15, 16, 19, 21, 31})
    r = subprocess.run([str(exe)] + [str(n) for n in horizons], capture_output=True, text=True)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-4000:]
    assert [int(ln.split()[1]) for ln in r.stdout.splitlines() if ln.startswith("HORIZON")] == horizons


def test_masks_are_constants_of_the_build(tmp_path):
    """The kernel takes the masks as template arguments: each must be a constant expression (C++17 constexpr
    when the header is read with the device compiler's marking), here for the headline horizon's values."""
    src = tmp_path / "cexpr.cpp"
    src.write_text(r"""
#define __HIPCC__ 1
#define __host__
#define __device__
#include "qsp_layout.h"
using namespace qsp;
static_assert(lane_mask_lig_eq(20, 1, 0) == ((1ull << 0) | (1ull << 21) | (1ull << 42) | (1ull << 63)), "lig == 0 at N = 20");
static_assert(lane_mask_instances(20, 1) == (1ull << 63) - 1, "three instances of 21 lanes, one padding lane");
static_assert(lane_mask_lig_le(20, 1, 19) == ~((1ull << 20) | (1ull << 41) | (1ull << 62)), "all but the terminal lanes");
static_assert(lane_mask_walk_fwd(20, 1, 0) == lane_mask_lig_le(20, 1, 19), "no terminal lane steps forward");
static_assert(lane_mask_stage(20, 1) == lane_mask_lig_le(20, 1, 19), "lig < N");
static_assert(lane_mask_tree(20, 1, 16) == ((0x1full << 0) | (0x1full << 21) | (0x1full << 42) | (1ull << 63)), "lig + 16 < 21");
int main() { return 0; }
""")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)])
