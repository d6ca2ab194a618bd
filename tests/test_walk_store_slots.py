"""Where the matrix-core factor walk's block lanes store (mfw_store_k, mfw_store_z in qsp_layout.h), read from
the header itself by a small C program: for every horizon and layout mfw_fits accepts, rows 0, 1 store to the
output slots the stage lane collects (K row-major at O_K, Z at O_Z), and rows 2, 3 to dump slots that lie inside
the record, outside the outputs O_K .. O_K + O_COUNT, and inside the instance's records of the region."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <stdio.h>
#include "qsp_layout.h"
int main(void) {
    printf("%d %d %d %d\n", MFW_REC, O_K, O_Z, O_COUNT);
    for (int S = 1; S <= 2; ++S)
        for (int N = 1; N <= 127; ++N) {
            if (!mfw_fits(N, S)) continue;
            const int G = instances_per_wave(N, S), CM = mfw_records(N);
            printf("L %d %d %d %d %d %d\n", S, N, G, CM, mfw_stride(CM, G), mfw_region(S) - C_COUNT);
            for (int r = 0; r < 4; ++r)
                for (int cc = 0; cc < 4; ++cc) printf("S %d %d %d %d\n", r, cc, mfw_store_k(r, cc), mfw_store_z(r, cc));
        }
    return 0;
}
"""


def test_dump_slots_lie_in_the_record_and_off_the_outputs(tmp_path):
    src, exe = tmp_path / "slots.c", tmp_path / "slots"
    src.write_text(PROG)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "uclv_qs_pushing_matlab_amd", "csrc"),
                           str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    REC, O_K, O_Z, O_COUNT = (int(v) for v in lines[0].split())
    layouts, slots = [], []
    for ln in lines[1:]:
        f = ln.split()
        if f and f[0] == "L":
            layouts.append(tuple(int(v) for v in f[1:]))
            slots.append({})
        elif f:
            r, cc, k, z = (int(v) for v in f[1:])
            slots[-1][r, cc] = (k, z)
    horizons = {(S, N) for S, N, *_ in layouts}
    assert {(1, N) for N in range(12, 32)} | {(2, N) for N in range(24, 128)} == horizons
    for (S, N, G, CM, IS, cap), sl in zip(layouts, slots):
        for (r, cc), (k, z) in sl.items():
            if r < 2:   # what the collect reads: K (2 x 4) at O_K, rows 0, 1 of Z at O_Z
                assert k == O_K + 4 * r + cc and z == O_Z + 4 * r + cc, (S, N, r, cc, k, z)
            else:
                for slot in (k, z):
                    assert O_K + O_COUNT <= slot < REC, (S, N, r, cc, slot)
        # one store instruction, one address per lane: no two lanes of a block on one slot
        assert len({k for k, _ in sl.values()}) == 16 and len({z for _, z in sl.values()}) == 16, (S, N)
        # the last block's last record, dump slots included, ends below the region's constants
        assert (G - 1) * IS + CM * REC <= cap, (S, N)
