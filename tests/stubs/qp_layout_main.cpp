// Stand-alone host check of QpLaneData::has_structure / free_entries (csrc/qsp_point.hpp; no GPU) for
// tests/test_qp_layout_host.py.  A: pack_lin's (qsp_math.hpp) full 4 x 4 of a = {11 .. 16}.  Output: "layout ok",
// has_structure(A) and free_entries(A), then per position p = 0 .. 15: p, has_structure of A with 0.5 added at
// p, of A with a NaN at p, and free_entries of the first.
#include <cstdio>

#include "qsp_point.hpp"

int main() {
    qsp::Lin L = {};
    for (int q = 0; q < 6; ++q) L.a[q] = 11.0 + q;
    double xn[4], A[16], B[8], a[6];
    qsp::pack_lin(L, xn, A, B);
    std::printf("layout ok\n");
    qsp::QpLaneData::free_entries(A, a);
    std::printf("%d %g %g %g %g %g %g\n", qsp::QpLaneData::has_structure(A) ? 1 : 0, a[0], a[1], a[2], a[3], a[4], a[5]);
    for (int p = 0; p < 16; ++p) {
        double Ap[16], An[16];
        for (int q = 0; q < 16; ++q) Ap[q] = An[q] = A[q];
        Ap[p] += 0.5;
        An[p] = __builtin_nan("");
        qsp::QpLaneData::free_entries(Ap, a);
        std::printf("%d %d %d %g %g %g %g %g %g\n", p, qsp::QpLaneData::has_structure(Ap) ? 1 : 0,
                    qsp::QpLaneData::has_structure(An) ? 1 : 0, a[0], a[1], a[2], a[3], a[4], a[5]);
    }
    return 0;
}
