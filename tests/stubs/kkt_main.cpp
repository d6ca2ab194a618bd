// Stand-alone host check of csrc/qsp_kkt.hpp (no GPU, no HIP runtime): kkt_qp_stage, the function the kernel
// of qsp_qp_residuals runs per (lane, stage), folded over the stages of each lane of a QP batch read from a
// file, and the six per-lane maxima printed in hex for tests/test_kkt_host.py to compare with numpy.
//   kkt_main FILE
// FILE: int32 N, nb, stage0_s_bound, pad; then doubles A (nb x N x 16), B (nb x N x 8), b (nb x N x 4),
// H, g (nb x (6N+4)), lo, hi (nb x N x 3), dx0 (nb x 4), dx (nb x (N+1) x 4), du (nb x N x 2), pi (nb x N x 4),
// lam (nb x N x 6).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qsp_kkt.hpp"

static bool read_doubles(std::FILE* f, std::vector<double>& v, size_t n) {
    v.resize(n);
    return std::fread(v.data(), sizeof(double), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[4];
    if (std::fread(hdr, sizeof(int32_t), 4, f) != 4 || hdr[0] < 1 || hdr[1] < 1) return 4;
    const size_t N = (size_t)hdr[0], nb = (size_t)hdr[1];
    const int s0 = hdr[2];
    std::vector<double> A, B, b, H, g, lo, hi, dx0, dx, du, pi, lam;
    using Q = qsp::QpLaneData;
    const bool ok = read_doubles(f, A, nb * N * Q::NA) && read_doubles(f, B, nb * N * Q::NB) && read_doubles(f, b, nb * N * Q::Nb) &&
                    read_doubles(f, H, nb * Q::hg(N)) && read_doubles(f, g, nb * Q::hg(N)) &&
                    read_doubles(f, lo, nb * N * Q::NBOUND) && read_doubles(f, hi, nb * N * Q::NBOUND) && read_doubles(f, dx0, nb * 4) &&
                    read_doubles(f, dx, nb * (N + 1) * 4) && read_doubles(f, du, nb * N * 2) &&
                    read_doubles(f, pi, nb * N * 4) && read_doubles(f, lam, nb * N * 6);
    std::fclose(f);
    if (!ok) return 5;
    std::printf("kkt ok\n");
    const qsp::PointIn pt = {nullptr, 0, nullptr, dx0.data(), dx.data(), du.data(), pi.data(), lam.data(), nullptr, nullptr};
    for (size_t i = 0; i < nb; ++i) {
        double lane[qsp::KKT_QP_NRES] = {0, 0, 0, 0, 0, 0};
        bool fin = true;
        const qsp::QpLaneData q(A.data(), B.data(), b.data(), H.data(), g.data(), lo.data(), hi.data(), (int)N, i);
        for (int kk = 0; kk <= (int)N; ++kk) {   // the kernel's own views (qsp_point.hpp) do the indexing
            double res[qsp::KKT_QP_NRES];
            const qsp::PointRows r(pt, (int)N, i, kk);
            const bool sf = qsp::kkt_qp_stage((int)N, s0, kk, q.Ak(kk), q.Bk(kk), q.bk(kk), q.Hk(kk), q.gk(kk), q.lok(kk), q.hik(kk),
                                              r.x0, r.x, r.u, r.x1, r.pi, r.pip, r.lam, res);
            qsp::kkt_fold(qsp::KKT_QP_NRES, res, sf, lane, fin);
        }
        for (int q = 0; q < qsp::KKT_QP_NRES; ++q) std::printf("%a%c", fin ? lane[q] : __builtin_nan(""), q == 5 ? '\n' : ' ');
    }
    return 0;
}
