// Stand-alone host check of csrc/qsp_sens.hpp (no GPU, no HIP runtime): the sensitivity walk of qsp_qp_sens'
// kernel -- sens_terminal, sens_back_step for k = N-1 .. 0, then sens_fwd_step for k = 0 .. N-1 -- per lane of
// a QP batch read from a file, every output printed in hex for tests/test_sens_host.py to compare with numpy
// and for tests/test_gpu_sens.py to compare with the device, bit for bit.
//   sens_main FILE
// FILE: int32 N, nb, pad, pad; then doubles A (nb x N x 16), B (nb x N x 8), H (nb x (6N+4)).
// Output: "sens ok", then per lane five lines: flag; K0 (8); P0 (10); K (N x 8); dU (N x 8).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qsp_sens.hpp"

static bool read_doubles(std::FILE* f, std::vector<double>& v, size_t n) {
    v.resize(n);
    return std::fread(v.data(), sizeof(double), n, f) == n;
}

static void print_row(const double* v, size_t n, bool fin) {
    for (size_t q = 0; q < n; ++q) std::printf("%a%c", fin ? v[q] : __builtin_nan(""), q + 1 == n ? '\n' : ' ');
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[4];
    if (std::fread(hdr, sizeof(int32_t), 4, f) != 4 || hdr[0] < 1 || hdr[1] < 1) return 4;
    const size_t N = (size_t)hdr[0], nb = (size_t)hdr[1];
    std::vector<double> A, B, H;
    using Q = qsp::QpLaneData;
    const bool ok = read_doubles(f, A, nb * N * Q::NA) && read_doubles(f, B, nb * N * Q::NB) && read_doubles(f, H, nb * Q::hg(N));
    std::fclose(f);
    if (!ok) return 5;
    std::printf("sens ok\n");
    std::vector<double> K(N * 8), dU(N * 8);
    for (size_t i = 0; i < nb; ++i) {
        const Q q(A.data(), B.data(), nullptr, H.data(), nullptr, nullptr, nullptr, (int)N, i);   // the kernel's view
        double P[10], a[6], Kk[8];
        bool fin = qsp::sens_terminal(q.Hk((int)N), P);
        for (int k = (int)N; k-- > 0;) {
            Q::free_entries(q.Ak(k), a);
            fin = qsp::sens_back_step(a, q.Bk(k), q.Hk(k), q.Hk(k) + 4, P, Kk) && fin;
            for (int j = 0; j < 8; ++j) K[k * 8 + j] = Kk[j];
        }
        double Phi[16];
        qsp::sens_identity(Phi);
        for (int k = 0; k < (int)N; ++k) {
            Q::free_entries(q.Ak(k), a);
            fin = qsp::sens_fwd_step(a, q.Bk(k), K.data() + k * 8, Phi, dU.data() + k * 8) && fin;
        }
        std::printf("%d\n", fin ? 0 : 1);
        print_row(K.data(), 8, fin);
        print_row(P, 10, fin);
        print_row(K.data(), N * 8, fin);
        print_row(dU.data(), N * 8, fin);
    }
    return 0;
}
