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
    const bool ok = read_doubles(f, A, nb * N * 16) && read_doubles(f, B, nb * N * 8) && read_doubles(f, H, nb * (6 * N + 4));
    std::fclose(f);
    if (!ok) return 5;
    std::printf("sens ok\n");
    std::vector<double> K(N * 8), dU(N * 8);
    for (size_t i = 0; i < nb; ++i) {
        const double* Hl = H.data() + i * (6 * N + 4);
        double P[10], a[6], Kk[8];
        bool fin = qsp::sens_terminal(Hl + 6 * N, P);
        for (size_t k = N; k-- > 0;) {
            const double* Ak = A.data() + (i * N + k) * 16;
            a[0] = Ak[2]; a[1] = Ak[3]; a[2] = Ak[6]; a[3] = Ak[7]; a[4] = Ak[11]; a[5] = Ak[15];
            fin = qsp::sens_back_step(a, B.data() + (i * N + k) * 8, Hl + 6 * k, Hl + 6 * k + 4, P, Kk) && fin;
            for (int q = 0; q < 8; ++q) K[k * 8 + q] = Kk[q];
        }
        double Phi[16];
        qsp::sens_identity(Phi);
        for (size_t k = 0; k < N; ++k) {
            const double* Ak = A.data() + (i * N + k) * 16;
            a[0] = Ak[2]; a[1] = Ak[3]; a[2] = Ak[6]; a[3] = Ak[7]; a[4] = Ak[11]; a[5] = Ak[15];
            fin = qsp::sens_fwd_step(a, B.data() + (i * N + k) * 8, K.data() + k * 8, Phi, dU.data() + k * 8) && fin;
        }
        std::printf("%d\n", fin ? 0 : 1);
        print_row(K.data(), 8, fin);
        print_row(P, 10, fin);
        print_row(K.data(), N * 8, fin);
        print_row(dU.data(), N * 8, fin);
    }
    return 0;
}
