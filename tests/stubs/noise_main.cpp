// Stand-alone host check of csrc/qsp_noise.hpp (no GPU, no HIP runtime): the header's Philox4x32-10 against the
// published known answers, and the noise of a small generator printed for tests/test_sim_noise_host.py to
// compare with the numpy restatement.  The functions are __host__ __device__: this is the code the kernels run.
//   noise_main SEED STREAM STEP_OFFSET LANE_OFFSET N_STEPS B   (sigma 1, 2, 3, 4; scale of lane i = i mod 3)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "qsp_noise.hpp"

static int kat(const uint32_t c[4], const uint32_t k[2], const uint32_t want[4]) {
    uint32_t out[4];
    qsp::philox4x32_10(c, k, out);
    int bad = 0;
    for (int j = 0; j < 4; ++j) bad += out[j] != want[j];
    if (bad) std::printf("FAIL philox: %08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
    return bad;
}

int main(int argc, char** argv) {
    const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0}, w0[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
    const uint32_t c1[4] = {~0u, ~0u, ~0u, ~0u}, k1[2] = {~0u, ~0u}, w1[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
    const uint32_t c2[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k2[2] = {0xa4093822u, 0x299f31d0u},
                   w2[4] = {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u};
    if (kat(c0, k0, w0) + kat(c1, k1, w1) + kat(c2, k2, w2)) return 1;
    if (argc != 7) return 2;
    const unsigned long long seed = std::strtoull(argv[1], nullptr, 0);
    qsp::SimNoiseGen g = {};
    g.on = 1;
    g.stream = (uint32_t)std::strtoull(argv[2], nullptr, 0);
    g.key0 = (uint32_t)seed;
    g.key1 = (uint32_t)(seed >> 32);
    g.step0 = std::strtoull(argv[3], nullptr, 0);
    g.lane0 = (uint32_t)std::strtoull(argv[4], nullptr, 0);
    const int n_steps = std::atoi(argv[5]), B = std::atoi(argv[6]);
    for (int c = 0; c < 4; ++c) g.sigma[c] = 1.0 + c;
    std::vector<double> scale((size_t)B);
    for (int i = 0; i < B; ++i) scale[i] = i % 3;
    std::printf("noise ok\n");
    for (int t = 0; t < n_steps; ++t)
        for (int i = 0; i < B; ++i) {
            double n[4];
            qsp::sim_noise(g, scale.data(), i, t, n);
            std::printf("%a %a %a %a\n", n[0], n[1], n[2], n[3]);
        }
    return 0;
}
