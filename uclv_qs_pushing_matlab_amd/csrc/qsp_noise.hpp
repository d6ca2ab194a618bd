// qsp_noise.hpp — sim_noise (helper.m:240-242, :154-156) drawn where it is added: a counter-based generator,
// so that the noise of (lane, step) is a pure function of the handle's generator block (SimNoiseGen,
// qsp_kernels.h) and needs no table, and every shard or chunk of a run draws the same numbers.
//
//   bits      Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11;
//             the Random123 constants), one call per (lane, step):
//                 counter = (lane0 + lane, step low word, step high word, stream),  step = step0 + t
//                 key     = (seed low word, seed high word)
//   uniforms  u_j = (w_j + 0.5) 2^-32 of the four output words: exact in double, never 0 or 1
//   normals   Box-Muller on (u0, u1) and on (u2, u3): r = sqrt(-2 log u0), z0 = r cos(2 pi u1),
//             z1 = r sin(2 pi u1); |z| <= sqrt(2 log 2^33) = 6.76, always finite
//   noise     n_c = (sigma[c] * scale_lane) * z_c, plain products: the table that sim_noise_kernel writes and
//             the value a loop kernel adds are the same bits (the build has -ffp-contract=off)
// tests/sim_noise_ref.py restates this in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "qsp_fp.hpp"
#include "qsp_kernels.h"

namespace qsp {

__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four standard normals of (lane, step t of this call)
__host__ __device__ __forceinline__ void sim_noise_normals(const SimNoiseGen& g, uint32_t lane, uint64_t t, double z[4]) {
    const uint64_t step = g.step0 + t;
    const uint32_t ctr[4] = {g.lane0 + lane, (uint32_t)step, (uint32_t)(step >> 32), g.stream};
    const uint32_t key[2] = {g.key0, g.key1};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    const double two_pi = 6.283185307179586476925;   // 2 * M_PI as a double
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
        const double u0 = ((double)w[j] + 0.5) * 0x1p-32, u1 = ((double)w[j + 1] + 0.5) * 0x1p-32;
        const double r = sqrt(-2.0 * log(u0));
        double sn, cs;
        sin_cos(two_pi * u1, &sn, &cs);
        z[j] = r * cs;
        z[j + 1] = r * sn;
    }
}

// the noise of (lane, step t of this call): n[c] is what the loop adds to x[c]
__host__ __device__ __forceinline__ void sim_noise(const SimNoiseGen& g, const double* lane_scale, int lane, int t, double n[4]) {
    double z[4];
    sim_noise_normals(g, (uint32_t)lane, (uint64_t)t, z);
    const double scale = lane_scale ? lane_scale[lane] : 1.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) n[c] = (g.sigma[c] * scale) * z[c];
}

}  // namespace qsp
