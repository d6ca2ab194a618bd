// Stand-alone check of csrc/qsp_devbuf.hpp (no GPU, no HIP runtime): Dev<T> over counting stand-ins for the
// four HIP calls it makes, here on malloc, and Dims against the shapes written out from the comments of
// SolveArgs / ClosedLoopArgs / OpenLoopArgs.  Built with the address and undefined-behaviour sanitizers by
// tests/test_devbuf.py, so a copy past a capacity or a leaked or doubly freed allocation ends the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "qsp_devbuf.hpp"

static std::set<void*> g_live;
static int g_mallocs = 0, g_frees = 0, g_copies = 0, g_fills = 0, g_fail_next = 0;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_fail_next > 0) {
        --g_fail_next;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    ++g_mallocs;
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    if (!g_live.erase(p)) {
        std::printf("FAIL: hipFree of a pointer that is not live\n");
        std::exit(1);
    }
    std::free(p);
    ++g_frees;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) {
    std::memcpy(dst, src, bytes);
    ++g_copies;
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) {
    std::memset(dst, value, bytes);
    ++g_fills;
    return hipSuccess;
}
}

static int g_bad = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_bad;                                                       \
        }                                                                  \
    } while (0)

using qsp::Dev;
using qsp::Dims;

static void test_ensure() {
    const int f0 = g_frees, m0 = g_mallocs;
    {
        Dev<double> b;
        CHECK(b.data() == nullptr && b.count() == 0);
        CHECK(b.ensure(0) == hipSuccess && b.data() == nullptr && g_mallocs == m0);
        CHECK(b.ensure(10) == hipSuccess && b.count() == 10 && g_mallocs == m0 + 1);
        double* p = b.data();
        CHECK(b.ensure(10) == hipSuccess && b.data() == p && b.count() == 10);   // equal: kept
        CHECK(b.ensure(3) == hipSuccess && b.data() == p && b.count() == 10);    // smaller: kept
        CHECK(g_mallocs == m0 + 1 && g_frees == f0);
        CHECK(b.ensure(11) == hipSuccess && b.count() == 11);                    // larger: replaced ...
        CHECK(g_mallocs == m0 + 2 && g_frees == f0 + 1);                         // ... with exactly one free
        CHECK(g_live.size() == 1 && g_live.count(b.data()) == 1);
    }
    CHECK(g_live.empty() && g_frees == f0 + 2);
}

struct Several {
    Dev<double> a, b;
    Dev<int32_t> c;
    Dev<uint8_t> d[3];
    Dev<qsp::ShapeDev> e;
};

static void test_destructors() {
    {
        Several s;   // destroyed part-filled
        CHECK(s.a.ensure(7) == hipSuccess && s.c.ensure(5) == hipSuccess && s.d[1].ensure(33) == hipSuccess);
        CHECK(s.e.ensure(2) == hipSuccess);
        CHECK(g_live.size() == 4);
    }
    CHECK(g_live.empty());
    const int f0 = g_frees;
    {
        Dev<int32_t> never;   // never allocated: nothing to free
    }
    CHECK(g_frees == f0 && g_live.empty());
    {
        Dev<double> b;
        CHECK(b.ensure(4) == hipSuccess);
        g_fail_next = 1;      // the allocation that replaces it fails once: the old one is gone, nothing is held
        CHECK(b.ensure(8) == hipErrorOutOfMemory);
        CHECK(b.data() == nullptr && b.count() == 0 && g_live.empty());
        double h[4] = {1, 2, 3, 4};
        CHECK(b.upload(nullptr, h, 4) == hipErrorInvalidValue);
        CHECK(b.ensure(8) == hipSuccess && b.count() == 8);   // and the buffer is usable again
    }
    CHECK(g_live.empty());
    {
        Dev<double> b;
        g_fail_next = 1;      // the first allocation fails: destroyed empty
        CHECK(b.ensure(8) == hipErrorOutOfMemory && b.data() == nullptr && b.count() == 0);
    }
    CHECK(g_live.empty() && g_fail_next == 0);
}

static void test_capacity() {
    Dev<double> b;
    CHECK(b.ensure(4) == hipSuccess);
    double in[8] = {1, 2, 3, 4, 5, 6, 7, 8}, out[8] = {0};
    const int c0 = g_copies, s0 = g_fills;
    CHECK(b.upload(nullptr, in, 5) == hipErrorInvalidValue);     // above the capacity: an error, nothing touched
    CHECK(b.download(nullptr, out, 5) == hipErrorInvalidValue);
    CHECK(b.fill(nullptr, 0xff, 5) == hipErrorInvalidValue);
    CHECK(g_copies == c0 && g_fills == s0 && out[0] == 0.0);
    CHECK(b.upload(nullptr, in, 4) == hipSuccess && b.download(nullptr, out, 4) == hipSuccess);
    CHECK(std::memcmp(in, out, 4 * sizeof(double)) == 0 && out[4] == 0.0);
    CHECK(b.fill(nullptr, 0, 2) == hipSuccess && b.download(nullptr, out, 3) == hipSuccess);
    CHECK(out[0] == 0.0 && out[1] == 0.0 && out[2] == 3.0);
    CHECK(g_copies == c0 + 3 && g_fills == s0 + 1);
    Dev<int32_t> empty;
    int32_t w = 7;
    CHECK(empty.upload(nullptr, &w, 1) == hipErrorInvalidValue && empty.fill(nullptr, 0, 1) == hipErrorInvalidValue);
}

// the numbers written out from the comments of qsp_kernels.h at (B, N)
static void test_dims(size_t B, size_t N) {
    const Dims d{B, N};
    const size_t T = 7, D = 3, M = 5;
    CHECK(d.lane() == B);
    CHECK(d.x0() == 4 * B && d.res() == 4 * B && d.yref_e() == 4 * B && d.u0() == 2 * B);
    CHECK(d.X() == 4 * B * (N + 1) && d.U() == 2 * B * N && d.PI() == 4 * B * N);
    CHECK(d.yref() == 6 * B * N && d.lam() == 6 * B * N);
    CHECK(d.stages() == B * (N + 1));
    CHECK(d.lin() == 24 * B * (N + 1) && d.nlp() == 20 * B * (N + 1) && d.qp() == 16 * B * (N + 1));
    CHECK(d.adj() == 11 * B * N);
    CHECK(qsp::WHIST_PER_PART == 4 * 1024 && Dims::hist() == 2 * 4 * 1024);
    CHECK(d.cl_X(T) == B * (T + 1) * 4 && d.cl_Xsim(T) == B * T * 4 && d.cl_U(T) == B * T * 2);
    CHECK(d.cl_status(T) == B * T && d.cl_noise(T) == T * B * 4 && d.metrics() == B * 10);
    CHECK(d.delay(D) == B * D * 2 && d.ring(D, M) == D * B * M);
    CHECK(Dims::traj(T) == T * 6 && d.traj_lanes(T) == B * T * 6);
}

int main() {
    test_ensure();
    test_destructors();
    test_capacity();
    test_dims(5, 10);
    test_dims(3, 32);
    CHECK(qsp::L_A == 0 && qsp::L_B == 6 && qsp::L_BB == 14 && qsp::L_G == 18 && qsp::L_COUNT == 24);
    CHECK(qsp::W_COUNT == 20 && qsp::Q_COUNT == 16 && qsp::ADJ_REC == 11 && qsp::PACK_KEYS_MAX == 1024);
    CHECK(g_live.empty() && g_mallocs == g_frees);
    if (g_bad) return 1;
    std::printf("devbuf ok: %d allocations, %d frees, %d copies, %d fills\n", g_mallocs, g_frees, g_copies, g_fills);
    return 0;
}
