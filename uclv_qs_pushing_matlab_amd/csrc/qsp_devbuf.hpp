// qsp_devbuf.hpp — host side of the C ABI's device memory (qsp_capi.hip): how many elements each array of
// the kernels' argument blocks holds (Dims), stated once, and the typed buffer that owns one (Dev<T>).
// Host only: nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "qsp_kernels.h"

namespace qsp {
#pragma GCC visibility push(hidden)   // internal to the library: no symbol of these leaves it

// Element counts (not bytes) of the arrays of a handle of B lanes and horizon N: the shapes that the
// comments of SolveArgs, ClosedLoopArgs and OpenLoopArgs (qsp_kernels.h) document.
struct Dims {
    size_t B = 0, N = 0;
    size_t lane() const { return B; }                  // one per lane: ids, status, counters, cost, flags
    size_t x0() const { return B * 4; }                // also wx0, the closed loop's plant state
    size_t res() const { return B * 4; }               // wres: stat, eq, ineq, comp
    size_t u0() const { return B * 2; }
    size_t X() const { return B * (N + 1) * 4; }
    size_t U() const { return B * N * 2; }
    size_t PI() const { return B * N * 4; }
    size_t yref() const { return B * N * 6; }
    size_t yref_e() const { return B * 4; }
    size_t lam() const { return B * N * 6; }           // qp_lam, qsp_get_lam, the KKT evaluators' LAM
    size_t kkt_parts() const { return B * KKT_NPARTS; }
    size_t kkt_stage_res() const { return B * (N + 1) * 4; }
    size_t qp_res() const { return B * KKT_QP_NRES; }
    size_t qp_A() const { return B * N * QpLaneData::NA; }   // caller-given QP data (qsp_point.hpp)
    size_t qp_B() const { return B * N * QpLaneData::NB; }
    size_t qp_Hg() const { return B * QpLaneData::hg(N); }
    size_t qp_bound() const { return B * N * QpLaneData::NBOUND; }
    size_t sens_K0() const { return B * 8; }           // the sensitivities' outputs: K0 2 x 4 per lane,
    size_t sens_gains() const { return B * N * 8; }    // K and dU 2 x 4 per stage,
    size_t sens_P0() const { return B * 10; }          // P0's upper triangle;
    size_t sens_ws() const { return SF_COUNT * N * B; }   // and workspaces (SensField, SENS_NK)
    size_t sens_wK() const { return SENS_NK * N * B; }
    size_t stages() const { return B * (N + 1); }      // stride of the SoA workspaces
    size_t lin() const { return L_COUNT * stages(); }
    size_t nlp() const { return W_COUNT * stages(); }
    size_t qp() const { return Q_COUNT * stages(); }
    size_t adj() const { return ADJ_REC * B * N; }
    static size_t hist() { return (size_t)SQP_MAX_PARTS * WHIST_PER_PART; }
    // closed loop of T steps: logs, noise, metrics; delay buffers of D columns
    size_t cl_X(size_t T) const { return B * (T + 1) * 4; }
    size_t cl_Xsim(size_t T) const { return B * T * 4; }
    size_t cl_U(size_t T) const { return B * T * 2; }
    size_t cl_status(size_t T) const { return B * T; }
    size_t cl_noise(size_t T) const { return T * B * 4; }   // a noise table: the caller's, or qsp_gen_sim_noise's
    size_t metrics() const { return B * CL_NMETRICS; }
    size_t delay(size_t D) const { return B * D * 2; }
    // reference table of T rows: shared, or one per lane
    static size_t traj(size_t T) { return T * 6; }
    size_t traj_lanes(size_t T) const { return B * T * 6; }
    // open loop: the plant's delay ring of D columns for M candidates per lane
    size_t ring(size_t D, size_t M) const { return D * B * M; }
};

// A device array of T that owns its allocation: grow-only ensure() (kept when large enough, else freed and
// allocated anew, contents lost), freed by the destructor.  The copies and fill are asynchronous on the
// stream given and refuse a count above the capacity before anything is touched.
template <class T>
class Dev {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p_) (void)hipFree(p_); }
    T* data() const { return p_; }
    size_t count() const { return n_; }
    hipError_t ensure(size_t count) {
        if (count <= n_) return hipSuccess;
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e == hipSuccess) {
            p_ = static_cast<T*>(q);
            n_ = count;
        }
        return e;
    }
    hipError_t upload(hipStream_t stream, const T* host, size_t count) const {
        if (count > n_) return hipErrorInvalidValue;
        return hipMemcpyAsync(p_, host, count * sizeof(T), hipMemcpyHostToDevice, stream);
    }
    hipError_t download(hipStream_t stream, T* host, size_t count) const {
        if (count > n_) return hipErrorInvalidValue;
        return hipMemcpyAsync(host, p_, count * sizeof(T), hipMemcpyDeviceToHost, stream);
    }
    hipError_t fill(hipStream_t stream, int byte, size_t count) const {
        if (count > n_) return hipErrorInvalidValue;
        return hipMemsetAsync(p_, byte, count * sizeof(T), stream);
    }
};

#pragma GCC visibility pop
}  // namespace qsp
