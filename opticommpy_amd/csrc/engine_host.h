// engine_host.h -- the host half that the DSP engines share (engine_metrics, engine_cpr, engine_eq, engine_fec, engine_sync; HIP
// only, nothing else includes it): grow-only device buffers, the per-engine state and the prologue of an entry point, staging of
// array arguments and results, the launch grid, the rocFFT plan cache and the upload of numpy's pairwise leaves.
// An engine brings its own `Work` (derived from WorkBase: its Bufs, and the host vectors its asynchronous uploads read) and
// names `using Call = CallT<Work>`; every entry point then starts with `Call c(device, err); if (c.rc) return c.rc;`.
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "metrics_kernels.h"
#include "ssf_internal.h"

namespace ssf {
namespace eng {

// a device allocation that only grows
struct Buf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t need(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
};

struct WorkBase {
    hipStream_t st = nullptr;                 // non-blocking, made by the first call on the device
};

// one engine's state: W is that engine's own Work type, so every engine has its own mutex and, per device, its own stream,
// buffers and plans (they live until the process ends).  Engines run concurrently from different threads, and one may call
// another while it holds its own lock (sync_run -> rx_decimate).
template <class W> struct State {
    static inline std::mutex mu;
    static inline std::map<int, W> work;
};

// one call into an engine: holds the engine's lock from construction on; rc and *err carry the first failure
template <class W> struct CallT {
    std::lock_guard<std::mutex> lock{State<W>::mu};
    W *w = nullptr;
    std::string *err;
    int rc = SSF_OK;
    // selects the device and, unless the call only allocates or frees (stream = false: w stays NULL), finds the device's Work
    CallT(int device, std::string *e, bool stream = true) : err(e) {
        if (!ok(hipSetDevice(device), "hipSetDevice") || !stream) return;
        w = &State<W>::work[device];
        if (!w->st) ok(hipStreamCreateWithFlags(&w->st, hipStreamNonBlocking), "hipStreamCreate");
    }
    bool ok(hipError_t e, const char *what) {
        if (e == hipSuccess) return true;
        rc = e == hipErrorOutOfMemory ? SSF_ERR_OOM : SSF_ERR_HIP;
        *err = std::string(what) + ": " + hipGetErrorString(e);
        (void)hipGetLastError();
        return false;
    }
    bool fft_fail(const char *what) {
        rc = SSF_ERR_FFT, *err = what;
        return false;
    }
    bool need(Buf &b, size_t bytes) { return ok(b.need(bytes), "hipMalloc"); }
    // device view of an array argument: a device pointer as it is, host memory through a staging buffer
    const void *input(const void *p, Buf &stage, size_t bytes) {
        if (on_device(p)) return p;
        if (!need(stage, bytes)) return nullptr;
        if (!ok(hipMemcpyAsync(stage.p, p, bytes, hipMemcpyHostToDevice, w->st), "hipMemcpy")) return nullptr;
        return stage.p;
    }
    // where a result is computed: the caller's device memory, or `stage` when the caller's pointer is host memory (or NULL)
    void *target(void *user, Buf &stage, size_t bytes) {
        if (user && on_device(user)) return user;
        return need(stage, bytes) ? stage.p : nullptr;
    }
    bool deliver(void *user, const void *dev, size_t bytes) {
        if (!user || user == dev) return true;
        return ok(hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, w->st), "hipMemcpy");
    }
    bool launched() { return ok(hipGetLastError(), "kernel launch"); }
    bool sync() { return ok(hipStreamSynchronize(w->st), "hipStreamSynchronize"); }
};

// workgroups of `block` lanes for a grid-stride loop over `count` elements.  The number of workgroups is the number of partial
// sums, which fixes the order of every sum: an engine's cap is part of its results.
inline int grid_blocks(long long count, int block, int max_blocks, int min_blocks = 0) {
    const long long nb = (count + block - 1) / block;
    return (int)(nb < min_blocks ? min_blocks : nb < max_blocks ? nb : max_blocks);
}

// ---- rocFFT: double precision, in place, on the engine's stream; plans are kept per device in the engine's Work
struct FftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    void *work = nullptr;
};
using FftPlans = std::map<std::tuple<long long, int, int>, FftPlan>;      // (length, batch, inverse)

inline void fft_setup_once() {
    static std::once_flag once;               // one for all engines: an inline function's static
    std::call_once(once, [] { rocfft_setup(); });
}

// `batch` transforms of `length` points each, contiguous in buf; c.w->plans (FftPlans) is the cache
template <class C> bool transform(C &c, void *buf, long long length, int batch, bool inverse) {
    fft_setup_once();
    FftPlan &p = c.w->plans[std::make_tuple(length, batch, (int)inverse)];
    if (!p.plan) {
        const size_t len = (size_t)length;
        if (rocfft_plan_create(&p.plan, rocfft_placement_inplace, inverse ? rocfft_transform_type_complex_inverse : rocfft_transform_type_complex_forward,
                               rocfft_precision_double, 1, &len, (size_t)batch, nullptr) != rocfft_status_success) {
            p.plan = nullptr;
            return c.fft_fail("rocfft_plan_create failed");
        }
        size_t ws = 0;
        rocfft_plan_get_work_buffer_size(p.plan, &ws);
        if (rocfft_execution_info_create(&p.info) != rocfft_status_success) return c.fft_fail("rocfft_execution_info_create failed");
        if (ws) {
            if (!c.ok(hipMalloc(&p.work, ws), "hipMalloc")) return false;
            rocfft_execution_info_set_work_buffer(p.info, p.work, ws);
        }
        rocfft_execution_info_set_stream(p.info, c.w->st);
    }
    void *io[1] = {buf};
    if (rocfft_execute(p.plan, io, nullptr, p.info) != rocfft_status_success) return c.fft_fail("rocfft_execute failed");
    return true;
}

// ---- the leaves of numpy's pairwise sum over n elements (mk::pw_leaves), on the device: nleaf + 1 starts, the last one n
struct PwLeaves {
    Buf start;
    std::vector<long long> host;              // source of an asynchronous upload: it outlives the call
    long long of = -1;                        // the n that `start` holds, kept while n stays the same
};
template <class C> bool pairwise_leaves(C &c, PwLeaves &l, long long n, long long &nleaf, const long long *&leaf_start) {
    nleaf = mk::pw_leaves(n, nullptr);
    if (l.of != n) {
        if (!c.sync()) return false;                                // an earlier upload may still read l.host
        l.host.assign(nleaf + 1, n);
        mk::pw_leaves(n, l.host.data());
        l.of = -1;
        if (!c.need(l.start, l.host.size() * sizeof(long long))) return false;
        if (!c.ok(hipMemcpyAsync(l.start.p, l.host.data(), l.host.size() * sizeof(long long), hipMemcpyHostToDevice, c.w->st), "hipMemcpy"))
            return false;
        l.of = n;
    }
    leaf_start = (const long long *)l.start.p;
    return true;
}

}  // namespace eng
}  // namespace ssf
