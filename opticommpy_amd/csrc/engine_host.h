// engine_host.h -- the host half that the DSP engines share.  Every engine_*.hip whose entry points start with a `Call` includes
// it (HIP only, nothing else does): grow-only device buffers, the per-engine state and the prologue of an entry point, staging of
// array arguments and results, uploads, the launch grid, the rocFFT plan cache and the upload of numpy's pairwise leaves.
// An engine brings its own `Work` (derived from WorkBase: its Bufs, and host vectors kept between calls for their capacity) and
// names `using Call = CallT<Work>`; every entry point then starts with `Call c(device, err); if (c.rc) return c.rc;`.
//
// The invariant: whenever an engine's lock is free, its stream is idle.  A call that succeeds ends with sync(); a call that fails
// waits on the stream at the moment the failure is recorded.  Host memory that a call handed to the stream -- the caller's arrays,
// the call's own locals, a vector in Work -- is therefore no longer referenced after any return, and the next call may overwrite
// or free it without a wait of its own.  An entry point's part: return at the first failure, enqueue nothing after it.
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
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
        return fail(e == hipErrorOutOfMemory ? SSF_ERR_OOM : SSF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    bool fft_fail(const char *what) { return fail(SSF_ERR_FFT, what); }
    // a failure the engine finds itself (a result it read back, an argument only it can judge)
    bool reject(int code, const char *message) { return fail(code, message); }
    bool need(Buf &b, size_t bytes) { return ok(b.need(bytes), "hipMalloc"); }
    // host memory to device memory on the call's stream; the host side only has to live until the call returns
    bool h2d(void *dev, const void *host, size_t bytes) { return ok(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, w->st), "hipMemcpy"); }
    bool upload(Buf &b, const void *host, size_t bytes) { return need(b, bytes) && h2d(b.p, host, bytes); }
    template <class T> bool upload(Buf &b, const std::vector<T> &host) { return upload(b, host.data(), host.size() * sizeof(T)); }
    // device view of an array argument: a device pointer as it is, host memory through a staging buffer
    const void *input(const void *p, Buf &stage, size_t bytes) {
        if (on_device(p)) return p;
        return upload(stage, p, bytes) ? stage.p : nullptr;
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

  private:
    // the one way a call fails: the first failure keeps rc and *err, and the stream is drained before anyone can return (the
    // header's invariant; a constructor that failed has no stream yet, a call with stream = false no Work)
    bool fail(int code, std::string message) {
        if (rc == SSF_OK) rc = code, *err = std::move(message);
        if (w && w->st) (void)hipStreamSynchronize(w->st);
        (void)hipGetLastError();
        return false;
    }
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
    std::vector<long long> host;              // kept for its capacity
    long long of = -1;                        // the n that `start` holds, kept while n stays the same
};
template <class C> bool pairwise_leaves(C &c, PwLeaves &l, long long n, long long &nleaf, const long long *&leaf_start) {
    nleaf = mk::pw_leaves(n, nullptr);
    if (l.of != n) {
        l.host.assign(nleaf + 1, n);
        mk::pw_leaves(n, l.host.data());
        l.of = -1;
        if (!c.upload(l.start, l.host)) return false;
        l.of = n;
    }
    leaf_start = (const long long *)l.start.p;
    return true;
}

}  // namespace eng
}  // namespace ssf
