// ssf_api.hip -- the extern "C" boundary declared in include/ssf.h.
#include <map>
#include <memory>
#include <thread>
#include <utility>

#include "ssf_internal.h"

using namespace ssf;

namespace {
thread_local std::string g_err;   // errors raised without a plan (plan creation, discovery)

int set_err(int code, const std::string &m) {
    g_err = m;
    return code;
}

int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_err(SSF_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return set_err(SSF_ERR_NO_DEVICE, "device index out of range");
    return SSF_OK;
}

// the tail of an entry point that goes into an engine: run(err) is the engine's function, its text goes out as "<name>: <text>"
template <class F> int engine_result(const char *name, F &&run) {
    std::string err;
    const int rc = run(&err);
    return rc ? set_err(rc, std::string(name) + ": " + err) : SSF_OK;
}
// ... after the device index has been checked
template <class F> int engine_call(const char *name, int device, F &&run) {
    if (int rc = check_device(device)) return rc;
    return engine_result(name, run);
}

int check_params(ssf_plan *pl, const ssf_params *p, int s0, int s1) {
    if (!p) return fail(pl, SSF_ERR_BAD_ARG, "params is NULL");
    if (p->model != SSF_MODEL_NLSE && p->model != SSF_MODEL_MANAKOV) return fail(pl, SSF_ERR_BAD_ARG, "bad model");
    if (p->model == SSF_MODEL_MANAKOV && (pl->nrows % 2)) return fail(pl, SSF_ERR_BAD_ARG, "Manakov model needs an even number of rows");
    if (p->model == SSF_MODEL_NLSE && p->direction < 0) return fail(pl, SSF_ERR_BAD_ARG, "NLSE model has no back-propagation mode");
    if (!(p->Fs > 0) || !(p->Fc > 0)) return fail(pl, SSF_ERR_BAD_ARG, "Fs and Fc must be positive");
    if (!(p->Lspan > 0)) return fail(pl, SSF_ERR_BAD_ARG, "Lspan must be positive");
    if (!(p->hz > 0) && !(p->model == SSF_MODEL_MANAKOV && p->nlprMethod)) return fail(pl, SSF_ERR_BAD_ARG, "hz must be positive");
    if (p->model == SSF_MODEL_MANAKOV && p->maxIter < 1) return fail(pl, SSF_ERR_BAD_ARG, "maxIter must be >= 1");
    if (p->Nspans < 0 || s0 < 1 || s1 > p->Nspans) return fail(pl, SSF_ERR_BAD_ARG, "span range outside [1, Nspans]");
    if (p->amp < SSF_AMP_NONE || p->amp > SSF_AMP_EDFA) return fail(pl, SSF_ERR_BAD_ARG, "bad amp");
    if (p->amp == SSF_AMP_EDFA && p->direction >= 0) {
        if (!(p->alpha * p->Lspan > 0)) return fail(pl, SSF_ERR_BAD_ARG, "EDFA gain should be a positive scalar");   // devices.py:709
        if (!(p->NF >= 3)) return fail(pl, SSF_ERR_BAD_ARG, "The minimal EDFA noise figure is 3 dB");                 // devices.py:710
    }
    if (p->n_save < 0 || (p->n_save > 0 && !p->save_spans)) return fail(pl, SSF_ERR_BAD_ARG, "bad save_spans");
    return SSF_OK;
}
}  // namespace

extern "C" {

const char *ssf_version(void) { return "opticommpy_amd-ssf 0.1 (gfx950)"; }

int ssf_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) return set_err(SSF_ERR_HIP, hipGetErrorString(e));
    return n;
}

int ssf_device_info(int device, ssf_device_info_t *out) {
    if (!out) return set_err(SSF_ERR_BAD_ARG, "out is NULL");
    hipDeviceProp_t pr;
    hipError_t e = hipGetDeviceProperties(&pr, device);
    if (e != hipSuccess) return set_err(SSF_ERR_NO_DEVICE, hipGetErrorString(e));
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->name, sizeof(out->name), "%s", pr.name);
    std::snprintf(out->arch, sizeof(out->arch), "%s", pr.gcnArchName);
    out->compute_units = pr.multiProcessorCount;
    out->total_mem_bytes = (int64_t)pr.totalGlobalMem;
    out->lds_per_block_bytes = (int64_t)pr.sharedMemPerBlock;
    return SSF_OK;
}

const char *ssf_last_error(const ssf_plan *plan) { return plan ? plan->err.c_str() : g_err.c_str(); }

static bool smooth13(int64_t n) {
    for (int q : {2, 3, 5, 7, 11, 13})
        while (n % q == 0) n /= q;
    return n == 1;
}

int ssf_plan_create(int device, int64_t N, int32_t nrows, int32_t precision, int32_t engine, ssf_plan **out) {
    if (!out) return set_err(SSF_ERR_BAD_ARG, "out is NULL");
    *out = nullptr;
    if (N < 2 || nrows < 1) return set_err(SSF_ERR_BAD_ARG, "N must be >= 2 and nrows >= 1");
    if (precision != SSF_C64 && precision != SSF_C128) return set_err(SSF_ERR_BAD_ARG, "bad precision");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_err(SSF_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return set_err(SSF_ERR_NO_DEVICE, "device index out of range");
    if (hipSetDevice(device) != hipSuccess) return set_err(SSF_ERR_HIP, "hipSetDevice failed");
    auto *pl = new ssf_plan();
    pl->device = device;
    pl->N = N;
    pl->nrows = nrows;
    pl->precision = precision;
    if (hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking) != hipSuccess) {
        delete pl;
        return set_err(SSF_ERR_HIP, "hipStreamCreate failed");
    }
    (void)pl->stager.init();          // falls back to plain copies if pinned memory is unavailable
    // SSF_ENGINE_FUSED / AUTO: the fused pipeline when it takes N natively, otherwise the general-length engine with its
    // transforms built from the fused kernels (Bluestein); rocFFT only on request (the on-GPU cross-check) or, under AUTO,
    // for lengths beyond the Bluestein range (2N - 1 > 2^22 complex128 / 2^23 complex64)
    const bool native = fused_supports(N, nrows, precision), general = !native && general_supports(N, nrows, precision);
    int want = engine;
    if (want == SSF_ENGINE_AUTO) {
        want = (native || general) ? SSF_ENGINE_FUSED : SSF_ENGINE_ROCFFT;
        // AUTO is never the slower engine: lengths the hand-written kernels only reach through a Bluestein convolution, but
        // whose prime factors are all <= 13 (30 030 = 2 3 5 7 11 13), are one or two native kernels for rocFFT (measured,
        // tools/bench_lengths.py: 30 030: 4 653 against 3 446 steps/s); primes and other lengths stay on the fused kernels
        // (10 007: 3 753 against 2 950; rocFFT itself falls back to Bluestein there).  SSF_ENGINE_FUSED still forces them.
        // The one-launch LDS rows (2^a 3^b 5^c <= 8192) win from about 4000 samples on (6000: 7 491 against 4 918 steps/s); below,
        // a single workgroup per row is one long latency chain and rocFFT's small kernels are faster (1500: 6 040 against
        // 7 427, 3000: 5 477 against 6 393; gpurun_out/r3e/lengths.txt).
        const bool rows_win = fused_rows_supports(N) && N >= 4000;
        if (!native && general && !rows_win && smooth13(N)) want = SSF_ENGINE_ROCFFT;
    }
    if (want == SSF_ENGINE_FUSED && !native && !general) {
        (void)hipStreamDestroy(pl->stream);
        delete pl;
        return set_err(SSF_ERR_UNSUPPORTED, "fused engine: N beyond the range of its transforms (use SSF_ENGINE_ROCFFT)");
    }
    pl->engine = want == SSF_ENGINE_ROCFFT ? make_rocfft_engine(pl) : native ? make_fused_engine(pl) : make_general_engine(pl);
    if (!pl->engine) {
        const int code = pl->err.find("out of memory") != std::string::npos ? SSF_ERR_OOM : SSF_ERR_HIP;
        set_err(code, pl->err.empty() ? "engine creation failed" : pl->err);
        (void)hipStreamDestroy(pl->stream);
        delete pl;
        return code;
    }
    pl->engine_id = pl->engine->id();
    *out = pl;
    return SSF_OK;
}

int ssf_plan_set_lanes(ssf_plan *plan, int32_t n_lanes) {
    if (!plan || !plan->engine) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (n_lanes < 1) return fail(plan, SSF_ERR_BAD_ARG, "ssf_plan_set_lanes: n_lanes must be >= 1");
    plan->lanes = n_lanes;
    return plan->engine->set_lanes(n_lanes);
}

int ssf_plan_pipeline(const ssf_plan *plan) {
    if (!plan || !plan->engine) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    return plan->engine->pipeline();
}

// ssf_plan_set_units rebuilds the engine; if that fails AND the rebuild with the old unit count fails too (out of memory twice) the
// plan is left without one: every entry point that needs it says so instead of dereferencing a null pointer
#define SSF_NEED_ENGINE(plan)                                                                                        \
    do {                                                                                                             \
        if (!(plan)->engine) return fail((plan), SSF_ERR_STATE, "the plan has no engine (ssf_plan_set_units failed)"); \
    } while (0)

int ssf_plan_set_units(ssf_plan *plan, int32_t n_units) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (n_units < 1 || plan->nrows % n_units) return fail(plan, SSF_ERR_BAD_ARG, "ssf_plan_set_units: nrows must be a multiple of n_units");
    if (n_units == plan->units) return SSF_OK;
    // (rebuilding the engine would silently drop an attached coupling communicator / reducer: the caller would go on believing
    //  the plan is coupled -- and a plan of independent units is not a coupled batch anyway)
    if (plan->coupled) return fail(plan, SSF_ERR_STATE, "ssf_plan_set_units: detach the coupling communicator / reducer first (ssf_set_coupling[_comm](plan, NULL))");
    if (plan->engine_id != SSF_ENGINE_FUSED || !fused_supports(plan->N, plan->nrows, plan->precision))
        return fail(plan, SSF_ERR_UNSUPPORTED, "independent units need the natively split fused engine");
    if (n_units > 65535) return fail(plan, SSF_ERR_BAD_ARG, "ssf_plan_set_units: at most 65535 units");
    SSF_HIP(plan, hipSetDevice(plan->device));
    (void)plan->sink.sync();
    delete plan->engine;
    plan->engine = nullptr;
    const int old = plan->units;
    plan->units = n_units;
    plan->has_field = false;
    plan->engine = make_fused_engine(plan);
    if (plan->engine) (void)plan->engine->set_lanes(plan->lanes);
    if (!plan->engine) {                                    // (out of memory?) back to what worked
        const std::string why = plan->err;
        plan->units = old;
        plan->engine = make_fused_engine(plan);
        return fail(plan, why.find("out of memory") != std::string::npos ? SSF_ERR_OOM : SSF_ERR_HIP,
                    why.empty() ? "engine creation failed" : why);
    }
    return SSF_OK;
}

int ssf_get_unit_stats(ssf_plan *plan, int32_t unit, ssf_stats *out) {
    if (!plan || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_get_unit_stats: NULL argument");
    ssf_stats u{};
    SSF_NEED_ENGINE(plan);
    int rc = plan->engine->unit_stats(unit, &u);
    if (rc) return fail(plan, rc, "ssf_get_unit_stats: no such unit (or not a plan of independent units)");
    *out = plan->stats;
    out->steps = u.steps;
    out->iterations = u.iterations;
    out->transforms = u.transforms;
    out->nonconverged_steps = u.nonconverged_steps;
    out->decided_ahead = u.decided_ahead;
    out->rebuilt_iterates = u.rebuilt_iterates;
    out->recovered_fields = u.recovered_fields;
    out->bytes_algorithmic = (double)u.transforms * 2.0 * (plan->precision == SSF_C128 ? 16.0 : 8.0) * (double)plan->N;
    return SSF_OK;
}

int ssf_plan_destroy(ssf_plan *plan) {
    if (!plan) return SSF_OK;
    (void)hipSetDevice(plan->device);
    (void)plan->sink.sync();
    delete plan->engine;
    if (plan->stream) (void)hipStreamDestroy(plan->stream);
    delete plan;
    return SSF_OK;
}

static int upload_common(ssf_plan *plan, const void *field, bool aos) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (!field) return fail(plan, SSF_ERR_BAD_ARG, "field is NULL");
    SSF_HIP(plan, hipSetDevice(plan->device));
    SSF_NEED_ENGINE(plan);
    int rc = plan->engine->upload(field, aos);
    if (rc) return rc;
    plan->stats = ssf_stats{};
    plan->stats.engine = plan->engine_id;
    plan->has_field = true;
    return SSF_OK;
}
int ssf_upload(ssf_plan *plan, const void *field_soa) { return upload_common(plan, field_soa, false); }
int ssf_upload_aos(ssf_plan *plan, const void *field_aos) { return upload_common(plan, field_aos, true); }

int ssf_execute(ssf_plan *plan, const ssf_params *params, int32_t span_first, int32_t span_last, const void *noise,
                ssf_stats *stats, ssf_trace *trace) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (!plan->has_field) return fail(plan, SSF_ERR_STATE, "ssf_execute before ssf_upload");
    int rc = check_params(plan, params, span_first, span_last);
    if (!rc && plan->sink.active()) {          // every capture of this call must fit the caller's (N, ld) array
        long long ncap = 0;
        for (int i = 0; i < params->n_save; ++i)
            if (params->save_spans[i] >= span_first && params->save_spans[i] <= span_last) ++ncap;
        if (((long long)plan->sink.count() + ncap) * plan->nrows > plan->sink.leading())
            return fail(plan, SSF_ERR_BAD_ARG, "snapshot sink: the captures of this call do not fit the destination's columns");
    }
    if (rc) return rc;
    SSF_HIP(plan, hipSetDevice(plan->device));
    if (trace) trace->count = 0;
    if (span_first <= span_last) {
        SSF_NEED_ENGINE(plan);
        rc = plan->engine->execute(*params, span_first, span_last, noise, &plan->stats, trace);
        if (rc) return rc;
    }
    const double s = plan->precision == SSF_C128 ? 16.0 : 8.0;
    plan->stats.bytes_algorithmic = (double)plan->stats.transforms * 2.0 * s * (double)plan->N;
    if (stats) *stats = plan->stats;
    return SSF_OK;
}

static int download_common(ssf_plan *plan, void *dst, int which, bool aos) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (!dst) return fail(plan, SSF_ERR_BAD_ARG, "destination is NULL");
    if (!plan->has_field) return fail(plan, SSF_ERR_STATE, "download before ssf_upload");
    SSF_NEED_ENGINE(plan);
    if (which < -1 || which >= plan->engine->n_snapshots()) return fail(plan, SSF_ERR_BAD_ARG, "no such snapshot");
    SSF_HIP(plan, hipSetDevice(plan->device));
    return plan->engine->download(dst, which, aos);
}
int ssf_download(ssf_plan *plan, void *field_soa) { return download_common(plan, field_soa, -1, false); }
int ssf_download_aos(ssf_plan *plan, int32_t which, void *field_aos) { return download_common(plan, field_aos, which, true); }

int ssf_download_snapshots(ssf_plan *plan, void *snap_soa) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (!snap_soa) return fail(plan, SSF_ERR_BAD_ARG, "snapshot buffer is NULL");
    const size_t fb = (size_t)plan->N * plan->nrows * (plan->precision == SSF_C128 ? 16 : 8);
    SSF_NEED_ENGINE(plan);
    for (int i = 0; i < plan->engine->n_snapshots(); ++i) {
        int rc = download_common(plan, (char *)snap_soa + (size_t)i * fb, i, false);
        if (rc) return rc;
    }
    return SSF_OK;
}

int ssf_set_snapshot_sink(ssf_plan *plan, void *dst, int64_t ld, int32_t first_index) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (dst && (ld < plan->nrows || first_index < 0)) return fail(plan, SSF_ERR_BAD_ARG, "ssf_set_snapshot_sink: ld < nrows or negative index");
    SSF_HIP(plan, hipSetDevice(plan->device));
    SSF_HIP(plan, plan->sink.set(plan->device, dst, ld, first_index, plan->precision == SSF_C128 ? 16 : 8));
    return SSF_OK;
}

int ssf_sync_snapshots(ssf_plan *plan) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    SSF_HIP(plan, hipSetDevice(plan->device));
    SSF_HIP(plan, hipStreamSynchronize(plan->stream));        // device destinations: ordered on the plan's stream
    SSF_HIP(plan, plan->sink.sync());
    return SSF_OK;
}

int ssf_run(ssf_plan *plan, const ssf_params *params, const void *in, void *out, void *snaps, const void *noise,
            ssf_stats *stats, ssf_trace *trace) {
    int rc = ssf_upload(plan, in);
    if (rc) return rc;
    rc = ssf_execute(plan, params, 1, params ? params->Nspans : 0, noise, stats, trace);
    if (rc) return rc;
    if (out && (rc = ssf_download(plan, out))) return rc;
    if (snaps && plan->stats.n_snapshots > 0 && (rc = ssf_download_snapshots(plan, snaps))) return rc;
    return SSF_OK;
}

int ssf_set_coupling(ssf_plan *plan, ssf_reduce_fn reduce, void *ctx) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    SSF_NEED_ENGINE(plan);
    int rc = plan->engine->set_coupling(reduce, ctx);
    if (rc == SSF_OK) plan->coupled = reduce != nullptr;
    return rc ? fail(plan, rc, "coupled batches need the general-length engine (create the plan with SSF_ENGINE_ROCFFT)") : SSF_OK;
}

int ssf_set_coupling_comm(ssf_plan *plan, ssf_comm *comm) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    SSF_NEED_ENGINE(plan);
    if (comm && ssf::comm_device(comm) != plan->device) return fail(plan, SSF_ERR_BAD_ARG, "ssf_set_coupling_comm: the communicator lives on another device");
    if (comm && plan->units > 1) return fail(plan, SSF_ERR_UNSUPPORTED, "ssf_set_coupling_comm: a plan of independent units is not a coupled batch");
    int rc = plan->engine->set_coupling_comm(comm);
    if (rc == SSF_OK) plan->coupled = comm != nullptr;
    return rc ? fail(plan, rc, "device-side coupling needs the device-resident fused pipeline (else: ssf_set_coupling on SSF_ENGINE_ROCFFT)") : SSF_OK;
}

int ssf_couple_reduce_selftest(int device, int32_t nranks, int32_t npart, const double *parts, double *out5) {
    if (int rc = check_device(device)) return rc;
    if (hipSetDevice(device) != hipSuccess) return set_err(SSF_ERR_HIP, "hipSetDevice");
    std::string err;
    int rc = ssf::fused_couple_reduce_selftest(nranks, npart, parts, out5, &err);
    return rc ? set_err(rc, err.empty() ? "ssf_couple_reduce_selftest: bad argument" : err) : SSF_OK;
}

int ssf_set_profiling(ssf_plan *plan, int32_t enable) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    SSF_NEED_ENGINE(plan);
    int rc = plan->engine->set_profiling(enable);
    return rc ? fail(plan, rc, "per-kernel profiling is only available on the fused engine") : SSF_OK;
}

int ssf_get_kernel_times(ssf_plan *plan, ssf_kernel_times *out) {
    if (!plan) return set_err(SSF_ERR_BAD_ARG, "plan is NULL");
    if (!out) return fail(plan, SSF_ERR_BAD_ARG, "out is NULL");
    SSF_NEED_ENGINE(plan);
    int rc = plan->engine->kernel_times(out);
    return rc ? fail(plan, rc, "per-kernel profiling is only available on the fused engine") : SSF_OK;
}

namespace {
// memory shape of the fused row stage, no arithmetic (see include/ssf.h)
__global__ void __launch_bounds__(256) k_burst_copy(const double2 *__restrict__ a, double2 *__restrict__ b) {
    const double2 *g = a + (size_t)blockIdx.x * 4096;
    double2 *o = b + (size_t)blockIdx.x * 4096;
    double2 v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = g[threadIdx.x + 256 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) o[threadIdx.x + 256 * q] = v[q];
}
}  // namespace

int ssf_device_copy_bandwidth(int device, int64_t bytes, int32_t launches, double *gbs) {
    if (!gbs || bytes < 65536 || bytes % 65536 || launches < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_device_copy_bandwidth: bytes must be a positive multiple of 64 KiB");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return set_err(SSF_ERR_BAD_ARG, "no such device");
    if (hipSetDevice(device) != hipSuccess) return set_err(SSF_ERR_HIP, "hipSetDevice failed");
    double2 *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = SSF_OK;
    float ms = 0;
    const unsigned nwg = (unsigned)(bytes / 65536);
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) rc = set_err(SSF_ERR_OOM, "hipMalloc failed");
    if (!rc && (hipMemset(a, 0, bytes) != hipSuccess || hipMemset(b, 0, bytes) != hipSuccess)) rc = set_err(SSF_ERR_HIP, "hipMemset failed");
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = set_err(SSF_ERR_HIP, "hipEventCreate failed");
    if (!rc) {
        for (int i = 0; i < 4; ++i) hipLaunchKernelGGL(k_burst_copy, dim3(nwg), dim3(256), 0, 0, i & 1 ? b : a, i & 1 ? a : b);
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < launches; ++i) hipLaunchKernelGGL(k_burst_copy, dim3(nwg), dim3(256), 0, 0, i & 1 ? b : a, i & 1 ? a : b);
        (void)hipEventRecord(e1, 0);
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess)
            rc = set_err(SSF_ERR_HIP, "copy probe failed");
        else *gbs = 2.0 * (double)bytes * launches / ((double)ms * 1e-3) / 1e9;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    return rc;
}

int ssf_linear_channel(ssf_plan *plan, double Fs, double Fc, double alpha, double D, double L, const void *in,
                       void *out) {
    int rc = in ? ssf_upload(plan, in) : SSF_OK;                    // NULL: the field the plan holds (ssf_upload_aos)
    if (rc) return rc;
    SSF_NEED_ENGINE(plan);
    if ((rc = plan->engine->linear_channel(Fs, Fc, alpha, D, L))) return rc;
    return out ? ssf_download(plan, out) : SSF_OK;                  // NULL: left in the plan (ssf_download_aos)
}

int ssf_overlap_save(int device, int64_t sigLen, int32_t nrows, int32_t precision, int32_t nfft, int32_t K,
                     const void *Hfft, const void *sig_in, void *sig_out) {
    if (sigLen < 1 || nrows < 1 || !Hfft || !sig_in || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_overlap_save: bad argument");
    if (precision != SSF_C64 && precision != SSF_C128) return set_err(SSF_ERR_BAD_ARG, "bad precision");
    int lg = 0;
    while ((1 << lg) < nfft) ++lg;
    const int lgmax = precision == SSF_C128 ? 13 : 14;
    if ((1 << lg) != nfft || lg < 4 || lg > lgmax)
        return set_err(SSF_ERR_UNSUPPORTED, "ssf_overlap_save: nfft must be a power of two in [16, 8192 (c128) / 16384 (c64)]");
    if (K < 1 || K > nfft) return set_err(SSF_ERR_BAD_ARG, "FFT size is smaller than filter length");   // core.py:1012
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_err(SSF_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return set_err(SSF_ERR_NO_DEVICE, "device index out of range");
    std::string err;
    // complex128 goes through the receiver pipeline's pooled backend (stream, pinned staging and device
    // blocks are kept between calls); complex64 through the one-shot path of the fused engine
    int rc = precision == SSF_C128 ? ssf::rx_overlap_save(device, sigLen, nrows, nfft, K, Hfft, sig_in, sig_out, &err)
                                   : fused_overlap_save(device, sigLen, nrows, precision, lg, K, Hfft, sig_in, sig_out, &err);
    if (rc) set_err(rc, err);
    return rc;
}

int ssf_mgpu_run(int32_t n_dev, const int32_t *dev_ids, int32_t n_units, int64_t N, int32_t rows_per_unit,
                 int32_t precision, int32_t engine, const ssf_params *params, const void *fields_in,
                 void *fields_out, ssf_stats *stats) {
    if (n_dev < 1 || !dev_ids || n_units < 1 || !params || !fields_in || !fields_out)
        return set_err(SSF_ERR_BAD_ARG, "ssf_mgpu_run: bad argument");
    const size_t unit_bytes = (size_t)rows_per_unit * (size_t)N * (precision == SSF_C128 ? 16 : 8);
    // Two lanes (plan + stream + host thread) per device when it has more than one unit: one unit's transfers overlap
    // the other's kernels, and the kernels of two independent fields fill each other's load / store phases
    // (measured +12-15 % field-steps/s).  Units are independent: the results do not depend on it.
    int lanes = 2;
    if (const char *e = std::getenv("SSF_MGPU_LANES")) lanes = std::max(1, std::min(4, std::atoi(e)));
    // Small units (a launch is one ~10 us latency chain whatever its size): all the units of a device go through ONE plan as
    // independent units -- every launch carries all of them, own control block and decisions per unit, results bit-equal to
    // one plan per unit (ssf_plan_set_units).  SSF_MGPU_BATCH=0 turns it off.
    bool batch = N <= (1ll << 18) && n_units > n_dev && params->model == SSF_MODEL_MANAKOV && (rows_per_unit % 2) == 0 &&
                 engine != SSF_ENGINE_ROCFFT && fused_supports(N, rows_per_unit, precision);
    if (const char *e = std::getenv("SSF_MGPU_BATCH")) batch = batch && std::atoi(e) != 0;
    if (batch) {
        std::vector<int> brc((size_t)n_dev, SSF_OK);
        std::vector<std::string> berr((size_t)n_dev);
        std::vector<std::thread> bt;
        for (int d = 0; d < n_dev; ++d) {
            const int u0 = (int)((int64_t)n_units * d / n_dev), u1 = (int)((int64_t)n_units * (d + 1) / n_dev);
            bt.emplace_back([=, &brc, &berr] {
                constexpr int kMaxBatch = 64;
                for (int b0 = u0; b0 < u1 && brc[(size_t)d] == SSF_OK; b0 += kMaxBatch) {
                    const int nb = std::min(kMaxBatch, u1 - b0);
                    ssf_plan *pl = nullptr;
                    int rc = ssf_plan_create(dev_ids[d], N, rows_per_unit * nb, precision, engine, &pl);
                    if (!rc && nb > 1) rc = ssf_plan_set_units(pl, nb);
                    ssf_params p = *params;
                    p.rng_row_offset = params->rng_row_offset + b0 * rows_per_unit;     // unit u draws rows u * rows_per_unit ...
                    ssf_stats st{};
                    if (!rc) rc = ssf_run(pl, &p, (const char *)fields_in + (size_t)b0 * unit_bytes,
                                          (char *)fields_out + (size_t)b0 * unit_bytes, nullptr, nullptr, &st, nullptr);
                    for (int u = 0; u < nb && !rc && stats; ++u) {
                        if (nb > 1) rc = ssf_get_unit_stats(pl, u, &stats[b0 + u]);
                        else stats[b0 + u] = st;
                    }
                    if (rc) {
                        brc[(size_t)d] = rc;
                        berr[(size_t)d] = ssf_last_error(pl);
                    }
                    if (pl) ssf_plan_destroy(pl);
                }
            });
        }
        for (auto &t : bt) t.join();
        for (int d = 0; d < n_dev; ++d)
            if (brc[(size_t)d]) return set_err(brc[(size_t)d], "device " + std::to_string(dev_ids[d]) + ": " + berr[(size_t)d]);
        return SSF_OK;
    }
    const int nslots = n_dev * lanes;
    std::vector<int> rcs((size_t)nslots, SSF_OK);
    std::vector<std::string> errs((size_t)nslots);
    std::vector<std::thread> th;
    for (int d = 0; d < n_dev; ++d) {
        // contiguous block of units per device: [u0, u1)
        const int u0 = (int)((int64_t)n_units * d / n_dev), u1 = (int)((int64_t)n_units * (d + 1) / n_dev);
        for (int l = 0; l < lanes; ++l) {
            const int slot = d * lanes + l;
            th.emplace_back([=, &rcs, &errs] {
                if (u0 + l >= u1) return;
                ssf_plan *pl = nullptr;
                int rc = ssf_plan_create(dev_ids[d], N, rows_per_unit, precision, engine, &pl);
                if (rc) {
                    rcs[(size_t)slot] = rc;
                    errs[(size_t)slot] = ssf_last_error(nullptr);
                    return;
                }
                if (std::min(lanes, u1 - u0) > 1) (void)ssf_plan_set_lanes(pl, std::min(lanes, u1 - u0));
                for (int u = u0 + l; u < u1 && rc == SSF_OK; u += lanes) {
                    ssf_stats st{};
                    ssf_params pu = *params;                   // a shared seed keys ONE noise stream: unit u draws its own rows of it
                    pu.rng_row_offset = params->rng_row_offset + u * rows_per_unit;
                    rc = ssf_run(pl, &pu, (const char *)fields_in + (size_t)u * unit_bytes,
                                 (char *)fields_out + (size_t)u * unit_bytes, nullptr, nullptr, &st, nullptr);
                    if (stats) stats[u] = st;
                }
                if (rc) {
                    rcs[(size_t)slot] = rc;
                    errs[(size_t)slot] = ssf_last_error(pl);
                }
                ssf_plan_destroy(pl);
            });
        }
    }
    for (auto &t : th) t.join();
    for (int i = 0; i < nslots; ++i)
        if (rcs[(size_t)i]) return set_err(rcs[(size_t)i], "device " + std::to_string(dev_ids[i / lanes]) + ": " + errs[(size_t)i]);
    return SSF_OK;
}

// ---- device-resident arrays ------------------------------------------------------------------
int ssf_device_malloc(int device, int64_t bytes, void **ptr) {
    if (!ptr || bytes < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_device_malloc: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return set_err(SSF_ERR_NO_DEVICE, "device index out of range");
    if (hipSetDevice(device) != hipSuccess) return set_err(SSF_ERR_HIP, "hipSetDevice failed");
    hipError_t e = hipMalloc(ptr, (size_t)bytes);
    if (e != hipSuccess) return set_err(e == hipErrorOutOfMemory ? SSF_ERR_OOM : SSF_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    return SSF_OK;
}

int ssf_device_free(int device, void *ptr) {
    if (!ptr) return SSF_OK;
    if (hipSetDevice(device) != hipSuccess) return set_err(SSF_ERR_HIP, "hipSetDevice failed");
    hipError_t e = hipFree(ptr);
    return e == hipSuccess ? SSF_OK : set_err(SSF_ERR_HIP, std::string("hipFree: ") + hipGetErrorString(e));
}

int ssf_device_memcpy(int device, void *dst, const void *src, int64_t bytes) {
    if (!dst || !src || bytes < 0) return set_err(SSF_ERR_BAD_ARG, "ssf_device_memcpy: bad argument");
    if (hipSetDevice(device) != hipSuccess) return set_err(SSF_ERR_HIP, "hipSetDevice failed");
    const bool dst_dev = ssf::on_device(dst), src_dev = ssf::on_device(src);
    hipError_t e;
    if (dst_dev != src_dev && bytes >= (1 << 20)) {
        // large host <-> device copies of pageable memory go through the pinned double buffer (a plain
        // hipMemcpy of pageable memory runs at a fraction of the link rate)
        // one lane (stream + pinned double buffer + events) per device and host thread: events and streams belong to
        // the device they were created on
        struct Lane {
            hipStream_t st = nullptr;
            ssf::Stager stg;
        };
        thread_local std::map<int, std::unique_ptr<Lane>> lanes;
        std::unique_ptr<Lane> &slot = lanes[device];
        if (!slot) {
            slot.reset(new Lane());
            if (hipStreamCreateWithFlags(&slot->st, hipStreamNonBlocking) != hipSuccess) {
                slot.reset();
                return set_err(SSF_ERR_HIP, "hipStreamCreate failed");
            }
            (void)slot->stg.init();            // (current device = `device`; falls back to plain copies without pinned memory)
        }
        Lane &lane = *slot;
        e = dst_dev ? lane.stg.h2d(dst, src, (size_t)bytes, lane.st) : lane.stg.d2h(dst, src, (size_t)bytes, lane.st);
    } else {
        e = hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDefault);
    }
    return e == hipSuccess ? SSF_OK : set_err(SSF_ERR_HIP, std::string("ssf_device_memcpy: ") + hipGetErrorString(e));
}

// ---- receiver side (engine_rx.hip) -----------------------------------------------------------
int ssf_fir_filter(int device, int64_t sigLen, int32_t ncols, int32_t ntaps, const void *taps, const void *in, void *out) {
    if (!taps || !in || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_fir_filter: NULL argument");
    return engine_call("ssf_fir_filter", device, [&](std::string *err) { return ssf::rx_fir(device, sigLen, ncols, ntaps, taps, in, out, err); });
}

int ssf_fir_long(int device, int64_t inLen, int64_t outLen, int32_t ncols, int64_t ntaps, const void *taps, int64_t shift,
                 const void *in, void *out) {
    if (!taps || !in || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_fir_long: NULL argument");
    return engine_call("ssf_fir_long", device, [&](std::string *err) { return ssf::rx_fir_long(device, inLen, outLen, ncols, ntaps, taps, shift, in, out, err); });
}

int ssf_device_axpy(int device, int64_t n, double alpha, const double *x, double *y) {
    if (!x || !y) return set_err(SSF_ERR_BAD_ARG, "ssf_device_axpy: NULL argument");
    return engine_call("ssf_device_axpy", device, [&](std::string *err) { return ssf::rx_axpy(device, n, alpha, x, y, err); });
}

int ssf_delay_signal(int device, int64_t N, double delay, double Fs, const void *in, void *out) {
    if (!in || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_delay_signal: NULL argument");
    return engine_call("ssf_delay_signal", device, [&](std::string *err) { return ssf::rx_delay(device, N, delay, Fs, in, out, err); });
}

int ssf_edfa(int device, int64_t n, int32_t ncols, double G_lin, double p_noise, int64_t rng_seed, int32_t rng_row_offset,
             const void *field_in, const void *noise, void *field_out) {
    if (!field_in || !field_out || n < 1 || ncols < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_edfa: bad argument");
    if (!(G_lin > 0) || p_noise < 0) return set_err(SSF_ERR_BAD_ARG, "ssf_edfa: the gain must be positive, the noise power non-negative");
    const double sigma = (!noise && rng_seed != 0) ? std::sqrt(p_noise / 2) : 0.0;                  // core.py:739-763
    return engine_call("ssf_edfa", device, [&](std::string *err) {
        return ssf::rx_optics(device, ssf::kOptEdfa, n, ncols, std::sqrt(G_lin), sigma, (unsigned long long)rng_seed,
                              (unsigned)rng_row_offset, field_in, noise, field_out, nullptr, err);
    });
}

int ssf_pbs(int device, int64_t N, int32_t ncols, double theta, const void *E, void *Ex, void *Ey) {
    if (!E || !Ex || !Ey || N < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_pbs: bad argument");
    return engine_call("ssf_pbs", device, [&](std::string *err) {
        return ssf::rx_optics(device, ssf::kOptPbs, N, ncols, std::cos(theta), std::sin(theta), 0, 0, E, nullptr, Ex, Ey, err);
    });
}

int ssf_optical_hybrid_2x4(int device, int64_t N, const void *Es, const void *Elo, void *Eo) {
    if (!Es || !Elo || !Eo || N < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_optical_hybrid_2x4: bad argument");
    return engine_call("ssf_optical_hybrid_2x4", device, [&](std::string *err) {
        return ssf::rx_optics(device, ssf::kOptHybrid, N, 1, 0.0, 0.0, 0, 0, Es, Elo, Eo, nullptr, err);
    });
}

int ssf_nlin_phase_rot(int device, int64_t n, double gamma, const void *Ex, const void *Ey, const double *Pch, double *phi) {
    if (!Ex || !Ey || !Pch || !phi) return set_err(SSF_ERR_BAD_ARG, "ssf_nlin_phase_rot: NULL argument");
    return engine_result("ssf_nlin_phase_rot", [&](std::string *err) { return mk_nlin_phase(device, n, gamma, Ex, Ey, Pch, phi, err); });
}

int ssf_convergence_condition(int device, int64_t n, const void *Ex_fd, const void *Ey_fd, const void *Ex_conv,
                              const void *Ey_conv, double *lim) {
    if (!Ex_fd || !Ey_fd || !Ex_conv || !Ey_conv || !lim) return set_err(SSF_ERR_BAD_ARG, "ssf_convergence_condition: NULL argument");
    return engine_result("ssf_convergence_condition", [&](std::string *err) { return mk_convergence(device, n, Ex_fd, Ey_fd, Ex_conv, Ey_conv, lim, err); });
}

int ssf_decimate(int device, int64_t N, int32_t ncols, int32_t SpSin, int32_t decFactor, const void *in, void *out,
                 int32_t *sampDelay) {
    if (!in || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_decimate: NULL argument");
    return engine_call("ssf_decimate", device, [&](std::string *err) { return ssf::rx_decimate(device, N, ncols, SpSin, decFactor, in, out, sampDelay, err); });
}

int ssf_rx_run(int device, int32_t mode, int64_t N, int32_t nmodes, const ssf_rx_params *params, const void *in0,
               const void *lo, const double *unit_normals, void *out) {
    if (!params || !in0 || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_rx_run: NULL argument");
    if (mode < SSF_RX_PHOTODIODE || mode > SSF_RX_IQ_MIXING) return set_err(SSF_ERR_BAD_ARG, "ssf_rx_run: unknown mode");
    if ((mode == SSF_RX_COHERENT || mode == SSF_RX_PDM_COHERENT) && !lo) return set_err(SSF_ERR_BAD_ARG, "ssf_rx_run: the LO field is NULL");
    return engine_call("ssf_rx_run", device, [&](std::string *err) { return ssf::rx_run(device, mode, N, nmodes, params, in0, lo, unit_normals, out, err); });
}

int ssf_rx_chain(int device, int64_t N, const ssf_rx_params *params, const void *Es, const void *Elo, const void *taps, int32_t ntaps,
                 int32_t SpSin, int32_t decFactor, const void *edc_Hfft, int32_t edc_K, int32_t edc_nfft, void *sig_out,
                 int32_t *sampDelay) {
    if (!params || !Es || !Elo || !taps || !edc_Hfft || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_rx_chain: NULL argument");
    return engine_call("ssf_rx_chain", device, [&](std::string *err) {
        return ssf::rx_chain(device, N, params, Es, Elo, taps, ntaps, SpSin, decFactor, edc_Hfft, edc_K, edc_nfft, sig_out, sampDelay, err);
    });
}

int ssf_wdm_tx(int device, const ssf_tx_params *params, const void *symbols, const double *taps, const double *phi,
               const double *amp, const double *deltaF, void *sig_out, double *power_out) {
    if (!params || !symbols || !taps || !amp || !deltaF || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_wdm_tx: NULL argument");
    return engine_call("ssf_wdm_tx", device, [&](std::string *err) { return ssf::tx_wdm(device, params, symbols, taps, phi, amp, deltaF, sig_out, power_out, err); });
}

// ---- IM/DD transmitter and AWGN channel (engine_rx.hip, imddtx_kernels.h): every check comes before the first allocation or launch
static bool tx_real_or_complex(int32_t dtype) { return dtype == SSF_M_F64 || dtype == SSF_M_C128; }

int ssf_pam_tx(int device, int64_t nSymbols, int32_t SpS, int32_t nPolModes, int32_t ntaps, const double *symbols, const double *taps,
               double mzmScale, double Vpi, double Vb, double ER, double amp, void *sig_out) {
    if (!symbols || !taps || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_pam_tx: NULL argument");
    if (nSymbols < 1 || SpS < 1 || nPolModes < 1 || ntaps < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_pam_tx: sizes must be at least 1");
    if (ntaps > 4096) return set_err(SSF_ERR_UNSUPPORTED, "ssf_pam_tx: at most 4096 pulse-shaping taps");
    if (nSymbols > (int64_t)1 << 40 || nSymbols * SpS > (int64_t)1 << 40) return set_err(SSF_ERR_BAD_ARG, "ssf_pam_tx: too many samples");
    if (!(Vpi != 0) || !std::isfinite(Vpi) || !std::isfinite(Vb) || !std::isfinite(ER) || !std::isfinite(mzmScale) || !std::isfinite(amp))
        return set_err(SSF_ERR_BAD_ARG, "ssf_pam_tx: Vpi must be non-zero and every modulator parameter finite");
    if (int rc = check_device(device)) return rc;
    if (ssf::on_device(symbols) || ssf::on_device(taps)) return set_err(SSF_ERR_BAD_ARG, "ssf_pam_tx: symbols and taps are host arrays");
    return engine_result("ssf_pam_tx", [&](std::string *err) {
        return ssf::tx_pam(device, nSymbols, SpS, nPolModes, ntaps, symbols, taps, mzmScale, Vpi, Vb, ER, amp, sig_out, err);
    });
}

int ssf_modulate_optical(int device, int32_t kind, int64_t n, int32_t u_dtype, const void *u, const void *Ei, double Ei_re, double Ei_im,
                         double Vpi, double VbI, double VbQ, double Vphi, double ERI, double ERQ, void *out) {
    if (!u || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_modulate_optical: NULL argument");
    if (kind < SSF_MOD_PM || kind > SSF_MOD_IQM) return set_err(SSF_ERR_BAD_ARG, "ssf_modulate_optical: kind is SSF_MOD_PM, SSF_MOD_MZM or SSF_MOD_IQM");
    if (n < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_modulate_optical: n must be at least 1");
    if (!tx_real_or_complex(u_dtype)) return set_err(SSF_ERR_UNSUPPORTED, "ssf_modulate_optical: the drive is float64 or complex128");
    if (!(Vpi != 0) || !std::isfinite(Vpi)) return set_err(SSF_ERR_BAD_ARG, "ssf_modulate_optical: Vpi must be finite and non-zero");
    return engine_call("ssf_modulate_optical", device, [&](std::string *err) {
        return ssf::tx_modulate(device, kind, n, u_dtype == SSF_M_C128, u, Ei, Ei_re, Ei_im, Vpi, VbI, VbQ, Vphi, ERI, ERQ, out, err);
    });
}

int ssf_awgn(int device, int64_t n, int32_t ncols, int32_t in_dtype, int32_t out_dtype, int32_t complex_noise, double Fs_over_B,
             double snr_lin, const void *sig_in, const void *unit_normals, int64_t rng_seed, void *sig_out) {
    if (!sig_in || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_awgn: NULL argument");
    if (n < 1 || ncols < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_awgn: sizes must be at least 1");
    if (!tx_real_or_complex(in_dtype) || !tx_real_or_complex(out_dtype)) return set_err(SSF_ERR_UNSUPPORTED, "ssf_awgn: float64 or complex128 arrays");
    if (out_dtype == SSF_M_F64 && (in_dtype != SSF_M_F64 || complex_noise))
        return set_err(SSF_ERR_BAD_ARG, "ssf_awgn: a float64 result needs a float64 signal and real noise");
    if (!(Fs_over_B > 0) || !std::isfinite(Fs_over_B)) return set_err(SSF_ERR_BAD_ARG, "ssf_awgn: Fs / B must be positive and finite");
    if (!(snr_lin > 0) || !std::isfinite(snr_lin)) return set_err(SSF_ERR_BAD_ARG, "ssf_awgn: the linear SNR must be positive and finite");
    if (!unit_normals && rng_seed == 0) return set_err(SSF_ERR_BAD_ARG, "ssf_awgn: unit normals or a non-zero rng_seed");
    return engine_call("ssf_awgn", device, [&](std::string *err) {
        return ssf::ch_awgn(device, n, ncols, in_dtype == SSF_M_C128, out_dtype == SSF_M_C128, complex_noise != 0, Fs_over_B, snr_lin,
                            sig_in, unit_normals, (unsigned long long)rng_seed, sig_out, err);
    });
}

int ssf_upsample(int device, int64_t rows, int32_t w, int32_t factor, double scale, const void *in, void *out) {
    if (!in || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_upsample: NULL argument");
    if (rows < 1 || w < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_upsample: sizes must be at least 1");
    if (factor < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_upsample: the factor must be at least 1");
    if (!std::isfinite(scale)) return set_err(SSF_ERR_BAD_ARG, "ssf_upsample: the scale must be finite");
    if (in == out && factor > 1) return set_err(SSF_ERR_BAD_ARG, "ssf_upsample: in place only with factor 1");
    return engine_call("ssf_upsample", device, [&](std::string *err) { return ssf::tx_stuff(device, rows, w, factor, scale, in, out, err); });
}

// ---- link metrics (engine_metrics.hip): every check comes before the first allocation or launch
static bool metrics_bad_M(int32_t M) { return M < 2 || M > 1024 || (M & (M - 1)) != 0; }
static bool metrics_bad_dtype(int32_t d) { return d < SSF_M_C128 || d > SSF_M_F32; }

int ssf_metrics(int device, const ssf_metrics_params *p, const void *rx, const void *tx, const double *const_raw,
                const double *const_norm, const double *px, const float *evm_w32, ssf_metrics_result *out) {
    if (!p || !rx || !const_norm || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: NULL argument");
    if (metrics_bad_M(p->M)) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: M must be a power of two, 2 .. 1024");
    if (metrics_bad_dtype(p->dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: bad dtype");
    if (p->nModes < 1 || p->nModes > 64) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: nModes must be 1 .. 64");
    if (p->n < 1 || p->discard < 0 || 2 * p->discard >= p->n) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: no symbols left to evaluate");
    const int32_t all = SSF_METRICS_BER | SSF_METRICS_GMI | SSF_METRICS_MI | SSF_METRICS_EVM | SSF_METRICS_EVM_BLIND;
    if (p->want == 0 || (p->want & ~all)) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: bad selection");
    if (p->want & SSF_METRICS_EVM_BLIND) {
        if (p->want != SSF_METRICS_EVM_BLIND || tx || !evm_w32)
            return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: the blind EVM stands alone, takes no tx and needs evm_w32");
    } else {
        if (!tx || !const_raw) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: tx or const_raw is NULL");
        if (!(p->Es > 0) || !(p->H > 0)) return set_err(SSF_ERR_BAD_ARG, "ssf_metrics: Es and H must be positive");
    }
    return engine_call("ssf_metrics", device, [&](std::string *err) { return ssf::metrics_run(device, p, rx, tx, const_raw, const_norm, px, evm_w32, out, err); });
}

int ssf_pnorm(int device, int64_t count, int32_t dtype, const void *x, void *y) {
    if (!x || !y || count < 1 || metrics_bad_dtype(dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_pnorm: bad argument");
    return engine_call("ssf_pnorm", device, [&](std::string *err) { return ssf::metrics_pnorm(device, count, dtype, x, y, err); });
}

int ssf_signal_power(int device, int64_t count, int64_t rows, int32_t dtype, const void *x, double *out) {
    if (!x || !out || count < 1 || rows < 1 || count % rows || metrics_bad_dtype(dtype))
        return set_err(SSF_ERR_BAD_ARG, "ssf_signal_power: bad argument");
    return engine_call("ssf_signal_power", device, [&](std::string *err) { return ssf::metrics_power(device, count, rows, dtype, x, out, err); });
}

int ssf_demodulate(int device, int64_t count, int32_t dtype, int32_t M, const double *const_raw, const void *symb,
                   int32_t *bits_out) {
    if (!const_raw || !symb || !bits_out || count < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_demodulate: bad argument");
    if (metrics_bad_M(M) || metrics_bad_dtype(dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_demodulate: bad M or dtype");
    return engine_call("ssf_demodulate", device, [&](std::string *err) { return ssf::metrics_demod(device, count, dtype, M, const_raw, symb, bits_out, err); });
}

// ---- theoretical and Monte-Carlo mutual information (engine_theory.hip): every check comes before the first allocation or launch
static bool theory_bad_px(const double *px, int32_t M) {
    for (int m = 0; m < M; ++m)
        if (!(px[m] > 0) || !std::isfinite(px[m])) return true;
    return false;
}
static bool theory_bad_table(const double *tab, int32_t M) {
    for (int m = 0; m < 2 * M; ++m)
        if (!std::isfinite(tab[m])) return true;
    return false;
}

int ssf_theory_mi(int device, int32_t M, int32_t nS, const double *const_tab, const double *px, const double *sigma, double *mi_out) {
    if (!const_tab || !px || !sigma || !mi_out) return set_err(SSF_ERR_BAD_ARG, "ssf_theory_mi: NULL argument");
    if (M < 1 || M > 1024) return set_err(SSF_ERR_BAD_ARG, "ssf_theory_mi: M must be 1 .. 1024");
    if (nS < 1 || nS > 4096) return set_err(SSF_ERR_BAD_ARG, "ssf_theory_mi: nS must be 1 .. 4096");
    if (theory_bad_table(const_tab, M)) return set_err(SSF_ERR_BAD_ARG, "ssf_theory_mi: the table must be finite");
    if (theory_bad_px(px, M)) return set_err(SSF_ERR_BAD_ARG, "ssf_theory_mi: px must be finite and positive");
    for (int s = 0; s < nS; ++s)
        if (!(sigma[s] > 0) || !std::isfinite(sigma[s])) return set_err(SSF_ERR_BAD_ARG, "ssf_theory_mi: sigma must be finite and positive");
    return engine_call("ssf_theory_mi", device, [&](std::string *err) { return ssf::theory_mi(device, M, nS, const_tab, px, sigma, mi_out, err); });
}

int ssf_calc_mi(int device, int64_t n, int32_t dtype, int32_t M, double sigma2, const double *const_tab, const double *px, const void *rx,
                const void *tx, double *mi_out) {
    if (!const_tab || !px || !rx || !tx || !mi_out) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_mi: NULL argument");
    if (n < 1 || metrics_bad_dtype(dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_mi: bad n or dtype");
    if (M < 1 || M > 1024) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_mi: M must be 1 .. 1024");
    if (!(sigma2 > 0) || !std::isfinite(sigma2)) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_mi: sigma2 must be finite and positive");
    if (theory_bad_table(const_tab, M)) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_mi: the table must be finite");
    if (theory_bad_px(px, M)) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_mi: px must be finite and positive");
    return engine_call("ssf_calc_mi", device, [&](std::string *err) { return ssf::theory_calc_mi(device, n, dtype, M, sigma2, const_tab, px, rx, tx, mi_out, err); });
}

// ---- carrier phase recovery (engine_cpr.hip): every check comes before the first allocation or launch
static const char *cpr_bad_shape(int64_t n, int32_t nModes, int32_t dtype) {
    if (n < 2) return "n must be at least 2";
    if (nModes < 1 || nModes > 64) return "nModes must be 1 .. 64";
    if (dtype != SSF_M_C128 && dtype != SSF_M_C64) return "dtype must be complex128 or complex64";
    return nullptr;
}
static const char *cpr_bad_search(int32_t Nh, int32_t B, int32_t M) {
    if (M < 2 || M > 1024) return "M must be 2 .. 1024";
    if (B < 1 || B > 1024) return "B must be 1 .. 1024";
    if (Nh < 0 || Nh > 1023) return "the half window must be 0 .. 1023";
    return nullptr;
}
static bool cpr_bad_foe(int32_t P, double Fs) { return P < 1 || P > 1024 || !(Fs > 0) || !std::isfinite(Fs); }

int ssf_cpr(int device, const ssf_cpr_params *p, const double *const_tab, const void *x, void *sig_out, double *phase_out,
            double *fo_out) {
    if (!p || !const_tab || !x || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_cpr: NULL argument");
    if (const char *m = cpr_bad_shape(p->n, p->nModes, p->dtype)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_cpr: ") + m);
    if (const char *m = cpr_bad_search(p->Nh, p->B, p->M)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_cpr: ") + m);
    if (p->runFOE && cpr_bad_foe(p->P, p->Fs)) return set_err(SSF_ERR_BAD_ARG, "ssf_cpr: P must be 1 .. 1024 and Fs positive");
    return engine_call("ssf_cpr", device, [&](std::string *err) { return ssf::cpr_run(device, p, const_tab, x, sig_out, phase_out, fo_out, err); });
}

int ssf_bps(int device, int64_t n, int32_t nModes, int32_t dtype, int32_t Nh, int32_t B, int32_t M, const double *const_tab,
            const void *x, double *phase_out) {
    if (!const_tab || !x || !phase_out) return set_err(SSF_ERR_BAD_ARG, "ssf_bps: NULL argument");
    if (const char *m = cpr_bad_shape(n, nModes, dtype)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_bps: ") + m);
    if (const char *m = cpr_bad_search(Nh, B, M)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_bps: ") + m);
    return engine_call("ssf_bps", device, [&](std::string *err) { return ssf::cpr_bps(device, n, nModes, dtype, Nh, B, M, const_tab, x, phase_out, err); });
}

int ssf_foe(int device, int64_t n, int32_t nModes, int32_t dtype, int32_t P, double Fs, const void *x, void *sig_out,
            double *fo_out) {
    if (!x || !sig_out || !fo_out) return set_err(SSF_ERR_BAD_ARG, "ssf_foe: NULL argument");
    if (const char *m = cpr_bad_shape(n, nModes, dtype)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_foe: ") + m);
    if (cpr_bad_foe(P, Fs)) return set_err(SSF_ERR_BAD_ARG, "ssf_foe: P must be 1 .. 1024 and Fs positive");
    return engine_call("ssf_foe", device, [&](std::string *err) { return ssf::cpr_foe(device, n, nModes, dtype, P, Fs, x, sig_out, fo_out, err); });
}

// ---- sequence synchronisation (engine_sync.hip)
int ssf_symbol_sync(int device, const ssf_sync_params *p, const void *rx, const void *tx, void *out, ssf_sync_result *result) {
    if (!p || !rx || !tx || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: NULL argument");
    if (p->mode != SSF_SYNC_AMP && p->mode != SSF_SYNC_REAL) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: mode must be SSF_SYNC_AMP or SSF_SYNC_REAL");
    if (p->nModes < 1 || p->nModes > 8) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: nModes must be 1 .. 8");
    if (p->SpS < 1 || p->SpS * p->nModes > 256) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: SpS >= 1 and SpS * nModes <= 256");
    if (p->n_rx < 1 || p->n_rx % p->SpS) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: the length of rx is not a multiple of SpS");
    if (p->n_tx < 2 || p->n_rx / p->SpS < 2) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: at least 2 symbols on either side");
    if (p->n_tx > (1LL << 31) || p->n_rx > (1LL << 31)) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: at most 2^31 rows");
    for (int32_t d : {p->rx_dtype, p->tx_dtype})
        if (d != SSF_M_C128 && d != SSF_M_C64) return set_err(SSF_ERR_BAD_ARG, "ssf_symbol_sync: dtype must be complex128 or complex64");
    return engine_call("ssf_symbol_sync", device, [&](std::string *err) { return ssf::sync_run(device, p, rx, tx, out, result, err); });
}

int ssf_finddelay(int device, int64_t nx, int64_t ny, int32_t x_dtype, int32_t y_dtype, const void *x, const void *y, int64_t *delay_out) {
    if (!x || !y || !delay_out) return set_err(SSF_ERR_BAD_ARG, "ssf_finddelay: NULL argument");
    if (nx < 1 || ny < 1 || nx > (1LL << 31) || ny > (1LL << 31)) return set_err(SSF_ERR_BAD_ARG, "ssf_finddelay: lengths must be 1 .. 2^31");
    for (int32_t d : {x_dtype, y_dtype})
        if (d < SSF_M_C128 || d > SSF_M_F32) return set_err(SSF_ERR_BAD_ARG, "ssf_finddelay: unknown dtype");
    return engine_call("ssf_finddelay", device, [&](std::string *err) { return ssf::sync_finddelay(device, nx, ny, x_dtype, y_dtype, x, y, delay_out, err); });
}

int ssf_sync_transform_time(int device, int64_t L, int32_t nseq, int32_t nslots, int32_t nslots2, int32_t reps, double *seconds_out) {
    if (!seconds_out) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_transform_time: NULL argument");
    if (L < 4 || L > (1LL << 32) || (L & (L - 1))) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_transform_time: L must be a power of two, 4 .. 2^32");
    if (nseq < 1 || nseq > 24 || nslots < 1 || nslots > 64 || nslots2 < 0 || nslots2 > nslots || reps < 1 || reps > 1000)
        return set_err(SSF_ERR_BAD_ARG, "ssf_sync_transform_time: 1 <= nseq <= 24, 0 <= nslots2 <= nslots <= 64, 1 <= reps <= 1000");
    return engine_call("ssf_sync_transform_time", device, [&](std::string *err) {
        return ssf::sync_transform_time(device, L, nseq, nslots, nslots2, reps, seconds_out, err);
    });
}

// ---- adaptive MIMO equalizer (engine_eq.hip): every check comes before the first allocation or launch
static const char *eq_bad(const ssf_eq_params *p, const ssf_eq_stage *st, const void *ref) {
    if (p->nModes < 1 || p->nModes > 4) return "nModes must be 1 .. 4";
    if (p->nTaps < 1 || p->nTaps > 64) return "nTaps must be 1 .. 64";
    if (p->SpS < 1 || p->SpS > 8) return "SpS must be 1 .. 8";
    if (p->n < p->nTaps) return "n must be at least nTaps";
    if (p->dtype != SSF_M_C128 && p->dtype != SSF_M_C64) return "dtype must be complex128 or complex64";
    if (p->total != (p->n + 2 * (p->nTaps / 2) - p->nTaps) / p->SpS + 1) return "total must be (n + 2 (nTaps / 2) - nTaps) / SpS + 1";
    if (p->M < 2 || p->M > 1024) return "M must be 2 .. 1024";
    if (p->nRadii < 1 || p->nRadii > 1024) return "nRadii must be 1 .. 1024";
    if (p->numIter < 1) return "numIter must be at least 1";
    if (p->nStages < 1) return "nStages must be at least 1";
    if (!std::isfinite(p->Rcma)) return "Rcma must be finite";
    int64_t sum = 0;
    bool aided = false;
    for (int s = 0; s < p->nStages; ++s) {
        if (st[s].alg < SSF_EQ_NLMS || st[s].alg > SSF_EQ_STATIC) return "unknown algorithm";
        if (st[s].L < 1 || st[s].L > p->total - sum) return "every stage needs L >= 1 and their sum at most total";
        if (!std::isfinite(st[s].mu)) return "mu must be finite";
        sum += st[s].L;
        aided = aided || st[s].alg == SSF_EQ_NLMS || st[s].alg == SSF_EQ_DARDE;
    }
    if (aided && !ref) return "a data-aided stage needs ref";
    if (ref && p->ref_dtype != SSF_M_C128 && p->ref_dtype != SSF_M_C64) return "ref_dtype must be complex128 or complex64";
    if (ref && p->nref < (aided ? sum : 1)) return "ref must have at least as many rows as the stages have symbols";
    return nullptr;
}

int ssf_mimo_eq(int device, const ssf_eq_params *p, const ssf_eq_stage *stages, const double *const_tab, const double *radii_tab,
                void *H_inout, const void *x, const void *ref, void *sig_out, double *errsq_out) {
    if (!p || !stages || !const_tab || !radii_tab || !H_inout || !x || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_mimo_eq: NULL argument");
    if (const char *m = eq_bad(p, stages, ref)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_mimo_eq: ") + m);
    return engine_call("ssf_mimo_eq", device, [&](std::string *err) {
        return ssf::eq_run(device, p, stages, const_tab, radii_tab, H_inout, x, ref, sig_out, errsq_out, err);
    });
}

// ---- ffe, dfe, volterra, anorm (engine_siso.hip): every check comes before the first allocation or launch
static const char *siso_bad(const ssf_siso_params *p, const void *ref) {
    if (p->kind < SSF_SISO_FFE || p->kind > SSF_SISO_ANORM) return "unknown kind";
    if (p->n < 1) return "n must be at least 1";
    if (metrics_bad_dtype(p->dtype)) return "unknown dtype";
    if (p->kind == SSF_SISO_ANORM) return nullptr;
    const bool cx = p->dtype == SSF_M_C128 || p->dtype == SSF_M_C64;
    if (p->mode != SSF_SISO_DATA_AIDED && p->mode != SSF_SISO_FULLTIME) return "unknown mode";
    if (p->nTaps < 1 || p->nTaps > 256) return "nTaps must be 1 .. 256";
    if (p->SpS < 1 || p->SpS > 8 || p->SpS > p->nTaps) return "SpS must be 1 .. 8 and at most nTaps";
    if (p->n < p->SpS) return "n must be at least SpS";
    if (p->M < 2 || p->M > 1024) return "M must be 2 .. 1024";
    if (p->preconvIters < 1 || p->nTrain < 0) return "preconvIters >= 1 and nTrain >= 0";
    if (!std::isfinite(p->mu)) return "mu must be finite";
    int64_t ncoef = p->nTaps;
    if (p->kind == SSF_SISO_DFE) {
        if (p->nFB < 0 || p->nFB > 256) return "nFB must be 0 .. 256";
        ncoef += p->nFB;
    } else if (p->kind == SSF_SISO_VOLTERRA) {
        if (cx) return "volterra takes real data";
        if (p->order != 2 && p->order != 3) return "order must be 2 or 3";
        if (p->n2 < 1 || p->n3 < 1 || p->n2 > p->nTaps || p->n3 > p->nTaps) return "n2 and n3 must be 1 .. nTaps";
        ncoef += (int64_t)p->n2 * p->n2 + (p->order == 3 ? (int64_t)p->n3 * p->n3 * p->n3 : 0);
    }
    if (ncoef > 1536) return "more than 1536 coefficients";
    if (p->ncoef != ncoef) return "ncoef does not match the geometry";
    const int64_t N = p->n / p->SpS;
    if (p->nref < (p->nTrain < N ? p->nTrain : N)) return "ref must hold min(nTrain, N) values";
    if (p->nref > 0) {
        if (!ref) return "ref is NULL";
        if (metrics_bad_dtype(p->ref_dtype)) return "unknown ref_dtype";
        if (cx != (p->ref_dtype == SSF_M_C128 || p->ref_dtype == SSF_M_C64)) return "x and ref must both be real or both complex";
    }
    return nullptr;
}

int ssf_siso_eq(int device, ssf_siso_params *p, const double *const_tab, void *coef_inout, const void *x, const void *ref,
                void *sig_out, double *mse_out) {
    if (!p || !x || !sig_out) return set_err(SSF_ERR_BAD_ARG, "ssf_siso_eq: NULL argument");
    if (const char *m = siso_bad(p, ref)) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_siso_eq: ") + m);
    if (p->kind != SSF_SISO_ANORM && (!const_tab || !coef_inout || !mse_out)) return set_err(SSF_ERR_BAD_ARG, "ssf_siso_eq: NULL argument");
    return engine_call("ssf_siso_eq", device, [&](std::string *err) { return ssf::siso_run(device, p, const_tab, coef_inout, x, ref, sig_out, mse_out, err); });
}

// ---- mlse, detector, autocorr (engine_seqdet.hip): every check comes before the first allocation or launch
int ssf_mlse(int device, ssf_mlse_params *p, const double *h, const double *const_tab, const void *y, void *out, double *final_metric) {
    if (!p || !h || !const_tab || !y || !out || !final_metric) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: NULL argument");
    if (p->dtype != SSF_M_F64 && p->dtype != SSF_M_C128) return set_err(SSF_ERR_UNSUPPORTED, "ssf_mlse: float64 or complex128 arrays");
    if (p->M < 1 || p->M > 64) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: M must be 1 .. 64");
    if (p->taps < 1 || p->taps > 11) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: 1 .. 11 taps");
    int64_t states = 1;
    for (int i = 1; i < p->taps && states <= 1024; ++i) states *= p->M;
    if (states > 1024) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: more than 1024 states");
    if (p->cols < 1 || p->cols > 64) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: 1 .. 64 columns");
    if (p->n < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: n must be at least 1");
    if (p->n > ((int64_t)1 << 31)) return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: survivor memory above 2^31 bytes");
    const int64_t bytes = ssf::mlse_survivor_bytes(p->n, p->cols, p->M, p->taps);
    if (bytes > ((int64_t)1 << 31))
        return set_err(SSF_ERR_BAD_ARG, "ssf_mlse: survivor memory of " + std::to_string(bytes) + " bytes is above 2^31 bytes");
    return engine_call("ssf_mlse", device, [&](std::string *err) { return ssf::mlse_run(device, p, h, const_tab, y, out, final_metric, err); });
}

int ssf_detector(int device, int64_t n, int32_t dtype, int32_t M, int32_t rule, double sigma2, const double *const_tab, const double *logpx,
                 const void *r, void *decided, int64_t *ind) {
    if (!const_tab || !r || !decided || !ind) return set_err(SSF_ERR_BAD_ARG, "ssf_detector: NULL argument");
    if (rule != SSF_DET_ML && rule != SSF_DET_MAP) return set_err(SSF_ERR_BAD_ARG, "ssf_detector: unknown rule");
    if (rule == SSF_DET_MAP && !logpx) return set_err(SSF_ERR_BAD_ARG, "ssf_detector: NULL argument");
    if (dtype != SSF_M_F64 && dtype != SSF_M_C128) return set_err(SSF_ERR_UNSUPPORTED, "ssf_detector: float64 or complex128 arrays");
    if (M < 1 || M > 64) return set_err(SSF_ERR_BAD_ARG, "ssf_detector: M must be 1 .. 64");
    if (n < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_detector: n must be at least 1");
    if (rule == SSF_DET_MAP && !(sigma2 > 0)) return set_err(SSF_ERR_BAD_ARG, "ssf_detector: sigma2 must be positive");
    return engine_call("ssf_detector", device, [&](std::string *err) {
        return ssf::detector_run(device, n, dtype, M, rule, sigma2, const_tab, logpx, r, decided, ind, err);
    });
}

int ssf_autocorr(int device, int64_t n, int32_t nTaps, const void *x, double *r_out) {
    if (!x || !r_out) return set_err(SSF_ERR_BAD_ARG, "ssf_autocorr: NULL argument");
    if (nTaps < 1 || nTaps > 256) return set_err(SSF_ERR_BAD_ARG, "ssf_autocorr: nTaps must be 1 .. 256");
    if (n < nTaps) return set_err(SSF_ERR_BAD_ARG, "ssf_autocorr: nTaps exceeds n");
    return engine_call("ssf_autocorr", device, [&](std::string *err) { return ssf::autocorr_run(device, n, nTaps, x, r_out, err); });
}

// ---- syncDataSequences' glue, movingAverage, bert (engine_syncdata.hip): every check comes before the first allocation or launch
int ssf_sync_tile(int device, const ssf_sync_tile_params *p, const void *rx, const void *tx, void *rx_out, void *tx_out) {
    if (!p || !rx || !tx || !rx_out || !tx_out) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_tile: NULL argument");
    if (p->nModes < 1 || p->nModes > 8) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_tile: nModes must be 1 .. 8");
    if (p->SpS < 1 || p->n_rx < 1 || p->n_tx < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_tile: SpS, n_rx and n_tx must be at least 1");
    if (p->n_pad < p->n_rx || p->n_pad > (1LL << 31)) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_tile: n_rx <= n_pad <= 2^31");
    for (int32_t d : {p->rx_dtype, p->tx_dtype})
        if (d != SSF_M_C128 && d != SSF_M_C64 && d != SSF_M_F64) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_tile: dtype must be complex128, complex64 or float64");
    return engine_call("ssf_sync_tile", device, [&](std::string *err) { return ssf::syncdata_tile(device, p, rx, tx, rx_out, tx_out, err); });
}

int ssf_sync_extract(int device, int64_t n, int32_t nModes, int64_t n_out, int32_t out_dtype, int32_t normalize, const void *x, void *out,
                     int64_t *kept) {
    if (!x || !out || !kept) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_extract: NULL argument");
    if (nModes < 1 || nModes > 8) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_extract: nModes must be 1 .. 8");
    if (n < 1 || n > (1LL << 31) || n_out < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_extract: 1 <= n <= 2^31 and n_out >= 1");
    if (out_dtype != SSF_M_C128 && out_dtype != SSF_M_F64) return set_err(SSF_ERR_BAD_ARG, "ssf_sync_extract: out_dtype must be complex128 or float64");
    return engine_call("ssf_sync_extract", device, [&](std::string *err) {
        return ssf::syncdata_extract(device, n, nModes, n_out, out_dtype, normalize != 0, x, out, kept, err);
    });
}

int ssf_real_part(int device, int64_t count, const void *x, void *out) {
    if (!x || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_real_part: NULL argument");
    if (count < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_real_part: count must be at least 1");
    return engine_call("ssf_real_part", device, [&](std::string *err) { return ssf::syncdata_real_part(device, count, x, out, err); });
}

int ssf_copy_columns(int device, int64_t n, int32_t width, int32_t src_cols, int32_t src_first, int32_t dst_cols, int32_t dst_first, const void *src,
                     void *dst) {
    if (!src || !dst) return set_err(SSF_ERR_BAD_ARG, "ssf_copy_columns: NULL argument");
    if (n < 1 || n > (1LL << 40) || width < 1 || src_first < 0 || dst_first < 0 || src_first + (int64_t)width > src_cols || dst_first + (int64_t)width > dst_cols)
        return set_err(SSF_ERR_BAD_ARG, "ssf_copy_columns: n >= 1 and the block of columns inside both arrays");
    if (src == dst) return set_err(SSF_ERR_BAD_ARG, "ssf_copy_columns: src and dst must be different arrays");
    if (!ssf::on_device(src) || !ssf::on_device(dst)) return set_err(SSF_ERR_BAD_ARG, "ssf_copy_columns: src and dst are device arrays");
    return engine_call("ssf_copy_columns", device, [&](std::string *err) {
        return ssf::syncdata_copy_columns(device, n, width, src_cols, src_first, dst_cols, dst_first, src, dst, err);
    });
}

int ssf_moving_average(int device, int64_t n, int32_t cols, int32_t N, int32_t dtype, const void *x, void *out) {
    if (!x || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_moving_average: NULL argument");
    if (N < 2 || N > 2048) return set_err(SSF_ERR_BAD_ARG, "ssf_moving_average: N must be 2 .. 2048");
    if (n < 1 || cols < 1 || cols > 65535) return set_err(SSF_ERR_BAD_ARG, "ssf_moving_average: n >= 1 and 1 <= cols <= 65535");
    if (dtype != SSF_M_C128 && dtype != SSF_M_C64 && dtype != SSF_M_F64) return set_err(SSF_ERR_BAD_ARG, "ssf_moving_average: dtype must be complex128, complex64 or float64");
    return engine_call("ssf_moving_average", device, [&](std::string *err) { return ssf::syncdata_moving_average(device, n, cols, N, dtype, x, out, err); });
}

int ssf_bert(int device, int64_t n, const void *irx, const void *bits, double *scal_out) {
    if (!irx || !bits || !scal_out) return set_err(SSF_ERR_BAD_ARG, "ssf_bert: NULL argument");
    if (n < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_bert: n must be at least 1");
    return engine_call("ssf_bert", device, [&](std::string *err) { return ssf::syncdata_bert(device, n, irx, bits, scal_out, err); });
}

// ---- soft-decision FEC (engine_fec.hip): every check comes before the first allocation, upload or launch
int ssf_calc_llr(int device, int64_t n, int32_t dtype, int32_t M, double sigma2, const double *const_tab, const int32_t *bitmap,
                 const double *px, const void *x, double *llr_out) {
    if (!const_tab || !bitmap || !px || (n > 0 && (!x || !llr_out))) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_llr: NULL argument");
    if (n < 0) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_llr: n must not be negative");
    if (dtype != SSF_M_C128 && dtype != SSF_M_C64) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_llr: dtype must be complex128 or complex64");
    if (M < 2 || M > 1024 || (M & (M - 1))) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_llr: M must be a power of two, 2 .. 1024");
    if (!(sigma2 > 0) || !std::isfinite(sigma2)) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_llr: sigma2 must be positive");
    int b = 0;
    while ((1 << b) < M) ++b;
    for (int i = 0; i < M * b; ++i)
        if (bitmap[i] != 0 && bitmap[i] != 1) return set_err(SSF_ERR_BAD_ARG, "ssf_calc_llr: bitmap must hold 0 and 1 only");
    return engine_call("ssf_calc_llr", device, [&](std::string *err) { return ssf::fec_calc_llr(device, n, dtype, M, sigma2, const_tab, bitmap, px, x, llr_out, err); });
}

// the kernels index with these arrays unchecked: nothing that could send them out of bounds, or two threads to one edge, gets in
static const char *ldpc_graph_bad(int m, int n, int E, const int32_t *co, const int32_t *ev, const int32_t *vo, const int32_t *ve,
                                  int *max_dc) {
    if (m < 1 || n < 1 || E < 1) return "m, n and E must be positive";
    if (co[0] != 0 || co[m] != E) return "check_offsets must run from 0 to E";
    if (vo[0] != 0 || vo[n] != E) return "var_offsets must run from 0 to E";
    *max_dc = 0;
    for (int c = 0; c < m; ++c) {
        const int64_t d = (int64_t)co[c + 1] - co[c];
        if (d < 1) return "every check needs at least one edge and check_offsets must rise";
        if (d > 64) return "a check has more than 64 edges";
        if (co[c + 1] > E) return "check_offsets must run from 0 to E";
        if (d > *max_dc) *max_dc = (int)d;
    }
    for (int e = 0; e < E; ++e)
        if (ev[e] < 0 || ev[e] >= n) return "edge_var holds an index outside 0 .. n - 1";
    std::vector<unsigned char> seen((size_t)E, 0);
    for (int v = 0; v < n; ++v) {
        const int64_t d = (int64_t)vo[v + 1] - vo[v];
        if (d < 0 || vo[v + 1] > E) return "var_offsets must rise from 0 to E";
        if (d > 64) return "a variable has more than 64 edges";
        for (int k = vo[v]; k < vo[v + 1]; ++k) {
            const int e = ve[k];
            if (e < 0 || e >= E || ev[e] != v || seen[(size_t)e]) return "var_edge_indices must list every variable's own edges once";
            seen[(size_t)e] = 1;
        }
    }
    return nullptr;
}

int ssf_ldpc_graph_create(int device, int32_t m, int32_t n, int32_t E, const int32_t *check_offsets, const int32_t *edge_var,
                          const int32_t *var_offsets, const int32_t *var_edge_indices, ssf_ldpc_graph **out) {
    if (!check_offsets || !edge_var || !var_offsets || !var_edge_indices || !out)
        return set_err(SSF_ERR_BAD_ARG, "ssf_ldpc_graph_create: NULL argument");
    *out = nullptr;
    int max_dc = 0;
    if (const char *msg = ldpc_graph_bad(m, n, E, check_offsets, edge_var, var_offsets, var_edge_indices, &max_dc))
        return set_err(SSF_ERR_BAD_ARG, std::string("ssf_ldpc_graph_create: ") + msg);
    return engine_call("ssf_ldpc_graph_create", device, [&](std::string *err) {
        return ssf::fec_graph_create(device, m, n, E, check_offsets, edge_var, var_offsets, var_edge_indices, max_dc, out, err);
    });
}

int ssf_ldpc_graph_destroy(ssf_ldpc_graph *graph) {
    if (!graph) return SSF_OK;
    return engine_result("ssf_ldpc_graph_destroy", [&](std::string *err) { return ssf::fec_graph_destroy(graph, err); });
}

int ssf_ldpc_decode(int device, const ssf_ldpc_graph *graph, const ssf_ldpc_params *p, const void *llr_in, void *llr_out,
                    int8_t *bits_out, int8_t *fail_out, uint32_t *iter_out) {
    if (!graph || !p || !llr_in || !llr_out || !bits_out || !fail_out) return set_err(SSF_ERR_BAD_ARG, "ssf_ldpc_decode: NULL argument");
    const char *msg = nullptr;
    if (p->n_ < 1 || p->n_ > graph->n) msg = "n_ must be 1 .. n";
    else if (p->numCodewords < 1 || p->numCodewords > 65535) msg = "numCodewords must be 1 .. 65535";
    else if (p->maxIter < 1 || p->maxIter > 65535) msg = "maxIter must be 1 .. 65535";
    else if (p->alg != SSF_FEC_SPA && p->alg != SSF_FEC_MSA) msg = "alg must be SSF_FEC_SPA or SSF_FEC_MSA";
    else if (p->prec != SSF_FEC_F64 && p->prec != SSF_FEC_F32) msg = "prec must be SSF_FEC_F64 or SSF_FEC_F32";
    else if (p->in_dtype != SSF_FEC_F64 && p->in_dtype != SSF_FEC_F32) msg = "in_dtype must be SSF_FEC_F64 or SSF_FEC_F32";
    else if (p->engine < SSF_FEC_AUTO || p->engine > SSF_FEC_GLOBAL) msg = "unknown engine";
    else if (p->sync_every < 0) msg = "sync_every must not be negative";
    else if (device != graph->device) msg = "the graph lives on another device";
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_ldpc_decode: ") + msg);
    return engine_call("ssf_ldpc_decode", device, [&](std::string *err) {
        return ssf::fec_decode(device, graph, p, llr_in, llr_out, bits_out, fail_out, iter_out, err);
    });
}

// ---- LDPC encoding and Gray mapping (engine_enc.hip): the kernels index with the CSR unchecked, so nothing out of range gets in
static const char *encoder_bad(const ssf_ldpc_encoder_desc *d, const uint64_t *block1, const uint64_t *block2, const int32_t *indptr,
                               const int32_t *indices) {
    if (d->k < 1 || d->m1 < 1 || d->m2 < 0) return "k and m1 must be positive, m2 not negative";
    if (d->form == SSF_ENC_DENSE) {
        if (d->k > 32768) return "the dense form takes k <= 32768";
        if ((int64_t)d->m1 + d->m2 > (1 << 24)) return "too many parity rows";
        if (!block1 || (d->m2 > 0 && !block2)) return "NULL parity block";
        return nullptr;
    }
    if (d->form != SSF_ENC_SPARSE) return "form must be SSF_ENC_DENSE or SSF_ENC_SPARSE";
    if (d->k > 131072 || d->m1 > 262144) return "the sparse form takes k <= 131072 and m1 <= 262144";
    if (d->m2 != 0 || d->nnz < 0 || !indptr || (d->nnz > 0 && !indices)) return "the sparse form needs indptr, indices and m2 = 0";
    if (indptr[0] != 0 || indptr[d->m1] != d->nnz) return "indptr must run from 0 to nnz";
    for (int i = 0; i < d->m1; ++i)
        if (indptr[i + 1] < indptr[i] || indptr[i + 1] > d->nnz) return "indptr must rise from 0 to nnz";
    for (int e = 0; e < d->nnz; ++e)
        if (indices[e] < 0 || indices[e] >= d->k) return "indices holds a column outside 0 .. k - 1";
    return nullptr;
}

int ssf_ldpc_encoder_create(int device, const ssf_ldpc_encoder_desc *desc, const uint64_t *block1, const uint64_t *block2,
                            const int32_t *indptr, const int32_t *indices, ssf_ldpc_encoder **out) {
    if (!desc || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_ldpc_encoder_create: NULL argument");
    *out = nullptr;
    if (const char *msg = encoder_bad(desc, block1, block2, indptr, indices))
        return set_err(SSF_ERR_BAD_ARG, std::string("ssf_ldpc_encoder_create: ") + msg);
    return engine_call("ssf_ldpc_encoder_create", device, [&](std::string *err) { return ssf::enc_create(device, desc, block1, block2, indptr, indices, out, err); });
}

int ssf_ldpc_encoder_destroy(ssf_ldpc_encoder *encoder) {
    if (!encoder) return SSF_OK;
    return engine_result("ssf_ldpc_encoder_destroy", [&](std::string *err) { return ssf::enc_destroy(encoder, err); });
}

int ssf_ldpc_encode(int device, const ssf_ldpc_encoder *encoder, const ssf_ldpc_encode_params *p, const void *bits_in,
                    void *codewords_out) {
    if (!encoder || !p || !bits_in || !codewords_out) return set_err(SSF_ERR_BAD_ARG, "ssf_ldpc_encode: NULL argument");
    const int64_t full = (int64_t)encoder->rows + (encoder->form == SSF_ENC_SPARSE || encoder->systematic ? encoder->k : 0);
    const char *msg = nullptr;
    if (p->numCodewords < 1 || p->numCodewords > 65535) msg = "numCodewords must be 1 .. 65535";
    else if (p->n < 1 || p->n > full) msg = "n must be 1 .. the codeword's length";
    else if (device != encoder->device) msg = "the encoder lives on another device";
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_ldpc_encode: ") + msg);
    return engine_call("ssf_ldpc_encode", device, [&](std::string *err) { return ssf::enc_encode(device, encoder, p, bits_in, codewords_out, err); });
}

int ssf_modulate(int device, int64_t nsymb, int32_t M, const double *const_tab, const void *bits, void *symb_out) {
    if (!const_tab || !bits || !symb_out || nsymb < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_modulate: bad argument");
    if (M < 2 || M > 1024 || (M & (M - 1))) return set_err(SSF_ERR_BAD_ARG, "ssf_modulate: M must be a power of two, 2 .. 1024");
    return engine_call("ssf_modulate", device, [&](std::string *err) { return ssf::enc_modulate(device, nsymb, M, const_tab, bits, symb_out, err); });
}

// ---- OFDM (engine_ofdm.hip): the kernels index with the carrier tables unchecked, so nothing out of range gets in
static const char *ofdm_bad(const ssf_ofdm_params *p, bool mod) {
    if (p->nframes < 1) return "nframes must be positive";
    if (p->Nfft < 4 || p->Nfft > (1 << 20)) return "Nfft must be 4 .. 2^20";
    if (p->G < 0 || p->G > p->Nfft) return "G must be 0 .. Nfft";
    if (mod && (p->SpS < 1 || p->SpS > 64)) return "SpS must be 1 .. 64";
    if (p->Ns < 1 || p->Ns > p->Nfft) return "Ns must be 1 .. Nfft";
    if (p->Np < 0 || p->Np == 1) return "Np must be 0 or at least 2";
    if (p->Ni < 1 || (int64_t)p->Ni + p->Np > p->Ns) return "Ni must be 1 .. Ns - Np";
    if ((p->in_dtype != SSF_C64 && p->in_dtype != SSF_C128) || (mod && p->out_dtype != SSF_C64 && p->out_dtype != SSF_C128))
        return "dtype must be SSF_C64 or SSF_C128";
    if (p->route != SSF_OFDM_AUTO && p->route != SSF_OFDM_ROCFFT) return "route must be SSF_OFDM_AUTO or SSF_OFDM_ROCFFT";
    if (p->nframes * (mod ? p->SpS : 1) * (int64_t)p->Nfft >= (1ll << 31)) return "nframes * SpS * Nfft must stay below 2^31";
    if (p->Np > 0 && p->pilot_re == 0.0 && p->pilot_im == 0.0) return "the pilot symbol must not be zero";
    return nullptr;
}

int ssf_ofdm_modulate(int device, const ssf_ofdm_params *p, const int32_t *src_map, const void *symb, void *out) {
    if (!p || !src_map || !symb || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_ofdm_modulate: NULL argument");
    const char *msg = ofdm_bad(p, true);
    for (int64_t k = 0; !msg && k < (int64_t)p->SpS * p->Nfft; ++k) {
        const int32_t code = src_map[k], kind = code & 3;
        if (code < 0 || kind == 3 || (kind != 1 && (code >> 3) != 0) || (kind == 0 && code != 0) || (kind == 1 && (code >> 3) >= p->Ni))
            msg = "src_map holds a code that names no source";
    }
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_ofdm_modulate: ") + msg);
    return engine_call("ssf_ofdm_modulate", device, [&](std::string *err) { return ssf::ofdm_modulate(device, p, src_map, symb, out, err); });
}

int ssf_ofdm_demodulate(int device, const ssf_ofdm_params *p, const int32_t *bin_carrier, const int32_t *data_carriers,
                        const int32_t *pilot_carriers, const int32_t *pilot_hi, const void *sig, void *symb_out, void *H_out) {
    if (!p || !bin_carrier || !data_carriers || !sig || !symb_out) return set_err(SSF_ERR_BAD_ARG, "ssf_ofdm_demodulate: NULL argument");
    const char *msg = ofdm_bad(p, false);
    if (!msg && p->Np > 0 && (!pilot_carriers || !pilot_hi)) msg = "pilots need pilot_carriers and pilot_hi";
    for (int k = 0; !msg && k < p->Nfft; ++k)
        if (bin_carrier[k] < -1 || bin_carrier[k] >= p->Ns) msg = "bin_carrier holds a carrier outside -1 .. Ns - 1";
    for (int d = 0; !msg && d < p->Ni; ++d)
        if (data_carriers[d] < 0 || data_carriers[d] >= p->Ns) msg = "data_carriers holds a carrier outside 0 .. Ns - 1";
    for (int j = 0; !msg && j < p->Np; ++j)
        if (pilot_carriers[j] < 0 || pilot_carriers[j] >= p->Ns || (j > 0 && pilot_carriers[j] <= pilot_carriers[j - 1]))
            msg = "pilot_carriers must rise strictly inside 0 .. Ns - 1";
    for (int c = 0; !msg && p->Np > 0 && c < p->Ns; ++c)
        if (pilot_hi[c] < 1 || pilot_hi[c] >= p->Np) msg = "pilot_hi holds a segment outside 1 .. Np - 1";
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_ofdm_demodulate: ") + msg);
    return engine_call("ssf_ofdm_demodulate", device, [&](std::string *err) {
        return ssf::ofdm_demodulate(device, p, bin_carrier, data_carriers, pilot_carriers, pilot_hi, sig, symb_out, H_out, err);
    });
}

// ---- perturbation model (engine_nlin.hip): the kernels index LDS and the symbols with m and n unchecked, so nothing out of range gets in
int ssf_pert_nlin(int device, const ssf_nlin_params *p, const int32_t *pass, const double *coef, const int32_t *nidx,
                  const int32_t *phase_m, const double *phase_c, const void *x, const void *y, void *out0, void *out1, void *out2,
                  void *out3) {
    if (!p || !x || !out0) return set_err(SSF_ERR_BAD_ARG, "ssf_pert_nlin: NULL argument");
    const char *msg = nullptr;
    const int64_t L = p->L, W = 2 * L + 1;
    if (p->n < 1 || p->n > (1ll << 32)) msg = "n must be 1 .. 2^32";
    else if (L < 1 || L > 128) msg = "L must be 1 .. 128";
    else if (p->npass < 0 || p->npass > W + 2 || p->ncoef < 0 || p->ncoef > (W + 2) * W || p->nphase < 0 || p->nphase > W)
        msg = "npass, ncoef or nphase outside what a matrix of order 2L + 1 gives";
    else if (p->dense != 0 && p->dense != 1) msg = "dense must be 0 or 1";
    else if (p->entry != SSF_NLIN_CALC && p->entry != SSF_NLIN_FIELD) msg = "entry must be SSF_NLIN_CALC or SSF_NLIN_FIELD";
    else if ((p->in_dtype != SSF_C64 && p->in_dtype != SSF_C128) || (p->prec != SSF_C64 && p->prec != SSF_C128))
        msg = "dtype must be SSF_C64 or SSF_C128";
    else if (p->ispm_offset < -L || p->ispm_offset > L) msg = "ispm_offset must be -L .. L";
    else if (!std::isfinite(p->ispm_re) || !std::isfinite(p->ispm_im) || !std::isfinite(p->peak_power) || p->peak_power < 0.0)
        msg = "ispm and peak_power must be finite, peak_power not negative";
    else if (p->entry == SSF_NLIN_CALC && (!y || !out1 || !out2 || !out3)) msg = "SSF_NLIN_CALC needs y and four outputs";
    else if ((p->npass && !pass) || (p->ncoef && !coef) || (p->ncoef && !p->dense && !nidx) || (p->nphase && (!phase_m || !phase_c)))
        msg = "a table is missing";
    for (int k = 0; !msg && k < p->npass; ++k) {
        const int32_t kind = pass[4 * k], m = pass[4 * k + 1], first = pass[4 * k + 2], count = pass[4 * k + 3];
        if (kind < 0 || kind > 2 || m < -L || m > L || (kind != 0 && m != 0)) msg = "pass holds a kind or an m out of range";
        else if (first < 0 || count < 1 || (int64_t)first + count > p->ncoef) msg = "pass names coefficients outside coef";
        else if (p->dense && count != W) msg = "a dense pass needs 2L + 1 coefficients";
        else if (count > W) msg = "a pass holds more than 2L + 1 coefficients";           // its LDS slice holds no more
        for (int32_t j = 0; !msg && !p->dense && j < count; ++j) {
            if (nidx[first + j] < -L || nidx[first + j] > L) msg = "nidx holds an n outside -L .. L";
            else if (j > 0 && nidx[first + j] <= nidx[first + j - 1]) msg = "the n of a pass must rise strictly";
        }
    }
    for (int k = 0; !msg && k < p->nphase; ++k)
        if (phase_m[k] < -L || phase_m[k] > L) msg = "phase_m holds an m outside -L .. L";
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_pert_nlin: ") + msg);
    return engine_call("ssf_pert_nlin", device, [&](std::string *err) {
        return ssf::nlin_run(device, p, pass, coef, nidx, phase_m, phase_c, x, y, out0, out1, out2, out3, err);
    });
}

// ---- the sampling clock (engine_clock.hip): every check comes before the first allocation, upload or launch
static bool clock_bad_dtype(int32_t d) { return d < SSF_M_C128 || d > SSF_M_F32; }
static bool clock_bad_table(double qmin, double qdelta, int64_t levels) {
    return !std::isfinite(qmin) || !std::isfinite(qdelta) || !(qdelta > 0.0) || levels < 1;
}

int ssf_clock_interp(int device, const ssf_clock_params *p, const void *x, const double *t_re, const double *t_im, void *out) {
    if (!p || !x || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_clock_interp: NULL argument");
    const char *msg = nullptr;
    const bool cplx = p->dtype == SSF_M_C128 || p->dtype == SSF_M_C64;
    if (clock_bad_dtype(p->dtype)) msg = "unknown dtype";
    else if (p->n_in < 1 || p->n_out < 0 || p->ncols < 1 || p->n_in > (1LL << 40) || p->n_out > (1LL << 40)) msg = "sizes out of range";
    else if (p->form < SSF_CLOCK_REAL || p->form > SSF_CLOCK_COMPONENTS || cplx != (p->form != SSF_CLOCK_REAL)) msg = "form does not fit dtype";
    else if (!(p->inTs > 0.0) || !(p->outTs > 0.0) || !std::isfinite(p->inTs) || !std::isfinite(p->outTs)) msg = "inTs and outTs must be positive";
    else if (t_im && (!t_re || p->form != SSF_CLOCK_COMPONENTS)) msg = "t_im needs t_re and SSF_CLOCK_COMPONENTS";
    else if (p->clip && !(p->lo <= p->hi)) msg = "clip needs lo <= hi";
    else if (p->quantize && clock_bad_table(p->qmin, p->qdelta, p->qlevels)) msg = "bad quantizer table";
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_clock_interp: ") + msg);
    if (p->n_out == 0) return SSF_OK;
    return engine_call("ssf_clock_interp", device, [&](std::string *err) { return ssf::clock_interp(device, p, x, t_re, t_im, out, err); });
}

int ssf_quantize(int device, int64_t count, int32_t dtype, double qmin, double qdelta, int64_t qlevels, const void *x, double *out) {
    if (!x || !out || count < 1 || clock_bad_dtype(dtype) || clock_bad_table(qmin, qdelta, qlevels))
        return set_err(SSF_ERR_BAD_ARG, "ssf_quantize: bad argument");
    return engine_call("ssf_quantize", device, [&](std::string *err) { return ssf::clock_quantize(device, count, dtype, qmin, qdelta, qlevels, x, out, err); });
}

int ssf_clip(int device, int64_t count, int32_t dtype, double lo, double hi, const void *x, void *out) {
    if (!x || !out || count < 1 || clock_bad_dtype(dtype) || !(lo <= hi)) return set_err(SSF_ERR_BAD_ARG, "ssf_clip: bad argument");
    return engine_call("ssf_clip", device, [&](std::string *err) { return ssf::clock_clip(device, count, dtype, lo, hi, x, out, err); });
}

int ssf_minmax(int device, int64_t count, int32_t dtype, const void *x, double *out2) {
    if (!x || !out2 || count < 1 || clock_bad_dtype(dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_minmax: bad argument");
    return engine_call("ssf_minmax", device, [&](std::string *err) { return ssf::clock_minmax(device, count, dtype, x, out2, err); });
}

int ssf_clock_scale_add(int device, int64_t count, double scale, int32_t has_scale, const double *x, const double *noise, double *out) {
    if (!x || !out || count < 1) return set_err(SSF_ERR_BAD_ARG, "ssf_clock_scale_add: bad argument");
    return engine_call("ssf_clock_scale_add", device, [&](std::string *err) { return ssf::clock_scale_add(device, count, scale, has_scale, x, noise, out, err); });
}

int ssf_gardner(int device, const ssf_gardner_params *p, const void *x, void *sig_out, double *t_out, int64_t *last_n) {
    if (!p || !x || !sig_out || !t_out || !last_n) return set_err(SSF_ERR_BAD_ARG, "ssf_gardner: NULL argument");
    const char *msg = nullptr;
    if (p->dtype != SSF_M_C128 && p->dtype != SSF_M_C64) msg = "dtype must be complex128 or complex64";
    else if (p->n < 1 || p->lpad < 0 || p->Ln < 1 || p->n > (1LL << 40) || p->lpad > (1LL << 40) || p->Ln > (1LL << 41))
        msg = "n >= 1, lpad >= 0 and Ln >= 1 are needed";
    else if (p->nModes < 1 || p->nModes > 65535) msg = "nModes must be 1 .. 65535";
    else if (!std::isfinite(p->kp) || !std::isfinite(p->ki)) msg = "kp and ki must be finite";
    if (msg) return set_err(SSF_ERR_BAD_ARG, std::string("ssf_gardner: ") + msg);
    return engine_call("ssf_gardner", device, [&](std::string *err) { return ssf::clock_gardner(device, p, x, sig_out, t_out, last_n, err); });
}

int ssf_clock_drift(int device, int64_t n, int32_t ncols, int32_t per_column, const double *t, double *ppm_out) {
    if (!t || !ppm_out || n < 1 || ncols < 1 || ncols > 65535 || n > (1LL << 40)) return set_err(SSF_ERR_BAD_ARG, "ssf_clock_drift: bad argument");
    return engine_call("ssf_clock_drift", device, [&](std::string *err) { return ssf::clock_drift(device, n, ncols, per_column, t, ppm_out, err); });
}

// ---- the array layer of DeviceArray (engine_array.hip): every check comes before the first allocation or launch
static bool array_bad_dtype(int32_t d) { return d < SSF_M_C128 || d > SSF_M_F32; }
static bool array_bad_itemsize(int32_t s) { return s != 1 && s != 2 && s != 4 && s != 8 && s != 16; }
static const int64_t kArrayMax = (int64_t)1 << 40;            // elements of one array
// every element the descriptor reaches lies in [0, extent)
static bool array_bad_desc(const ssf_array_desc *d) {
    if (d->ndim < 0 || d->ndim > SSF_ARRAY_MAX_DIM || array_bad_itemsize(d->itemsize) || d->extent < 0 || d->extent > kArrayMax) return true;
    int64_t lo = d->offset, hi = d->offset, count = 1;
    for (int a = 0; a < d->ndim; ++a) {
        if (d->shape[a] < 0 || d->shape[a] > kArrayMax || d->stride[a] > kArrayMax || d->stride[a] < -kArrayMax) return true;
        count *= d->shape[a];
        if (count > kArrayMax) return true;
    }
    if (count == 0) return false;
    if (d->offset < 0 || d->offset >= d->extent) return true;
    for (int a = 0; a < d->ndim; ++a) {
        if (d->shape[a] == 1) continue;
        // an axis of more than one element steps by less than the allocation: its span (shape - 1) |stride| then fits 2^80 only
        // in 128 bits, where it is formed; lo and hi stay within 4 x 2^80
        const int64_t step = d->stride[a] < 0 ? -d->stride[a] : d->stride[a];
        if (step >= d->extent) return true;
        const __int128 span = (__int128)(d->shape[a] - 1) * step;
        if (span >= d->extent) return true;
        if (d->stride[a] < 0) lo -= (int64_t)span;
        else hi += (int64_t)span;
    }
    return lo < 0 || hi >= d->extent;
}
// a destination must not write an element twice: with the axes of more than one element ordered by |stride|, each steps over
// everything the ones before it reach
static bool array_desc_overlaps(const ssf_array_desc *d) {
    int64_t step[SSF_ARRAY_MAX_DIM], n[SSF_ARRAY_MAX_DIM];
    int k = 0;
    for (int a = 0; a < d->ndim; ++a) {
        if (d->shape[a] == 0) return false;
        if (d->shape[a] == 1) continue;
        step[k] = d->stride[a] < 0 ? -d->stride[a] : d->stride[a], n[k] = d->shape[a], ++k;
    }
    for (int i = 1; i < k; ++i)
        for (int j = i; j > 0 && step[j] < step[j - 1]; --j) std::swap(step[j], step[j - 1]), std::swap(n[j], n[j - 1]);
    int64_t reach = 0;                       // the furthest element the axes so far reach (array_bad_desc: below extent)
    for (int i = 0; i < k; ++i) {
        if (step[i] <= reach) return true;
        reach += (n[i] - 1) * step[i];
    }
    return false;
}

int ssf_array_copy(int device, const ssf_array_desc *src_desc, const void *src, const ssf_array_desc *dst_desc, void *dst) {
    if (!src_desc || !dst_desc || !src || !dst) return set_err(SSF_ERR_BAD_ARG, "ssf_array_copy: NULL argument");
    if (array_bad_desc(src_desc) || array_bad_desc(dst_desc)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_copy: a descriptor is malformed or leaves its array");
    if (array_desc_overlaps(dst_desc)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_copy: the destination descriptor reaches an element twice");
    if (src_desc->ndim != dst_desc->ndim || src_desc->itemsize != dst_desc->itemsize) return set_err(SSF_ERR_BAD_ARG, "ssf_array_copy: the two sides differ in ndim or itemsize");
    int64_t count = 1;
    for (int a = 0; a < src_desc->ndim; ++a) {
        if (src_desc->shape[a] != dst_desc->shape[a]) return set_err(SSF_ERR_BAD_ARG, "ssf_array_copy: the two sides differ in shape");
        count *= src_desc->shape[a];
    }
    if (src == dst) return set_err(SSF_ERR_BAD_ARG, "ssf_array_copy: in place is not supported");
    if (count == 0) return SSF_OK;
    return engine_call("ssf_array_copy", device, [&](std::string *err) { return ssf::array_copy(device, src_desc, src, dst_desc, dst, err); });
}

int ssf_array_take(int device, int64_t n_src, int64_t n_idx, int64_t inner, int32_t itemsize, int32_t idx_itemsize, const void *idx,
                   const void *src, void *dst) {
    if (!idx || !src || !dst || src == dst) return set_err(SSF_ERR_BAD_ARG, "ssf_array_take: NULL argument or in place");
    if (n_src < 1 || n_idx < 0 || inner < 0 || n_src > kArrayMax || n_idx > kArrayMax || inner > kArrayMax || (inner && (n_idx > kArrayMax / inner || n_src > kArrayMax / inner)))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_take: bad sizes");
    if (array_bad_itemsize(itemsize) || (idx_itemsize != 4 && idx_itemsize != 8)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_take: bad itemsize");
    if (n_idx == 0 || inner == 0) return SSF_OK;
    return engine_call("ssf_array_take", device, [&](std::string *err) {
        return ssf::array_take(device, n_src, n_idx, inner, itemsize, idx_itemsize, idx, src, dst, err);
    });
}

int ssf_array_transpose(int device, int64_t rows, int64_t cols, int32_t itemsize, const void *src, void *dst) {
    if (!src || !dst || src == dst) return set_err(SSF_ERR_BAD_ARG, "ssf_array_transpose: NULL argument or in place");
    if (rows < 0 || cols < 0 || rows > kArrayMax || cols > kArrayMax || (cols && rows > kArrayMax / cols) || array_bad_itemsize(itemsize))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_transpose: bad sizes");
    if (((rows + 31) / 32) * ((cols + 31) / 32) > 0x7fffffffLL) return set_err(SSF_ERR_UNSUPPORTED, "ssf_array_transpose: too many tiles");
    if (rows == 0 || cols == 0) return SSF_OK;
    return engine_call("ssf_array_transpose", device, [&](std::string *err) { return ssf::array_transpose(device, rows, cols, itemsize, src, dst, err); });
}

int ssf_array_fill(int device, int64_t count, int32_t itemsize, const void *value, void *dst) {
    if (!value || !dst || count < 0 || count > kArrayMax || array_bad_itemsize(itemsize)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_fill: bad argument");
    if (count == 0) return SSF_OK;
    if (int rc = check_device(device)) return rc;
    if (ssf::on_device(value)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_fill: the value is host memory");
    return engine_result("ssf_array_fill", [&](std::string *err) { return ssf::array_fill(device, count, itemsize, value, dst, err); });
}

int ssf_array_binary(int device, const ssf_array_binary_params *p, const void *a, const void *b, void *out) {
    if (!p || !a || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: NULL argument");
    if (p->op < SSF_ARRAY_ADD || p->op > SSF_ARRAY_DIV || p->kind < SSF_ARRAY_SAME || p->kind > SSF_ARRAY_COLUMN || (p->swap != 0 && p->swap != 1))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: unknown op, kind or swap");
    if (array_bad_dtype(p->a_dtype) || array_bad_dtype(p->b_dtype) || array_bad_dtype(p->out_dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: bad dtype");
    if ((p->a_dtype <= SSF_M_C64 || p->b_dtype <= SSF_M_C64) != (p->out_dtype <= SSF_M_C64))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: the result is complex exactly if an operand is");
    if (p->count < 0 || p->count > kArrayMax) return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: bad count");
    if (p->kind != SSF_ARRAY_SCALAR && !b) return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: the second operand is NULL");
    if ((p->kind == SSF_ARRAY_ROW || p->kind == SSF_ARRAY_COLUMN) && (p->inner < 1 || p->count % p->inner))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: inner must divide count");
    if (a == out || b == out) return set_err(SSF_ERR_BAD_ARG, "ssf_array_binary: in place is not supported");
    if (p->count == 0) return SSF_OK;
    return engine_call("ssf_array_binary", device, [&](std::string *err) { return ssf::array_binary(device, p, a, b, out, err); });
}

int ssf_array_unary(int device, int32_t op, int32_t in_dtype, int32_t out_dtype, int64_t count, const void *x, void *out) {
    if (!x || !out || x == out) return set_err(SSF_ERR_BAD_ARG, "ssf_array_unary: NULL argument or in place");
    if (op < SSF_ARRAY_NEG || op > SSF_ARRAY_CONVERT || array_bad_dtype(in_dtype) || array_bad_dtype(out_dtype) || count < 0 || count > kArrayMax)
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_unary: bad op, dtype or count");
    const bool in_c = in_dtype <= SSF_M_C64, out_c = out_dtype <= SSF_M_C64;
    const bool real_result = op >= SSF_ARRAY_REAL && op <= SSF_ARRAY_ANGLE;
    if (op == SSF_ARRAY_SQRT && in_c) return set_err(SSF_ERR_UNSUPPORTED, "ssf_array_unary: sqrt of real arrays only");
    if (real_result ? out_c : (op == SSF_ARRAY_CONVERT ? (in_c && !out_c) : in_c != out_c))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_unary: the result dtype does not fit the operation");
    if (count == 0) return SSF_OK;
    return engine_call("ssf_array_unary", device, [&](std::string *err) { return ssf::array_unary(device, op, in_dtype, out_dtype, count, x, out, err); });
}

int ssf_array_reduce(int device, int32_t op, int32_t dtype, int64_t rows, int32_t cols, const double *center, const void *x, double *out,
                     int64_t *arg_out) {
    if (!x || !out) return set_err(SSF_ERR_BAD_ARG, "ssf_array_reduce: NULL argument");
    if (op < SSF_ARRAY_SUM || op > SSF_ARRAY_MAX || array_bad_dtype(dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_array_reduce: bad op or dtype");
    if (rows < 1 || cols < 1 || cols > 65535 || rows > kArrayMax / cols) return set_err(SSF_ERR_BAD_ARG, "ssf_array_reduce: bad sizes");
    if (op == SSF_ARRAY_SUMSQDEV && !center) return set_err(SSF_ERR_BAD_ARG, "ssf_array_reduce: the squared deviations need a centre");
    if ((op == SSF_ARRAY_MIN || op == SSF_ARRAY_MAX) && (!arg_out || dtype <= SSF_M_C64))
        return set_err(SSF_ERR_BAD_ARG, "ssf_array_reduce: min and max are for real arrays and need arg_out");
    return engine_call("ssf_array_reduce", device, [&](std::string *err) {
        return ssf::array_reduce(device, op, dtype, rows, cols, op == SSF_ARRAY_SUMSQDEV ? center : nullptr, x, out, arg_out, err);
    });
}

int ssf_freq_shift(int device, int64_t n, int32_t ncols, int32_t dtype, double deltaF, double Fs, const void *x, void *out) {
    if (!x || !out || x == out) return set_err(SSF_ERR_BAD_ARG, "ssf_freq_shift: NULL argument or in place");
    if (n < 0 || ncols < 1 || n > kArrayMax / ncols || array_bad_dtype(dtype)) return set_err(SSF_ERR_BAD_ARG, "ssf_freq_shift: bad sizes or dtype");
    if (!std::isfinite(deltaF) || !std::isfinite(Fs) || Fs == 0) return set_err(SSF_ERR_BAD_ARG, "ssf_freq_shift: deltaF must be finite, Fs finite and non-zero");
    if (n == 0) return SSF_OK;
    return engine_call("ssf_freq_shift", device, [&](std::string *err) { return ssf::array_freq_shift(device, n, ncols, dtype, deltaF, Fs, x, out, err); });
}

}  // extern "C"
