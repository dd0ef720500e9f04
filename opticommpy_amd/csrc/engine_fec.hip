// engine_fec.hip -- soft-decision FEC on the device (ssf_calc_llr, ssf_ldpc_graph_create / destroy, ssf_ldpc_decode of
// include/ssf.h).  The node bodies and their semantics are fec_kernels.h; here are the two walks over them.
//   LDS     one workgroup per codeword runs the whole decode in one launch: messages (padded, fec::Padded), LLRs, posteriors and
//           decisions in LDS, the graph read from device memory (every workgroup reads the same arrays: they stay in L2), one
//           thread per check, then per variable, a barrier between the phases, parity through one flag in LDS, the loop left at
//           convergence.
//   global  messages, LLRs, posteriors and decisions in device memory, codeword-minor (msg[e][cw]); thread t of a launch is node
//           t / ncw of codeword t % ncw, with no padding: the lanes of a wave cover all codewords of a few neighbouring nodes, so
//           every access to an edge -- the variable update's gather included -- is one run of ncw consecutive values, and one
//           codeword alone is simply edge-major.  Two launches per iteration: k_check (the parity test of the iteration before,
//           then the check update) and k_var (variable update, posterior, decision).
//           k_check of iteration it + 1 writes unsat[it][cw] = 1 if a check of codeword cw fails; k_var of iteration it + 1 finds
//           it still 0 for a converged codeword, leaves that codeword's posterior as it is and sets done[cw], after which every
//           later launch skips the codeword.  The check update that ran in between only touched messages nobody reads again.
//           No host synchronisation per iteration unless sync_every asks for the flags.
// Both walks give every node to exactly one thread, which runs the body's loops in edge order: no floating-point atomics, no
// order left to the scheduler, so results repeat bit for bit and are the same from both engines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "engine_host.h"
#include "fec_kernels.h"

namespace ssf {
namespace {
using namespace fec;
using namespace eng;

constexpr int kBlock = 256;
constexpr int kLlrMaxM = 1024;

// ---- calcLLR: one symbol per thread, the tables in LDS
struct LlrArgs {
    const void *x;
    int dtype, M, b;
    long long n;
    double sigma2;
    const double *tab, *px;
    const unsigned *zmask, *omask;
    double *out;
};

__global__ __launch_bounds__(kBlock) void k_calc_llr(LlrArgs a) {
    __shared__ double s_tab[2 * kLlrMaxM], s_px[kLlrMaxM];
    __shared__ unsigned s_z[kLlrMaxM], s_o[kLlrMaxM];
    for (int i = threadIdx.x; i < a.M; i += kBlock) {
        s_tab[2 * i] = a.tab[2 * i], s_tab[2 * i + 1] = a.tab[2 * i + 1];
        s_px[i] = a.px[i], s_z[i] = a.zmask[i], s_o[i] = a.omask[i];
    }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += (long long)gridDim.x * kBlock) {
        double re, im, llr[kMaxBits];
        mk::load(a.dtype, a.x, i, re, im);
        llr_body(re, im, a.sigma2, a.M, a.b, s_tab, s_px, s_z, s_o, llr);
#pragma unroll
        for (int j = 0; j < kMaxBits; ++j)
            if (j < a.b) a.out[i * a.b + j] = llr[j];
    }
}

// ---- LDPC
struct DecArgs {
    const int *co, *ev, *vo, *ve;             // check_offsets, edge_var, var_offsets, var_edge_indices
    int m, n, E;
    const void *in;
    int in_dtype, n_, ncw, transposed, maxIter;
    void *out;                                // posterior LLRs of the message type, in the caller's orientation
    int8_t *bits, *fail;
    uint32_t *iter;
    // global engine only
    void *msg, *llr, *post;                   // (E, ncw), (n, ncw), (n, ncw) of the message type
    unsigned char *hard;                      // (n, ncw)
    int *unsat, *done;                        // (maxIter, ncw), (ncw)
};

template <class T, int MODE>
__global__ __launch_bounds__(kBlock) void k_ldpc_lds(DecArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    T *msg = (T *)smem;
    T *llr = msg + Padded::slots(a.E);
    T *post = llr + a.n;
    int *flag = (int *)(post + a.n);          // a failed check raises it; thread 0 lowers it a phase earlier
    unsigned char *hard = (unsigned char *)(post + a.n) + kLdsFlag;
    const int cw = blockIdx.x, tid = threadIdx.x;
    const Padded idx;
    for (int v = tid; v < a.n; v += kBlock) llr[v] = load_llr<T>(a.in, a.in_dtype, v, cw, a.n_, a.ncw, a.transposed);
    __syncthreads();
    for (int e = tid; e < a.E; e += kBlock) msg[idx(e)] = llr[a.ev[e]];
    __syncthreads();
    int it = 0, failed = 1;
    for (; it < a.maxIter; ++it) {
        for (int c = tid; c < a.m; c += kBlock) check_update<T, MODE>(msg, a.co[c], a.co[c + 1], idx);
        __syncthreads();                      // (every thread has read the flag of the iteration before by now)
        if (tid == 0) *flag = 0;
        for (int v = tid; v < a.n; v += kBlock) var_update<T>(msg, a.ve, a.vo[v], a.vo[v + 1], llr[v], post[v], hard[v], idx);
        __syncthreads();
        int odd = 0;
        for (int c = tid; c < a.m; c += kBlock) odd |= check_parity(hard, a.ev, a.co[c], a.co[c + 1], Plain());
        if (odd) *flag = 1;
        __syncthreads();
        failed = *flag;
        if (!failed) break;
    }
    for (int v = tid; v < a.n_; v += kBlock) {
        const long long o = user_index(v, cw, a.n_, a.ncw, a.transposed);
        ((T *)a.out)[o] = post[v];
        a.bits[o] = (int8_t)hard[v];
    }
    if (tid == 0) {
        a.fail[cw] = failed ? 1 : 0;
        if (a.iter) a.iter[cw] = (uint32_t)(failed ? a.maxIter - 1 : it);
    }
}

// ---- global engine: thread t of a launch is node t / ncw of codeword t % ncw, and every array is codeword-minor (x[i][cw])
struct Who {
    long long i;                              // node (or edge) index
    int cw;
    bool valid;
};
__device__ __forceinline__ Who who(const DecArgs &a, long long count) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    Who w;
    w.i = t / a.ncw, w.cw = (int)(t - w.i * a.ncw), w.valid = w.i < count;
    return w;
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_init(DecArgs a) {
    const Who w = who(a, a.n > a.E ? a.n : a.E);
    if (!w.valid) return;
    const long long o = w.i * a.ncw + w.cw;
    if (w.i < a.n) ((T *)a.llr)[o] = load_llr<T>(a.in, a.in_dtype, (int)w.i, w.cw, a.n_, a.ncw, a.transposed);
    if (w.i < a.E) ((T *)a.msg)[o] = load_llr<T>(a.in, a.in_dtype, a.ev[w.i], w.cw, a.n_, a.ncw, a.transposed);
}

// parity of iteration it - 1 (it > 0), then the check update of iteration it (unless parity_only)
template <class T, int MODE>
__global__ __launch_bounds__(kBlock) void k_check(DecArgs a, int it, int parity_only) {
    __shared__ int s_odd[kBlock];
    const Who w = who(a, a.m);
    const bool active = w.valid && !a.done[w.cw];     // (done is written by k_var only)
    const int c = (int)w.i;
    const Strided idx{a.ncw, w.cw};
    if (it > 0) {
        // a workgroup's threads are consecutive in (node, codeword): its first min(ncw, 256) threads meet every codeword it
        // holds.  Slot of a codeword: cw itself for fewer than 256 codewords, else the thread (then no two threads share one).
        // One plain store of one value per workgroup and codeword, and none once the flag is up.
        const int slot = a.ncw < kBlock ? w.cw : (int)threadIdx.x;
        s_odd[threadIdx.x] = 0;
        __syncthreads();
        if (active && check_parity(a.hard, a.ev, a.co[c], a.co[c + 1], idx)) s_odd[slot] = 1;
        __syncthreads();
        if (active && (int)threadIdx.x < a.ncw && s_odd[slot]) {
            int *u = a.unsat + (size_t)(it - 1) * a.ncw + w.cw;
            if (!*u) *u = 1;
        }
    }
    if (parity_only || !active) return;
    check_update<T, MODE>((T *)a.msg, a.co[c], a.co[c + 1], idx);
}

template <class T>
__global__ __launch_bounds__(kBlock) void k_var(DecArgs a, int it, int *d_fail, uint32_t *d_iter) {
    const Who w = who(a, a.n);
    if (!w.valid || a.done[w.cw]) return;
    if (it > 0 && a.unsat[(size_t)(it - 1) * a.ncw + w.cw] == 0) {        // converged at it - 1: the posterior stays
        if (w.i == 0) a.done[w.cw] = 1, d_fail[w.cw] = 0, d_iter[w.cw] = (uint32_t)(it - 1);
        return;
    }
    const int v = (int)w.i;
    const long long o = w.i * a.ncw + w.cw;
    var_update<T>((T *)a.msg, a.ve, a.vo[v], a.vo[v + 1], ((const T *)a.llr)[o], ((T *)a.post)[o], a.hard[o], Strided{a.ncw, w.cw});
}

// after the parity test of the last iteration run (index last): the codewords not yet done, and the outputs in the caller's layout
template <class T>
__global__ __launch_bounds__(kBlock) void k_finish(DecArgs a, int last, int *d_fail, uint32_t *d_iter) {
    const Who w = who(a, a.n);
    if (!w.valid) return;
    if (w.i == 0) {
        if (!a.done[w.cw]) d_fail[w.cw] = a.unsat[(size_t)last * a.ncw + w.cw] ? 1 : 0, d_iter[w.cw] = (uint32_t)last;
        a.fail[w.cw] = (int8_t)d_fail[w.cw];
        if (a.iter) a.iter[w.cw] = d_iter[w.cw];
    }
    if (w.i >= a.n_) return;
    const long long o = user_index((int)w.i, w.cw, a.n_, a.ncw, a.transposed);
    ((T *)a.out)[o] = ((const T *)a.post)[w.i * a.ncw + w.cw];
    a.bits[o] = (int8_t)a.hard[w.i * a.ncw + w.cw];
}

// ---- host side
struct Work : WorkBase {
    Buf in, tables, out, bits, fail, iter, msg, llr, post, hard, flags, state;
    std::vector<unsigned char> host_tab;      // kept for their capacity
    std::vector<int> host_done;
};
using Call = CallT<Work>;

template <class T, int MODE>
bool launch_lds(Call &c, const DecArgs &a, size_t lds) {
    if (!c.ok(hipFuncSetAttribute((const void *)k_ldpc_lds<T, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
              "hipFuncSetAttribute"))
        return false;
    k_ldpc_lds<T, MODE><<<a.ncw, kBlock, lds, c.w->st>>>(a);
    return c.launched();
}

template <class T, int MODE>
bool run_global(Call &c, const DecArgs &a, int sync_every, int *d_fail, uint32_t *d_iter) {
    Work &w = *c.w;
    const auto blocks = [&](long long nodes) { return (unsigned)((nodes * a.ncw + kBlock - 1) / kBlock); };
    const unsigned gi = blocks(std::max(a.n, a.E)), gc = blocks(a.m), gv = blocks(a.n);
    k_init<T><<<gi, kBlock, 0, w.st>>>(a);
    if (!c.launched()) return false;
    int it = 0;
    for (; it < a.maxIter; ++it) {
        k_check<T, MODE><<<gc, kBlock, 0, w.st>>>(a, it, 0);
        k_var<T><<<gv, kBlock, 0, w.st>>>(a, it, d_fail, d_iter);
        if (!c.launched()) return false;
        if (sync_every > 0 && it > 0 && it % sync_every == 0 && it + 1 < a.maxIter) {
            w.host_done.resize((size_t)a.ncw);
            if (!c.deliver(w.host_done.data(), a.done, (size_t)a.ncw * sizeof(int)) || !c.sync()) return false;
            bool all = true;
            for (int d : w.host_done) all = all && d;
            if (all) {
                ++it;
                break;
            }
        }
    }
    k_check<T, MODE><<<gc, kBlock, 0, w.st>>>(a, it, 1);
    k_finish<T><<<gv, kBlock, 0, w.st>>>(a, it - 1, d_fail, d_iter);
    return c.launched();
}

}  // namespace

int fec_calc_llr(int device, int64_t n, int dtype, int M, double sigma2, const double *table, const int32_t *bitmap, const double *px,
                 const void *x, double *llr_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    int b = 0;
    while ((1 << b) < M) ++b;
    const size_t out_bytes = (size_t)n * b * sizeof(double);
    double *out = (double *)c.target(llr_out, w.out, out_bytes);
    if (!out) return c.rc;
    const void *xd = c.input(x, w.in, (size_t)n * mk::elem_size(dtype));
    if (!xd) return c.rc;
    // [table 2 M doubles | px M doubles | zero masks M | one masks M]
    const size_t tab_bytes = (size_t)M * (3 * sizeof(double) + 2 * sizeof(unsigned));
    w.host_tab.resize(tab_bytes);
    double *ht = (double *)w.host_tab.data();
    unsigned *hz = (unsigned *)(ht + 3 * (size_t)M), *ho = hz + M;
    for (int i = 0; i < 2 * M; ++i) ht[i] = table[i];
    for (int i = 0; i < M; ++i) {
        ht[2 * (size_t)M + i] = px[i];
        unsigned z = 0, o = 0;
        for (int j = 0; j < b; ++j) {
            z |= bitmap[(size_t)i * b + j] == 0 ? 1u << j : 0u;
            o |= bitmap[(size_t)i * b + j] == 1 ? 1u << j : 0u;
        }
        hz[i] = z, ho[i] = o;
    }
    if (!c.upload(w.tables, w.host_tab)) return c.rc;
    LlrArgs a{};
    a.x = xd, a.dtype = dtype, a.M = M, a.b = b, a.n = n, a.sigma2 = sigma2, a.out = out;
    a.tab = (const double *)w.tables.p, a.px = a.tab + 2 * (size_t)M;
    a.zmask = (const unsigned *)(a.px + M), a.omask = a.zmask + M;
    if (n > 0) {
        const long long nb = (n + kBlock - 1) / kBlock;
        k_calc_llr<<<(unsigned)(nb < 8192 ? nb : 8192), kBlock, 0, w.st>>>(a);
        if (!c.launched()) return c.rc;
    }
    if (!c.deliver(llr_out, out, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

int fec_graph_create(int device, int m, int n, int E, const int32_t *co, const int32_t *ev, const int32_t *vo, const int32_t *ve,
                     int max_dc, ssf_ldpc_graph **out, std::string *err) {
    Call c(device, err, false);
    if (c.rc) return c.rc;
    ssf_ldpc_graph *g = new ssf_ldpc_graph();
    g->device = device, g->m = m, g->n = n, g->E = E, g->max_dc = max_dc;
    const size_t total = (size_t)(m + 1) + (size_t)(n + 1) + 2 * (size_t)E;
    if (!c.ok(hipMalloc((void **)&g->d_all, total * sizeof(int)), "hipMalloc")) {
        delete g;
        return c.rc;
    }
    g->d_co = g->d_all, g->d_ev = g->d_co + (m + 1), g->d_vo = g->d_ev + E, g->d_ve = g->d_vo + (n + 1);
    bool ok = c.ok(hipMemcpy(g->d_co, co, (size_t)(m + 1) * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") &&
              c.ok(hipMemcpy(g->d_ev, ev, (size_t)E * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") &&
              c.ok(hipMemcpy(g->d_vo, vo, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy") &&
              c.ok(hipMemcpy(g->d_ve, ve, (size_t)E * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
    if (!ok) {
        (void)hipFree(g->d_all);
        delete g;
        return c.rc;
    }
    *out = g;
    return SSF_OK;
}

int fec_graph_destroy(ssf_ldpc_graph *g, std::string *err) {
    Call c(g->device, err, false);
    if (!c.rc) c.ok(hipFree(g->d_all), "hipFree");
    delete g;
    return c.rc;
}

int fec_decode(int device, const ssf_ldpc_graph *g, const ssf_ldpc_params *p, const void *llr_in, void *llr_out, int8_t *bits_out,
               int8_t *fail_out, uint32_t *iter_out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const int ncw = p->numCodewords, n_ = p->n_;
    const size_t wsz = p->prec == kF64 ? 8 : 4, isz = p->in_dtype == kF64 ? 8 : 4;
    const size_t count = (size_t)n_ * ncw;
    const long long lds = lds_bytes(g->E, g->n, p->prec);
    const bool use_lds = p->engine == kEngineLds || (p->engine == kEngineAuto && lds <= kLdsBudget);
    if (use_lds && lds > kLdsBudget) {
        *err = "the graph needs " + std::to_string(lds) + " bytes of LDS, more than a workgroup has: use the global engine";
        return SSF_ERR_UNSUPPORTED;
    }
    DecArgs a{};
    a.co = g->d_co, a.ev = g->d_ev, a.vo = g->d_vo, a.ve = g->d_ve, a.m = g->m, a.n = g->n, a.E = g->E;
    a.in_dtype = p->in_dtype, a.n_ = n_, a.ncw = ncw, a.transposed = p->transposed, a.maxIter = p->maxIter;
    a.out = c.target(llr_out, w.out, count * wsz);
    a.bits = (int8_t *)c.target(bits_out, w.bits, count);
    a.fail = (int8_t *)c.target(fail_out, w.fail, (size_t)ncw);
    a.iter = iter_out ? (uint32_t *)c.target(iter_out, w.iter, (size_t)ncw * sizeof(uint32_t)) : nullptr;
    if (!a.out || !a.bits || !a.fail || (iter_out && !a.iter)) return c.rc;
    a.in = c.input(llr_in, w.in, count * isz);
    if (!a.in) return c.rc;

    const int mode = p->alg == kMSA ? -1 : spa_mode(g->max_dc);
    const bool f64 = p->prec == kF64;
    bool ok = false;
    if (use_lds) {
#define SSF_FEC_LDS_CASE(M_) (f64 ? launch_lds<double, M_>(c, a, (size_t)lds) : launch_lds<float, M_>(c, a, (size_t)lds))
        ok = mode < 0 ? SSF_FEC_LDS_CASE(-1) : mode == 8 ? SSF_FEC_LDS_CASE(8) : mode == 32 ? SSF_FEC_LDS_CASE(32) : SSF_FEC_LDS_CASE(0);
#undef SSF_FEC_LDS_CASE
    } else {
        const size_t flag_ints = (size_t)p->maxIter * ncw + ncw;      // unsat, done
        if (!c.need(w.msg, (size_t)ncw * g->E * wsz) || !c.need(w.llr, (size_t)ncw * g->n * wsz) || !c.need(w.post, (size_t)ncw * g->n * wsz) ||
            !c.need(w.hard, (size_t)ncw * g->n) || !c.need(w.flags, flag_ints * sizeof(int)) || !c.need(w.state, (size_t)ncw * 2 * sizeof(int)))
            return c.rc;
        a.msg = w.msg.p, a.llr = w.llr.p, a.post = w.post.p, a.hard = (unsigned char *)w.hard.p;
        a.unsat = (int *)w.flags.p, a.done = a.unsat + (size_t)p->maxIter * ncw;
        int *d_fail = (int *)w.state.p;
        uint32_t *d_iter = (uint32_t *)(d_fail + ncw);
        if (!c.ok(hipMemsetAsync(w.flags.p, 0, flag_ints * sizeof(int), w.st), "hipMemset")) return c.rc;
#define SSF_FEC_GLB_CASE(M_) \
    (f64 ? run_global<double, M_>(c, a, p->sync_every, d_fail, d_iter) : run_global<float, M_>(c, a, p->sync_every, d_fail, d_iter))
        ok = mode < 0 ? SSF_FEC_GLB_CASE(-1) : mode == 8 ? SSF_FEC_GLB_CASE(8) : mode == 32 ? SSF_FEC_GLB_CASE(32) : SSF_FEC_GLB_CASE(0);
#undef SSF_FEC_GLB_CASE
    }
    if (!ok) return c.rc;
    if (!c.deliver(llr_out, a.out, count * wsz) || !c.deliver(bits_out, a.bits, count) || !c.deliver(fail_out, a.fail, (size_t)ncw)) return c.rc;
    if (iter_out && !c.deliver(iter_out, a.iter, (size_t)ncw * sizeof(uint32_t))) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
