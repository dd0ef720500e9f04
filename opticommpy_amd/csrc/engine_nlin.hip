// engine_nlin.hip -- the first-order perturbation model on the device (ssf_pert_nlin of include/ssf.h).  The per-lane bodies are
// nlin_kernels.h; here are the kernels that walk them and the launch sequence:
//   k_power -> k_power_fin      sum |x|^2, sum |y|^2: a grid-stride running value per lane, block_reduce.h's tree per workgroup, one
//                               wave over the partials -- the order of the device pnorm, so a mean repeats bit for bit
//   k_stage                     the normalised symbols, 2 x N complex128 (rounded to single precision where the reference's are)
//   (perturbationNLIN: the three once for pnorm, once for the normalisation inside the calculation)
//   k_main<DENSE>               tiles x shares workgroups of 64 lanes: each share's dx, dy
//   k_finish                    the shares in order, the phases, the rounding to prec, and for perturbationNLIN the field
// The tables of a coefficient plan stay on the device under the plan's key (the last kPlans of them per device): a call that names
// a key that is there uploads nothing.
#include <hip/hip_runtime.h>

#include <cstring>
#include <list>
#include <vector>

#include "block_reduce.h"
#include "dev_ctx.h"
#include "engine_host.h"
#include "nlin_kernels.h"

namespace ssf {
namespace {
using namespace nlin;
using namespace eng;

struct NlinCtx : DevCtxCore {};
#define SSF_NLIN_CTX()                                                        \
    extern __shared__ __attribute__((aligned(16))) char ssf_smem[];           \
    NlinCtx ctx{{(int)threadIdx.x, (int)blockIdx.x, (int)blockDim.x, (int)gridDim.x, ssf_smem}}

struct PowerArgs {
    const void *in[2];
    long long stride, N;
    int in_c64, nb;
    double *part;                 // 2 x nb
    double *total;                // 2
};
// blockIdx.y: the column
__global__ void __launch_bounds__(kBlock) k_power(const PowerArgs a) {
    const int col = blockIdx.y;
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < a.N; t += (long long)gridDim.x * kBlock)
        acc += power_term(a.in[col], t * a.stride, a.in_c64);
    br::block_sum_store(acc, a.part + (long long)col * a.nb + blockIdx.x);
}
__global__ void __launch_bounds__(64) k_power_fin(const PowerArgs a) {
    for (int col = 0; col < 2; ++col) {
        const double s = br::wave_sum_partials(a.part + (long long)col * a.nb, a.nb, 1);
        if (threadIdx.x == 0) a.total[col] = s;
    }
}
__global__ void __launch_bounds__(kBlock) k_stage(const StageArgs a) {
    SSF_NLIN_CTX();
    stage_body(ctx, a, (int)blockIdx.y);
}
template <bool DENSE> __global__ void __launch_bounds__(kLanes) k_main(const MainArgs a) {
    SSF_NLIN_CTX();
    main_body<DENSE>(ctx, a, (long long)blockIdx.x, (int)blockIdx.y);
}
__global__ void __launch_bounds__(kBlock) k_finish(const FinishArgs a) {
    SSF_NLIN_CTX();
    finish_body(ctx, a);
}

constexpr size_t kPlans = 8;
struct PlanTables {
    uint64_t key = 0;
    Buf tab;                      // [pass | nidx | phase_m | pad to 16 | coef | phase_c]
    size_t sig[5] = {0, 0, 0, 0, 0};          // L, npass, ncoef, nphase, dense: what the entries were checked against
    std::vector<char> host;       // kept for its capacity
};
struct Work : WorkBase {
    Buf in0, in1, out[4], e1, xs, part, red, total;
    std::list<PlanTables> plans;  // most recently used first
};
using Call = CallT<Work>;

struct TableOffsets {
    size_t pass, nidx, phase_m, coef, phase_c, bytes;
};
TableOffsets offsets(const ssf_nlin_params *p) {
    TableOffsets o;
    o.pass = 0;
    o.nidx = o.pass + (size_t)p->npass * 4 * sizeof(int32_t);
    o.phase_m = o.nidx + (size_t)p->ncoef * sizeof(int32_t);
    o.coef = (o.phase_m + (size_t)p->nphase * sizeof(int32_t) + 15) / 16 * 16;
    o.phase_c = o.coef + (size_t)p->ncoef * 16;
    o.bytes = o.phase_c + (size_t)p->nphase * 16 + 16;
    return o;
}

// the device tables of the call's plan: found by key, or uploaded (in place of the one used longest ago)
const char *tables(Call &c, const ssf_nlin_params *p, const int32_t *pass, const double *coef, const int32_t *nidx, const int32_t *phase_m,
                   const double *phase_c) {
    Work &w = *c.w;
    const size_t sig[5] = {(size_t)p->L, (size_t)p->npass, (size_t)p->ncoef, (size_t)p->nphase, (size_t)p->dense};
    if (p->plan_key)
        for (auto it = w.plans.begin(); it != w.plans.end(); ++it)
            if (it->key == p->plan_key && !std::memcmp(it->sig, sig, sizeof(sig))) {
                w.plans.splice(w.plans.begin(), w.plans, it);
                return (const char *)it->tab.p;
            }
    if (w.plans.size() >= kPlans) w.plans.splice(w.plans.begin(), w.plans, std::prev(w.plans.end()));
    else w.plans.emplace_front();
    PlanTables &t = w.plans.front();
    t.key = 0;
    const TableOffsets o = offsets(p);
    t.host.assign(o.bytes, 0);
    if (p->npass) std::memcpy(t.host.data() + o.pass, pass, (size_t)p->npass * 4 * sizeof(int32_t));
    if (p->ncoef && nidx) std::memcpy(t.host.data() + o.nidx, nidx, (size_t)p->ncoef * sizeof(int32_t));
    if (p->nphase) std::memcpy(t.host.data() + o.phase_m, phase_m, (size_t)p->nphase * sizeof(int32_t));
    if (p->ncoef) std::memcpy(t.host.data() + o.coef, coef, (size_t)p->ncoef * 16);
    if (p->nphase) std::memcpy(t.host.data() + o.phase_c, phase_c, (size_t)p->nphase * 16);
    if (!c.upload(t.tab, t.host)) return nullptr;
    t.key = p->plan_key;
    std::memcpy(t.sig, sig, sizeof(sig));
    return (const char *)t.tab.p;
}

// total[0 .. 1] = the power sums of the two columns
bool power(Call &c, PowerArgs &a) {
    Work &w = *c.w;
    a.nb = grid_blocks(a.N, kBlock, kMaxBlocks);
    if (!c.need(w.red, (size_t)2 * kMaxBlocks * sizeof(double)) || !c.need(w.total, 2 * sizeof(double))) return false;
    a.part = (double *)w.red.p, a.total = (double *)w.total.p;
    k_power<<<dim3(a.nb, 2), kBlock, 0, w.st>>>(a);
    k_power_fin<<<1, 64, 0, w.st>>>(a);
    return c.launched();
}
bool stage(Call &c, const PowerArgs &pw, int round, cx<double> *out) {
    StageArgs s{};
    s.in[0] = pw.in[0], s.in[1] = pw.in[1], s.stride = pw.stride, s.in_c64 = pw.in_c64, s.round = round, s.total = pw.total;
    s.out = out, s.N = pw.N;
    k_stage<<<dim3(pw.nb, 2), kBlock, 0, c.w->st>>>(s);
    return c.launched();
}

}  // namespace

int nlin_run(int device, const ssf_nlin_params *p, const int32_t *pass, const double *coef, const int32_t *nidx, const int32_t *phase_m,
             const double *phase_c, const void *x, const void *y, void *out0, void *out1, void *out2, void *out3, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const long long N = p->n;
    const bool in_c64 = p->in_dtype == SSF_C64, prec_c64 = p->prec == SSF_C64, field = p->entry == SSF_NLIN_FIELD;
    const size_t esz = in_c64 ? 8 : 16, psz = prec_c64 ? 8 : 16;
    void *user[4] = {out0, out1, out2, out3};
    const size_t out_bytes[4] = {field ? (size_t)N * 2 * esz : (size_t)N * psz, field ? 0 : (size_t)N * psz, field ? 0 : (size_t)N * 8,
                                 field ? 0 : (size_t)N * 8};
    const int nout = field ? 1 : 4;
    FinishArgs f{};
    for (int k = 0; k < nout; ++k)
        if (!(f.out[k] = c.target(user[k], w.out[k], out_bytes[k]))) return c.rc;
    PowerArgs pw{};
    pw.N = N, pw.in_c64 = in_c64;
    if (field) {
        const char *e = (const char *)c.input(x, w.in0, (size_t)N * 2 * esz);
        if (!e) return c.rc;
        pw.in[0] = e, pw.in[1] = e + esz, pw.stride = 2;
    } else {
        pw.stride = 1;
        if (!(pw.in[0] = c.input(x, w.in0, (size_t)N * esz)) || !(pw.in[1] = c.input(y, w.in1, (size_t)N * esz))) return c.rc;
    }
    const char *tab = tables(c, p, pass, coef, nidx, phase_m, phase_c);
    if (!tab) return c.rc;
    const TableOffsets o = offsets(p);
    if (!c.need(w.xs, (size_t)2 * N * sizeof(cx<double>))) return c.rc;
    cx<double> *xs = (cx<double> *)w.xs.p;
    if (!power(c, pw)) return c.rc;
    if (field) {
        // pnorm per column, in the input's precision; then the calculation's own normalisation of that
        if (!c.need(w.e1, (size_t)2 * N * sizeof(cx<double>))) return c.rc;
        cx<double> *e1 = (cx<double> *)w.e1.p;
        if (!stage(c, pw, in_c64, e1)) return c.rc;
        pw.in[0] = e1, pw.in[1] = e1 + N, pw.stride = 1, pw.in_c64 = 0;
        if (!power(c, pw)) return c.rc;
        f.e1 = e1;
    }
    if (!stage(c, pw, in_c64 || prec_c64, xs)) return c.rc;
    const int split = split_for(N, p->npass);
    if (split > 0) {
        if (!c.need(w.part, (size_t)split * 2 * N * sizeof(cx<double>))) return c.rc;
        MainArgs m{};
        m.xs = xs, m.part = (cx<double> *)w.part.p, m.pass = (const int *)(tab + o.pass), m.coef = (const cx<double> *)(tab + o.coef);
        m.nidx = (const int *)(tab + o.nidx), m.N = N, m.L = p->L, m.npass = p->npass, m.split = split;
        const dim3 grid((unsigned)tiles_for(N), (unsigned)split);
        const size_t lds = lds_bytes_for(p->L);             // 50 KiB at L = 128: inside the default limit
        if (p->dense) k_main<true><<<grid, kLanes, lds, w.st>>>(m);
        else k_main<false><<<grid, kLanes, lds, w.st>>>(m);
        if (!c.launched()) return c.rc;
    }
    f.xs = xs, f.part = (const cx<double> *)w.part.p, f.phase_m = (const int *)(tab + o.phase_m), f.phase_c = (const cx<double> *)(tab + o.phase_c);
    f.N = N, f.split = split, f.nphase = p->nphase, f.ispm_offset = p->ispm_offset, f.entry = field ? 1 : 0, f.prec_c64 = prec_c64;
    f.out_c64 = in_c64, f.ispm_im = p->ispm_im, f.peak = p->peak_power;
    k_finish<<<grid_blocks(N, kBlock, 8192), kBlock, 0, w.st>>>(f);
    if (!c.launched()) return c.rc;
    for (int k = 0; k < nout; ++k)
        if (!c.deliver(user[k], f.out[k], out_bytes[k])) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
