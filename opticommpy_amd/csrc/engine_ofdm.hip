// engine_ofdm.hip -- OFDM modulation and demodulation on the device (ssf_ofdm_modulate, ssf_ofdm_demodulate of include/ssf.h).  The
// per-lane bodies are ofdm_kernels.h; here are the kernels that walk them and the launch sequences.
//   modulator     L = SpS Nfft a power of two, 16 .. 8192: k_mod<LG>, one launch.  Else k_mod_scatter -> rocFFT (batched, inverse)
//                 -> k_mod_store.
//   demodulator   Nfft a power of two, 16 .. 8192: k_demod<LG>; else k_demod_gather -> rocFFT (batched, forward) -> k_demod_store.
//                 Without pilots that is all: the stores gather the data carriers.  With pilots they leave every frame's spectrum and,
//                 per pilot and frame, |H_est| and its angle; k_chan (one workgroup) adds those over the frames -- a wave per pilot,
//                 lane-strided and then the shuffle tree of block_reduce.h, so a result repeats bit for bit -- divides, and draws the
//                 lines over the carriers; k_equalize divides and gathers.
// The carrier tables of the last call stay on the device: a call that names the same plan_key (and geometry) uploads nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <set>
#include <vector>

#include "block_reduce.h"
#include "dev_ctx.h"
#include "engine_host.h"
#include "ofdm_kernels.h"

namespace ssf {
namespace {
using namespace ofdm;
using namespace eng;

struct OfdmCtx : DevCtxCore {};
#define SSF_OFDM_CTX()                                                        \
    extern __shared__ __attribute__((aligned(16))) char ssf_smem[];           \
    OfdmCtx ctx{{(int)threadIdx.x, (int)blockIdx.x, (int)blockDim.x, (int)gridDim.x, ssf_smem}}

template <int LG> __global__ void __launch_bounds__(threads_for(LG)) k_mod(const ModArgs a) {
    SSF_OFDM_CTX();
    mod_body<LG>(ctx, a);
}
template <int LG> __global__ void __launch_bounds__(threads_for(LG)) k_demod(const DemodArgs a) {
    SSF_OFDM_CTX();
    demod_body<LG>(ctx, a);
}
__global__ void __launch_bounds__(kBlock) k_mod_scatter(const ModArgs a) {
    SSF_OFDM_CTX();
    mod_scatter_body(ctx, a);
}
__global__ void __launch_bounds__(kBlock) k_mod_store(const ModArgs a) {
    SSF_OFDM_CTX();
    mod_store_body(ctx, a);
}
__global__ void __launch_bounds__(kBlock) k_demod_gather(const DemodArgs a) {
    SSF_OFDM_CTX();
    demod_gather_body(ctx, a);
}
__global__ void __launch_bounds__(kBlock) k_demod_store(const DemodArgs a) {
    SSF_OFDM_CTX();
    demod_store_body(ctx, a);
}
__global__ void __launch_bounds__(kBlock) k_equalize(const EqArgs a) {
    SSF_OFDM_CTX();
    equalize_body(ctx, a);
}
// one workgroup: wave w takes the pilots w, w + 4, ...
__global__ void __launch_bounds__(kBlock) k_chan(const ChanArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < a.Np; j += kBlock / 64) {
        const double *m = a.habs + (long long)j * a.nframes, *g = a.hpha + (long long)j * a.nframes;
        double sm = 0.0, sg = 0.0;
        for (long long f = lane; f < a.nframes; f += 64) sm += m[f], sg += g[f];
        sm = br::wave_sum_down(sm), sg = br::wave_sum_down(sg);
        if (lane == 0) a.mean[j] = sm / (double)a.nframes, a.mean[a.Np + j] = sg / (double)a.nframes;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < a.Ns; c += kBlock) a.H[c] = chan_value(a, c);
}

struct Work : WorkBase {
    Buf in, out, work, Y, habs, hpha, mean, H, mod_tab, demod_tab;
    FftPlans plans;
    std::vector<int> host_mod, host_demod;    // kept for their capacity
    uint64_t mod_key = 0, demod_key = 0;      // what mod_tab / demod_tab hold (0: nothing that can be named)
    long long mod_sig[3] = {0, 0, 0}, demod_sig[6] = {0, 0, 0, 0, 0, 0};
    std::set<const void *> armed;             // kernels whose dynamic-LDS limit has been raised on this device
};
using Call = CallT<Work>;

template <class K> bool arm(Call &c, K kernel) {
    if (!c.w->armed.insert((const void *)kernel).second) return true;
    return c.ok(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024), "hipFuncSetAttribute");
}

// f(integral_constant<LG>) for the instantiation a transform of 2^lg points needs
template <class F> void dispatch(int lg, F &&f) {
    using std::integral_constant;
    switch (lg) {
    case 4: f(integral_constant<int, 4>{}); break;
    case 5: f(integral_constant<int, 5>{}); break;
    case 6: f(integral_constant<int, 6>{}); break;
    case 7: f(integral_constant<int, 7>{}); break;
    case 8: f(integral_constant<int, 8>{}); break;
    case 9: f(integral_constant<int, 9>{}); break;
    case 10: f(integral_constant<int, 10>{}); break;
    case 11: f(integral_constant<int, 11>{}); break;
    case 12: f(integral_constant<int, 12>{}); break;
    default: f(integral_constant<int, 13>{}); break;
    }
}

}  // namespace

int ofdm_modulate(int device, const ssf_ofdm_params *p, const int32_t *src_map, const void *symb, void *out, std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const long long F = p->nframes, L = (long long)p->SpS * p->Nfft;
    const bool lds = p->route != SSF_OFDM_ROCFFT && lds_length(L);
    const int lg = lds ? log2_exact(L) : 0;
    const size_t esz_in = p->in_dtype == SSF_C64 ? 8 : 16, esz_out = p->out_dtype == SSF_C64 ? 8 : 16;
    const size_t out_bytes = (size_t)F * (size_t)(L + (long long)p->SpS * p->G) * esz_out;
    ModArgs a{};
    a.nframes = F, a.L = (int)L, a.Ni = p->Ni, a.pre = p->SpS * p->G;
    a.in_c64 = p->in_dtype == SSF_C64, a.out_c64 = p->out_dtype == SSF_C64;
    a.pilot_re = (double)(float)p->pilot_re, a.pilot_im = (double)(float)p->pilot_im;
    a.scale = std::sqrt((double)L) / (double)L;
    a.out = c.target(out, w.out, out_bytes);
    if (!a.out) return c.rc;
    a.symb = c.input(symb, w.in, (size_t)F * p->Ni * esz_in);
    if (!a.symb) return c.rc;
    const long long sig[3] = {L, p->Ni, lds};
    if (!p->plan_key || p->plan_key != w.mod_key || sig[0] != w.mod_sig[0] || sig[1] != w.mod_sig[1] || sig[2] != w.mod_sig[2]) {
        w.mod_key = 0;
        mod_table(src_map, (int)L, lg, w.host_mod);
        if (!c.upload(w.mod_tab, w.host_mod)) return c.rc;
        w.mod_key = p->plan_key, w.mod_sig[0] = sig[0], w.mod_sig[1] = sig[1], w.mod_sig[2] = sig[2];
    }
    a.map = (const int *)w.mod_tab.p;
    if (lds) {
        bool armed = true;
        dispatch(lg, [&](auto lgc) {
            constexpr int LG = decltype(lgc)::value;
            if (!(armed = arm(c, k_mod<LG>))) return;
            const long long grid = (F + frames_per_workgroup(LG) - 1) / frames_per_workgroup(LG);
            k_mod<LG><<<(unsigned)grid, threads_for(LG), lds_bytes_for(LG), w.st>>>(a);
        });
        if (!armed || !c.launched()) return c.rc;
    } else {
        if (!c.need(w.work, (size_t)F * L * sizeof(cx<double>))) return c.rc;
        a.work = (cx<double> *)w.work.p;
        const int grid = grid_blocks(F * L, kBlock, 8192);
        k_mod_scatter<<<grid, kBlock, 0, w.st>>>(a);
        if (!c.launched()) return c.rc;
        if (!transform(c, a.work, L, (int)F, true)) return c.rc;
        k_mod_store<<<grid, kBlock, 0, w.st>>>(a);
        if (!c.launched()) return c.rc;
    }
    if (!c.deliver(out, a.out, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

int ofdm_demodulate(int device, const ssf_ofdm_params *p, const int32_t *bin_carrier, const int32_t *data_carriers,
                    const int32_t *pilot_carriers, const int32_t *pilot_hi, const void *sig_in, void *symb_out, void *H_out,
                    std::string *err) {
    Call c(device, err);
    if (c.rc) return c.rc;
    Work &w = *c.w;
    const long long F = p->nframes;
    const int Nfft = p->Nfft, Ns = p->Ns, Ni = p->Ni, Np = p->Np;
    const bool lds = p->route != SSF_OFDM_ROCFFT && lds_length(Nfft);
    const int lg = lds ? log2_exact(Nfft) : 0;
    const size_t esz = p->in_dtype == SSF_C64 ? 8 : 16;
    const size_t out_bytes = (size_t)F * Ni * esz, H_bytes = (size_t)Ns * sizeof(cx<double>);
    DemodArgs a{};
    a.nframes = F, a.Nfft = Nfft, a.G = p->G, a.Ns = Ns, a.Ni = Ni, a.Np = Np, a.in_c64 = p->in_dtype == SSF_C64;
    a.pilot_re = p->pilot_re, a.pilot_im = p->pilot_im, a.scale = 1.0 / std::sqrt((double)Nfft);
    a.out = c.target(symb_out, w.out, out_bytes);
    if (!a.out) return c.rc;
    a.sig = c.input(sig_in, w.in, (size_t)F * (size_t)(Nfft + p->G) * esz);
    if (!a.sig) return c.rc;
    const long long dsig[6] = {Nfft, Ns, Ni, Np, lds, 0};
    bool same = p->plan_key && p->plan_key == w.demod_key;
    for (int i = 0; i < 6; ++i) same = same && dsig[i] == w.demod_sig[i];
    if (!same) {
        w.demod_key = 0;
        demod_tables(bin_carrier, data_carriers, pilot_carriers, pilot_hi, Nfft, Ns, Ni, Np, lg, w.host_demod);
        if (!c.upload(w.demod_tab, w.host_demod)) return c.rc;
        w.demod_key = p->plan_key;
        for (int i = 0; i < 6; ++i) w.demod_sig[i] = dsig[i];
    }
    const DemodTables t = {0, Nfft, Nfft + Ns, Nfft + Ns + Ni, Nfft + Ns + Ni + Np};
    const int *tab = (const int *)w.demod_tab.p;
    a.dest = tab + t.dest, a.pidx = tab + t.pidx;
    if (Np) {
        if (!c.need(w.Y, (size_t)F * Ns * sizeof(cx<double>)) || !c.need(w.habs, (size_t)F * Np * sizeof(double)) ||
            !c.need(w.hpha, (size_t)F * Np * sizeof(double)) || !c.need(w.mean, (size_t)2 * Np * sizeof(double)))
            return c.rc;
        a.Y = (cx<double> *)w.Y.p, a.habs = (double *)w.habs.p, a.hpha = (double *)w.hpha.p;
    }
    if (lds) {
        bool armed = true;
        dispatch(lg, [&](auto lgc) {
            constexpr int LG = decltype(lgc)::value;
            if (!(armed = arm(c, k_demod<LG>))) return;
            const long long grid = (F + frames_per_workgroup(LG) - 1) / frames_per_workgroup(LG);
            k_demod<LG><<<(unsigned)grid, threads_for(LG), lds_bytes_for(LG), w.st>>>(a);
        });
        if (!armed || !c.launched()) return c.rc;
    } else {
        if (!c.need(w.work, (size_t)F * Nfft * sizeof(cx<double>))) return c.rc;
        a.work = (cx<double> *)w.work.p;
        const int grid = grid_blocks(F * Nfft, kBlock, 8192);
        k_demod_gather<<<grid, kBlock, 0, w.st>>>(a);
        if (!c.launched()) return c.rc;
        if (!transform(c, a.work, Nfft, (int)F, false)) return c.rc;
        k_demod_store<<<grid, kBlock, 0, w.st>>>(a);
        if (!c.launched()) return c.rc;
    }
    if (Np) {
        ChanArgs h{};
        h.habs = a.habs, h.hpha = a.hpha, h.mean = (double *)w.mean.p, h.pilots = tab + t.pilots, h.hi = tab + t.hi;
        h.nframes = F, h.Np = Np, h.Ns = Ns;
        h.H = (cx<double> *)c.target(H_out, w.H, H_bytes);
        if (!h.H) return c.rc;
        k_chan<<<1, kBlock, 0, w.st>>>(h);
        if (!c.launched()) return c.rc;
        EqArgs e{};
        e.Y = a.Y, e.H = h.H, e.carrier = tab + t.carrier, e.out = a.out, e.nframes = F, e.Ns = Ns, e.Ni = Ni, e.out_c64 = a.in_c64;
        k_equalize<<<grid_blocks(F * Ni, kBlock, 8192), kBlock, 0, w.st>>>(e);
        if (!c.launched()) return c.rc;
        if (!c.deliver(H_out, h.H, H_bytes)) return c.rc;
    }
    if (!c.deliver(symb_out, a.out, out_bytes)) return c.rc;
    if (!c.sync()) return c.rc;
    return SSF_OK;
}

}  // namespace ssf
