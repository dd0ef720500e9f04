// emu_ofdm.cpp -- the OFDM kernels of engine_ofdm.hip without a GPU (test-only): includes opticommpy_amd/csrc/ofdm_kernels.h, the
// bodies the gfx950 kernels call, and walks them with g++ in the engine's launch geometry.  The register-and-LDS transforms need
// their barriers: every lane of a workgroup is a fiber (ucontext) and ctx.sync() hands over to the next one, so one round of the
// scheduler is one __syncthreads() interval.  rocFFT's place (lengths that are no power of two) is taken by a plain O(n^2) DFT in
// double; k_chan's sum over the frames is the engine's: lane-strided, then the shuffle-down tree.
//   emu_ofdm mod in.bin out.bin     int32 [Nfft, G, SpS, Ni, in_c64, out_c64, rocfft], int64 nframes, double pilot (re, im),
//                                   int32 src_map[SpS Nfft], the symbols;  out: the samples
//   emu_ofdm demod in.bin out.bin   int32 [Nfft, G, Ns, Ni, Np, in_c64, rocfft], int64 nframes, double pilot (re, im), int32
//                                   bin_carrier[Nfft], data[Ni], pilots[Np], hi[Ns] (the last two with Np > 0), the signal;
//                                   out: the symbols, then (Np > 0) Ns complex128 of H
#include <ucontext.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "ofdm_kernels.h"

using namespace ssf::ofdm;

static void need(bool ok, const char *what) {
    if (!ok) {
        std::fprintf(stderr, "emu_ofdm: %s\n", what);
        std::exit(2);
    }
}
template <class T> static void rd(FILE *f, T *p, size_t n) { need(n == 0 || std::fread(p, sizeof(T), n, f) == n, "short input"); }
template <class T> static void wr(FILE *f, const T *p, size_t n) { need(n == 0 || std::fwrite(p, sizeof(T), n, f) == n, "short output"); }

// ---- a workgroup whose lanes are fibers
struct EmuCtx {
    int tid, bid, nthreads, nblocks;
    char *lds;
    static constexpr bool kWaveOps = false;
    void sync();
};
static ucontext_t g_main, *g_cur;
static const std::function<void(EmuCtx &)> *g_body;
static EmuCtx *g_ctx;
static bool g_yielded;
void EmuCtx::sync() {
    g_yielded = true;
    swapcontext(g_cur, &g_main);
}
static void fiber_entry() { (*g_body)(*g_ctx); }

static void run_grid(long long nblocks, int nthreads, size_t lds_bytes, const std::function<void(EmuCtx &)> &body) {
    constexpr size_t kStack = 64 * 1024;
    static std::vector<char> stacks;          // kept from launch to launch
    if (stacks.size() < (size_t)nthreads * kStack) stacks.resize((size_t)nthreads * kStack);
    std::vector<char> lds(lds_bytes + 16), done((size_t)nthreads);
    std::vector<ucontext_t> uc((size_t)nthreads);
    std::vector<EmuCtx> ctx((size_t)nthreads);
    g_body = &body;
    for (long long bid = 0; bid < nblocks; ++bid) {
        for (int t = 0; t < nthreads; ++t) {
            ctx[t] = EmuCtx{t, (int)bid, nthreads, (int)nblocks, lds.data()};
            getcontext(&uc[t]);
            uc[t].uc_stack.ss_sp = stacks.data() + (size_t)t * kStack;
            uc[t].uc_stack.ss_size = kStack;
            uc[t].uc_link = &g_main;          // a lane that returns from the body comes back to the scheduler
            makecontext(&uc[t], fiber_entry, 0);
            done[t] = 0;
        }
        for (int alive = nthreads; alive > 0;) {
            alive = 0;
            for (int t = 0; t < nthreads; ++t) {
                if (done[t]) continue;
                g_cur = &uc[t], g_ctx = &ctx[t], g_yielded = false;
                swapcontext(&g_main, &uc[t]);
                if (g_yielded) ++alive;
                else done[t] = 1;
            }
        }
    }
}
// element-wise kernels: no barrier inside, the lanes run one after the other
template <class F> static void run_flat(long long count, F body) {
    const long long nb = (count + kBlock - 1) / kBlock;
    const int nblocks = (int)(nb < 1 ? 1 : nb > 8192 ? 8192 : nb);      // eng::grid_blocks(count, kBlock, 8192)
    for (int bid = 0; bid < nblocks; ++bid)
        for (int tid = 0; tid < kBlock; ++tid) {
            EmuCtx c{tid, bid, kBlock, nblocks, nullptr};
            body(c);
        }
}

// what stands where rocFFT does: `batch` unnormalised transforms of n points in place, sign -1 forward, +1 inverse
static void dft_batch(cx<double> *x, int n, long long batch, int sign) {
    std::vector<cx<double>> w((size_t)n), y((size_t)n);
    for (int k = 0; k < n; ++k) {
        const double a = sign * ssf::fused::kTwoPi * (double)k / (double)n;
        w[k] = mk<double>(std::cos(a), std::sin(a));
    }
    for (long long f = 0; f < batch; ++f) {
        cx<double> *v = x + f * n;
        for (int k = 0; k < n; ++k) {
            cx<double> s = mk<double>(0.0, 0.0);
            for (int j = 0; j < n; ++j) s = s + v[j] * w[(size_t)((long long)j * k % n)];
            y[k] = s;
        }
        for (int k = 0; k < n; ++k) v[k] = y[k];
    }
}

template <class F> static void dispatch(int lg, F &&f) {
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

static int run_mod(FILE *fi, FILE *fo) {
    int h[7];
    long long F;
    double pilot[2];
    rd(fi, h, 7), rd(fi, &F, 1), rd(fi, pilot, 2);
    const int Nfft = h[0], G = h[1], SpS = h[2], Ni = h[3], in_c64 = h[4], out_c64 = h[5], rocfft = h[6];
    need(Nfft >= 4 && G >= 0 && G <= Nfft && SpS >= 1 && Ni >= 1 && Ni <= Nfft && F >= 1, "bad header");
    const int L = SpS * Nfft;
    std::vector<int> map((size_t)L), tab;
    rd(fi, map.data(), map.size());
    for (int k = 0; k < L; ++k) need((map[k] & 3) != 3 && map[k] >= 0 && (map[k] >> 3) < Ni, "bad code in src_map");
    std::vector<char> symb((size_t)F * Ni * (in_c64 ? 8 : 16)), out((size_t)F * SpS * (Nfft + G) * (out_c64 ? 8 : 16), (char)0xEE);
    rd(fi, symb.data(), symb.size());
    const bool lds = !rocfft && lds_length(L);
    const int lg = lds ? log2_exact(L) : 0;
    mod_table(map.data(), L, lg, tab);
    std::vector<cx<double>> work;
    ModArgs a{};
    a.map = tab.data(), a.symb = symb.data(), a.out = out.data(), a.nframes = F, a.L = L, a.Ni = Ni, a.pre = SpS * G;
    a.in_c64 = in_c64, a.out_c64 = out_c64, a.pilot_re = (double)(float)pilot[0], a.pilot_im = (double)(float)pilot[1];
    a.scale = std::sqrt((double)L) / (double)L;
    if (lds) {
        dispatch(lg, [&](auto lgc) {
            constexpr int LG = decltype(lgc)::value;
            run_grid((F + frames_per_workgroup(LG) - 1) / frames_per_workgroup(LG), threads_for(LG), lds_bytes_for(LG),
                     [&](EmuCtx &c) { mod_body<LG>(c, a); });
        });
    } else {
        work.resize((size_t)F * L);
        a.work = work.data();
        run_flat(F * L, [&](EmuCtx &c) { mod_scatter_body(c, a); });
        dft_batch(a.work, L, F, +1);
        run_flat(F * L, [&](EmuCtx &c) { mod_store_body(c, a); });
    }
    wr(fo, out.data(), out.size());
    return 0;
}

// k_chan's sums: lane l adds the frames l, l + 64, ..., then v[l] += v[l + o] for o = 32, 16 .. 1 (lane 0 is the wave's sum)
static double wave_sum_frames(const double *x, long long n) {
    double v[128] = {0};
    for (int l = 0; l < 64; ++l)
        for (long long f = l; f < n; f += 64) v[l] += x[f];
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < 64; ++l) v[l] += l + o < 64 ? v[l + o] : v[l];
    return v[0];
}

static int run_demod(FILE *fi, FILE *fo) {
    int h[7];
    long long F;
    double pilot[2];
    rd(fi, h, 7), rd(fi, &F, 1), rd(fi, pilot, 2);
    const int Nfft = h[0], G = h[1], Ns = h[2], Ni = h[3], Np = h[4], in_c64 = h[5], rocfft = h[6];
    need(Nfft >= 4 && G >= 0 && G <= Nfft && Ns >= 1 && Ns <= Nfft && Ni >= 1 && Np >= 0 && Np != 1 && Ni + Np <= Ns && F >= 1, "bad header");
    std::vector<int> bins((size_t)Nfft), data((size_t)Ni), pilots((size_t)Np), hi(Np ? (size_t)Ns : 0), tab;
    rd(fi, bins.data(), bins.size()), rd(fi, data.data(), data.size()), rd(fi, pilots.data(), pilots.size()), rd(fi, hi.data(), hi.size());
    for (int v : bins) need(v >= -1 && v < Ns, "bad bin_carrier");
    for (int v : data) need(v >= 0 && v < Ns, "bad data carrier");
    for (int j = 0; j < Np; ++j) need(pilots[j] >= 0 && pilots[j] < Ns && (j == 0 || pilots[j] > pilots[j - 1]), "bad pilot carrier");
    for (int v : hi) need(v >= 1 && v < Np, "bad segment");
    const size_t esz = in_c64 ? 8 : 16;
    std::vector<char> sig((size_t)F * (Nfft + G) * esz), out((size_t)F * Ni * esz, (char)0xEE);
    rd(fi, sig.data(), sig.size());
    const bool lds = !rocfft && lds_length(Nfft);
    const int lg = lds ? log2_exact(Nfft) : 0;
    const DemodTables t = demod_tables(bins.data(), data.data(), pilots.data(), hi.data(), Nfft, Ns, Ni, Np, lg, tab);
    std::vector<cx<double>> work, Y((size_t)(Np ? F * Ns : 0)), H((size_t)Ns);
    std::vector<double> habs((size_t)F * Np), hpha((size_t)F * Np), mean((size_t)2 * Np);
    DemodArgs a{};
    a.dest = tab.data() + t.dest, a.pidx = tab.data() + t.pidx, a.sig = sig.data(), a.out = out.data(), a.Y = Y.data();
    a.habs = habs.data(), a.hpha = hpha.data(), a.nframes = F, a.Nfft = Nfft, a.G = G, a.Ns = Ns, a.Ni = Ni, a.Np = Np, a.in_c64 = in_c64;
    a.pilot_re = pilot[0], a.pilot_im = pilot[1], a.scale = 1.0 / std::sqrt((double)Nfft);
    if (lds) {
        dispatch(lg, [&](auto lgc) {
            constexpr int LG = decltype(lgc)::value;
            run_grid((F + frames_per_workgroup(LG) - 1) / frames_per_workgroup(LG), threads_for(LG), lds_bytes_for(LG),
                     [&](EmuCtx &c) { demod_body<LG>(c, a); });
        });
    } else {
        work.resize((size_t)F * Nfft);
        a.work = work.data();
        run_flat(F * Nfft, [&](EmuCtx &c) { demod_gather_body(c, a); });
        dft_batch(a.work, Nfft, F, -1);
        run_flat(F * Nfft, [&](EmuCtx &c) { demod_store_body(c, a); });
    }
    if (Np) {
        ChanArgs c{};
        c.habs = habs.data(), c.hpha = hpha.data(), c.mean = mean.data(), c.pilots = tab.data() + t.pilots, c.hi = tab.data() + t.hi;
        c.H = H.data(), c.nframes = F, c.Np = Np, c.Ns = Ns;
        for (int j = 0; j < Np; ++j) {
            mean[j] = wave_sum_frames(c.habs + (long long)j * F, F) / (double)F;
            mean[Np + j] = wave_sum_frames(c.hpha + (long long)j * F, F) / (double)F;
        }
        for (int s = 0; s < Ns; ++s) H[s] = chan_value(c, s);
        EqArgs e{};
        e.Y = Y.data(), e.H = H.data(), e.carrier = tab.data() + t.carrier, e.out = out.data(), e.nframes = F, e.Ns = Ns, e.Ni = Ni;
        e.out_c64 = in_c64;
        run_flat(F * Ni, [&](EmuCtx &x) { equalize_body(x, e); });
    }
    wr(fo, out.data(), out.size());
    if (Np) wr(fo, H.data(), H.size());
    return 0;
}

int main(int argc, char **argv) {
    need(argc == 4, "usage: emu_ofdm mod|demod in.bin out.bin");
    FILE *fi = std::fopen(argv[2], "rb"), *fo = std::fopen(argv[3], "wb");
    need(fi && fo, "cannot open files");
    const int rc = argv[1][0] == 'm' ? run_mod(fi, fo) : run_demod(fi, fo);
    std::fclose(fi);
    std::fclose(fo);
    return rc;
}
