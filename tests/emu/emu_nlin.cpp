// emu_nlin.cpp -- the perturbation-model kernels of engine_nlin.hip without a GPU (test-only): includes
// opticommpy_amd/csrc/nlin_kernels.h, the bodies the gfx950 kernels call, and walks them with g++ in the engine's launch geometry
// and launch sequence.  The main kernel forms its lines cooperatively between barriers: every lane of a workgroup is a fiber
// (ucontext) and ctx.sync() hands over to the next one, so one round of the scheduler is one __syncthreads() interval.  The power
// sums are the engine's: a grid-stride running value per lane, the shuffle-down tree per wave, ((w0 + w1) + w2) + w3 per
// workgroup, one wave over the partials.
//   emu_nlin in.bin out.bin     int32 [L, npass, ncoef, nphase, dense, entry, in_c64, prec_c64, ispm_offset, 0, 0, 0], int64 N,
//                               double [ispm_re, ispm_im, peak], int32 pass[4 npass], complex128 coef[ncoef], int32 nidx[ncoef],
//                               int32 phase_m[nphase], complex128 phase_c[nphase], then x and y (entry 0) or the (N, 2) field
//                               (entry 1);  out: dx, dy (prec), phi_x, phi_y (double) -- or nlin (N, 2)
//   emu_nlin bench L N          times main_body<dense> alone on random symbols, one core: prints the seconds and the terms
#include <ucontext.h>

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "nlin_kernels.h"

using namespace ssf::nlin;

static void need(bool ok, const char *what) {
    if (!ok) {
        std::fprintf(stderr, "emu_nlin: %s\n", what);
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
static int grid_blocks(long long count, int block, int max_blocks) {      // eng::grid_blocks
    const long long nb = (count + block - 1) / block;
    return (int)(nb < max_blocks ? nb : max_blocks);
}
template <class F> static void run_flat(int nblocks, F body) {
    for (int bid = 0; bid < nblocks; ++bid)
        for (int tid = 0; tid < kBlock; ++tid) {
            EmuCtx c{tid, bid, kBlock, nblocks, nullptr};
            body(c);
        }
}

// v[l] += v[l + o], o = 32, 16 .. 1: lane 0 ends with the wave's sum (a lane past the wave reads its own value)
static double wave_sum_down(double *v) {
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < 64; ++l) v[l] += l + o < 64 ? v[l + o] : v[l];
    return v[0];
}
// k_power and k_power_fin for one column
static double power_sum(const void *in, long long stride, int c64, long long N) {
    const int nb = grid_blocks(N, kBlock, kMaxBlocks);
    std::vector<double> part((size_t)nb);
    for (int b = 0; b < nb; ++b) {
        double w[4];
        for (int wave = 0; wave < 4; ++wave) {
            double v[64];
            for (int l = 0; l < 64; ++l) {
                double acc = 0.0;
                for (long long t = (long long)b * kBlock + wave * 64 + l; t < N; t += (long long)nb * kBlock) acc += power_term(in, t * stride, c64);
                v[l] = acc;
            }
            w[wave] = wave_sum_down(v);
        }
        part[b] = ((w[0] + w[1]) + w[2]) + w[3];
    }
    double v[64];
    for (int l = 0; l < 64; ++l) {
        double a = 0.0;
        for (int b = l; b < nb; b += 64) a += part[b];
        v[l] = a;
    }
    return wave_sum_down(v);
}

struct Columns {
    const void *in[2];
    long long stride;
    int c64;
};
static void stage(const Columns &c, long long N, int round, cx<double> *out) {
    double total[2] = {power_sum(c.in[0], c.stride, c.c64, N), power_sum(c.in[1], c.stride, c.c64, N)};
    StageArgs s{};
    s.in[0] = c.in[0], s.in[1] = c.in[1], s.stride = c.stride, s.in_c64 = c.c64, s.round = round, s.total = total, s.out = out, s.N = N;
    const int nb = grid_blocks(N, kBlock, kMaxBlocks);
    for (int col = 0; col < 2; ++col) run_flat(nb, [&](EmuCtx &x) { stage_body(x, s, col); });
}

static void run_main(const MainArgs &m, bool dense) {
    const long long tiles = tiles_for(m.N);
    for (int share = 0; share < m.split; ++share)
        run_grid(tiles, kLanes, lds_bytes_for(m.L), [&](EmuCtx &c) {
            if (dense) main_body<true>(c, m, (long long)c.bid, share);
            else main_body<false>(c, m, (long long)c.bid, share);
        });
}

static int run_file(const char *in, const char *outp) {
    FILE *fi = std::fopen(in, "rb"), *fo = std::fopen(outp, "wb");
    need(fi && fo, "cannot open files");
    int h[12];
    long long N;
    double sc[3];
    rd(fi, h, 12), rd(fi, &N, 1), rd(fi, sc, 3);
    const int L = h[0], npass = h[1], ncoef = h[2], nphase = h[3], dense = h[4], entry = h[5], in_c64 = h[6], prec_c64 = h[7], off = h[8];
    need(L >= 1 && L <= kMaxL && npass >= 0 && ncoef >= 0 && nphase >= 0 && N >= 1 && off >= -L && off <= L, "bad header");
    std::vector<int> pass((size_t)4 * npass), nidx((size_t)ncoef), pm((size_t)nphase);
    std::vector<cx<double>> coef((size_t)ncoef), pc((size_t)nphase);
    rd(fi, pass.data(), pass.size()), rd(fi, coef.data(), coef.size()), rd(fi, nidx.data(), nidx.size());
    rd(fi, pm.data(), pm.size()), rd(fi, pc.data(), pc.size());
    for (int p = 0; p < npass; ++p) {
        need(pass[4 * p] >= 0 && pass[4 * p] <= 2 && std::abs(pass[4 * p + 1]) <= L, "bad pass");
        need(pass[4 * p + 2] >= 0 && pass[4 * p + 3] >= 1 && pass[4 * p + 2] + pass[4 * p + 3] <= ncoef, "bad pass range");
        need(!dense || pass[4 * p + 3] == 2 * L + 1, "bad dense pass");
        need(pass[4 * p + 3] <= 2 * L + 1, "a pass holds more than 2L + 1 coefficients");
        for (int j = 1; !dense && j < pass[4 * p + 3]; ++j) need(nidx[pass[4 * p + 2] + j] > nidx[pass[4 * p + 2] + j - 1], "n does not rise");
    }
    for (int v : nidx) need(std::abs(v) <= L, "bad n");
    for (int v : pm) need(std::abs(v) <= L, "bad m");
    const size_t esz = in_c64 ? 8 : 16, psz = prec_c64 ? 8 : 16;
    std::vector<char> x((size_t)N * esz * (entry ? 2 : 1)), y(entry ? 0 : (size_t)N * esz);
    rd(fi, x.data(), x.size()), rd(fi, y.data(), y.size());
    std::vector<cx<double>> e1(entry ? (size_t)2 * N : 0), xs((size_t)2 * N);
    Columns c{{x.data(), entry ? x.data() + esz : y.data()}, entry ? 2 : 1, in_c64};
    if (entry) {
        stage(c, N, in_c64, e1.data());
        c = Columns{{e1.data(), e1.data() + N}, 1, 0};
    }
    stage(c, N, in_c64 || prec_c64, xs.data());
    const int split = split_for(N, npass);
    std::vector<cx<double>> part((size_t)split * 2 * N);
    MainArgs m{};
    m.xs = xs.data(), m.part = part.data(), m.pass = pass.data(), m.coef = coef.data(), m.nidx = nidx.data();
    m.N = N, m.L = L, m.npass = npass, m.split = split;
    run_main(m, dense != 0);
    std::vector<char> o0(entry ? (size_t)N * 2 * esz : (size_t)N * psz, (char)0xEE), o1(entry ? 0 : (size_t)N * psz, (char)0xEE);
    std::vector<double> o2(entry ? 0 : (size_t)N), o3(entry ? 0 : (size_t)N);
    FinishArgs f{};
    f.xs = xs.data(), f.e1 = e1.data(), f.part = part.data(), f.phase_m = pm.data(), f.phase_c = pc.data();
    f.out[0] = o0.data(), f.out[1] = o1.data(), f.out[2] = o2.data(), f.out[3] = o3.data();
    f.N = N, f.split = split, f.nphase = nphase, f.ispm_offset = off, f.entry = entry, f.prec_c64 = prec_c64, f.out_c64 = in_c64;
    f.ispm_im = sc[1], f.peak = sc[2];
    run_flat(grid_blocks(N, kBlock, 8192), [&](EmuCtx &k) { finish_body(k, f); });
    wr(fo, o0.data(), o0.size()), wr(fo, o1.data(), o1.size()), wr(fo, o2.data(), o2.size()), wr(fo, o3.data(), o3.size());
    std::fclose(fi);
    std::fclose(fo);
    return 0;
}

// the dense main kernel alone on one core: the figure tools/bench_nlin.py sets next to the device's
static int run_bench(int L, long long N) {
    need(L >= 1 && L <= kMaxL && N >= 1, "bench: L 1 .. 128, N >= 1");
    const int W = 2 * L + 1;
    std::vector<cx<double>> xs((size_t)2 * N), coef((size_t)W * W);
    unsigned s = 12345;
    auto rnd = [&] { return (double)((s = s * 1664525u + 1013904223u) >> 8) / 16777216.0 - 0.5; };
    for (auto &v : xs) v = mk<double>(rnd(), rnd());
    for (auto &v : coef) v = mk<double>(rnd(), rnd());
    std::vector<int> pass;
    for (int j = 0; j < W; ++j) pass.insert(pass.end(), {PASS_IFWM, j - L, j * W, W});
    const int split = split_for(N, W);
    std::vector<cx<double>> part((size_t)split * 2 * N);
    MainArgs m{};
    m.xs = xs.data(), m.part = part.data(), m.pass = pass.data(), m.coef = coef.data(), m.N = N, m.L = L, m.npass = W, m.split = split;
    const auto t0 = std::chrono::steady_clock::now();
    run_main(m, true);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double chk = 0.0;
    for (const auto &v : part) chk += v.re;
    std::printf("{\"L\": %d, \"N\": %lld, \"seconds\": %.6f, \"terms\": %.0f, \"checksum\": %.6e}\n", L, N, sec, (double)N * W * W, chk);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && argv[1][0] == 'b') return run_bench(std::atoi(argv[2]), std::atoll(argv[3]));
    need(argc == 3, "usage: emu_nlin in.bin out.bin | emu_nlin bench L N");
    return run_file(argv[1], argv[2]);
}
