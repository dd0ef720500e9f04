// emu_imddtx.cpp -- the IM/DD transmitter's and the AWGN channel's kernels on the host: the bodies of
// opticommpy_amd/csrc/imddtx_kernels.h run over the grids of engine_rx.hip (tx_blocks / tx_ew_blocks workgroups; a reduction pass
// with 64 threads per workgroup that meet at ctx.sync(), an element-wise pass lane after lane), in the launch order of
// RxCore::pam_tx / modulate / awgn / stuff.  The pulse-shaping filter is not walked here (tests/test_emu_tx.py walks the overlap-save
// launch): the shaped signal comes in.  Built by tests/imddtx_cases.py with g++, also with -fsanitize=address,undefined.
//   emu_imddtx in.bin out.bin
// in.bin:  16 int64, then float64 values:
//   op 0 pam       (0, N, nPol)                                    mzmScale, Vpi, Vb, ER, amp; shaped (nPol, N)
//   op 1 modulate  (1, n, kind, u_cx, has_Ei)                      ei_re, ei_im, Vpi, VbI, VbQ, Vphi, ERI, ERQ; u; Ei
//   op 2 awgn      (2, n, ncols, in_cx, out_cx, cnoise, has_un, seed)   FsB, snr_lin; x; unit normals
//   op 3 stuff     (3, rows, w, factor)                            scale; in
// out.bin: the result's float64 values
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "imddtx_kernels.h"

using namespace ssf::rx;

namespace {

constexpr int kThreads = 64;
constexpr size_t kLds = 4096;

struct Barrier {
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0, generation = 0;
    void wait() {
        std::unique_lock<std::mutex> l(m);
        const int g = generation;
        if (++waiting == kThreads) {
            waiting = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(l, [&] { return g != generation; });
        }
    }
};

struct Ctx {
    int tid, bid, nthreads, nblocks;
    char *lds;
    Barrier *bar;
    static constexpr bool kWaveOps = false;
    void sync() {
        if (!bar) std::abort();            // (an element-wise body has no barrier)
        bar->wait();
    }
    double wave_sum(double v) { return v; }
    double wave_max(double v) { return v; }
};

// a reduction pass: kThreads threads walk the workgroups one after the other; the LDS is poisoned before each
void run_par(int nblocks, const std::function<void(Ctx &)> &body) {
    alignas(16) static char lds[kLds];
    Barrier bar;
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
        th.emplace_back([&, t] {
            for (int b = 0; b < nblocks; ++b) {
                if (t == 0) std::memset(lds, 0xFF, kLds);
                bar.wait();
                Ctx c{t, b, kThreads, nblocks, lds, &bar};
                body(c);
                bar.wait();
            }
        });
    for (auto &x : th) x.join();
}
// an element-wise pass at the device's geometry: kTxBlock lanes per workgroup
void run_seq(int nblocks, const std::function<void(Ctx &)> &body) {
    for (int b = 0; b < nblocks; ++b)
        for (int t = 0; t < kTxBlock; ++t) {
            Ctx c{t, b, kTxBlock, nblocks, nullptr, nullptr};
            body(c);
        }
}

bool read_all(FILE *f, std::vector<double> &v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(double), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    long long hd[16];
    if (std::fread(hd, sizeof(long long), 16, f) != 16) return 4;
    std::vector<double> out;
    const int op = (int)hd[0];
    if (op == 0) {
        const long long N = hd[1];
        const int nPol = (int)hd[2], nb = tx_blocks(N);
        std::vector<double> prm, shaped;
        if (N < 1 || nPol < 1 || !read_all(f, prm, 5) || !read_all(f, shaped, (size_t)nPol * N)) return 4;
        std::vector<Cd> sig((size_t)N), res((size_t)N * nPol);
        std::vector<double> part(2 * (size_t)nb);
        std::memset(part.data(), 0xFF, sizeof(double) * part.size());
        double sp, sm;
        mzm_arms(prm[3], &sp, &sm);
        for (int mode = 0; mode < nPol; ++mode) {
            for (long long n = 0; n < N; ++n) sig[(size_t)n] = mk<double>(shaped[(size_t)mode * N + n], 0.0);
            const PamPeakArgs pa{sig.data(), part.data(), N};
            run_par(nb, [&](Ctx &c) { pam_peak_body(c, pa); });
            const PamMzmArgs ma{sig.data(), res.data(), part.data(), part.data() + nb, N, nb, nPol, mode, prm[0], prm[1], prm[2], sp, sm};
            run_par(nb, [&](Ctx &c) { pam_mzm_body(c, ma); });
            const PamFinishArgs fa{res.data(), part.data() + nb, N, nb, nPol, mode, prm[4]};
            run_par(nb, [&](Ctx &c) { pam_finish_body(c, fa); });
        }
        out.resize(2 * res.size());
        std::memcpy(out.data(), res.data(), sizeof(Cd) * res.size());
    } else if (op == 1) {
        const long long n = hd[1];
        const int kind = (int)hd[2], u_cx = (int)hd[3], has_Ei = (int)hd[4];
        std::vector<double> prm, u, Ei;
        if (n < 1 || !read_all(f, prm, 8) || !read_all(f, u, (size_t)n * (u_cx ? 2 : 1)) || !read_all(f, Ei, has_Ei ? 2 * (size_t)n : 0)) return 4;
        out.resize(2 * (size_t)n);
        const ModArgs a = mod_args(kind, n, u_cx, u.data(), has_Ei ? (const Cd *)Ei.data() : nullptr, prm[0], prm[1], prm[2], prm[3], prm[4],
                                   prm[5], prm[6], prm[7], (Cd *)out.data());
        run_seq(tx_ew_blocks(n), [&](Ctx &c) { modulate_body(c, a); });
    } else if (op == 2) {
        AwgnArgs a{};
        a.total = hd[1] * hd[2];
        a.ncols = (int)hd[2];
        a.in_cx = (int)hd[3];
        a.out_cx = (int)hd[4];
        a.cnoise = (int)hd[5];
        a.seed = (unsigned long long)hd[7];
        const int has_un = (int)hd[6];
        std::vector<double> prm, x, un;
        if (a.total < 1 || !read_all(f, prm, 2) || !read_all(f, x, (size_t)a.total * (a.in_cx ? 2 : 1)) ||
            !read_all(f, un, has_un ? (size_t)a.total * (a.cnoise ? 2 : 1) : 0))
            return 4;
        a.nb = tx_blocks(a.total * (a.in_cx ? 2 : 1));
        std::vector<double> part((size_t)a.nb);
        std::memset(part.data(), 0xFF, sizeof(double) * part.size());
        out.resize((size_t)a.total * (a.out_cx ? 2 : 1));
        a.x = x.data();
        a.un = has_un ? un.data() : nullptr;
        a.out = out.data();
        a.part = part.data();
        a.FsB = prm[0];
        a.snr_lin = prm[1];
        const PowerArgs pa{x.data(), part.data(), a.total * (a.in_cx ? 2 : 1)};
        run_par(a.nb, [&](Ctx &c) { power_body(c, pa); });
        run_par(tx_ew_blocks(a.total), [&](Ctx &c) { awgn_body(c, a); });
    } else if (op == 3) {
        StuffArgs a{};
        const long long rows = hd[1];
        a.w = (int)hd[2];
        a.factor = (int)hd[3];
        std::vector<double> prm, in;
        if (rows < 1 || a.w < 1 || a.factor < 1 || !read_all(f, prm, 1) || !read_all(f, in, (size_t)rows * a.w)) return 4;
        a.total = rows * a.factor * a.w;
        out.resize((size_t)a.total);
        std::memset(out.data(), 0xFF, sizeof(double) * out.size());
        a.in = in.data();
        a.out = out.data();
        a.scale = prm[0];
        run_seq(tx_ew_blocks(a.total), [&](Ctx &c) { stuff_body(c, a); });
    } else {
        return 5;
    }
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    std::fwrite(out.data(), sizeof(double), out.size(), o);
    std::fclose(o);
    return 0;
}
