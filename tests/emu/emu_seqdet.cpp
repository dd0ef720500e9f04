// emu_seqdet.cpp -- g++ walk of the bodies of seqdet_kernels.h in the layout of engine_seqdet.hip's kernels: one lane per next
// state, path metrics double-buffered, y staged kStageChunk samples at a time, survivor rows gathered kSurvChunk steps at a time
// and flushed in 4-byte words, the final minimum by a lane-strided scan and a butterfly over (metric, index), then the three-step
// traceback (per-chunk maps, their composition in staged blocks, one walker per chunk); detector one symbol at a time; autocorr by
// workgroups, tiles, wavefronts and lanes with the shuffle tree of block_reduce.h.
//   emu_seqdet in.bin out.bin
// in.bin:  int64 head[9] = mode (0 mlse, 1 detector, 2 autocorr), n, cols, cx, M, taps, rule, nTaps, reps; double sigma2; then doubles:
//          mlse h (2 taps), c (2 M), y (n cols, interleaved pairs if cx) | detector c (2 M), logpx (M), r (n) | autocorr x (n)
// out.bin: doubles: mlse out (as y), final metric (cols), states, kernel, chunk, survivor bytes, seconds of the fastest repetition
//          | detector decided (as r), indices (n) | autocorr r (nTaps)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "seqdet_kernels.h"

using namespace ssf::sq;

static double wave_sum_down(double *v) {                  // br::wave_sum_down: lane 0's value
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) v[l] += v[l + o];
    return v[0];
}

template <bool CX>
static void mlse_column(const Trellis &t, const double *h, const double *c, const double *y, long long n, int cols, int col, uint8_t *surv,
                        uint16_t *maps, int *ends, double *out, double &fin_metric) {
    const int W = CX ? 2 : 1;
    std::vector<double> pm(2 * kMaxStates, 0.0), term(2 * kMaxM, 0.0), br(t.S), bi(t.S), ys(2 * kStageChunk, 0.0);
    std::vector<uint8_t> sv((size_t)kSurvChunk * kMaxStates, 0);
    for (int j = 0; j < t.M; ++j) candidate_term(t, h, c, j, term[2 * j], term[2 * j + 1]);
    for (int ns = 0; ns < t.S; ++ns) state_base(t, h, c, ns, br[ns], bi[ns]);
    int cur = 0;
    for (long long c0 = 0; c0 < n; c0 += kStageChunk) {
        const int cnt = n - c0 < kStageChunk ? (int)(n - c0) : kStageChunk;
        for (int i = 0; i < cnt; ++i) {
            ys[i] = y[((c0 + i) * cols + col) * W];
            if (CX) ys[kStageChunk + i] = y[((c0 + i) * cols + col) * W + 1];
        }
        for (int i = 0; i < cnt; ++i) {
            const int tt = i % kSurvChunk;
            for (int ns = 0; ns < t.S; ++ns) {           // the lanes
                double best;
                const int j = acs_any<CX>(t, &pm[cur * kMaxStates], term.data(), ns, br[ns], bi[ns], ys[i], CX ? ys[kStageChunk + i] : 0.0, best);
                pm[(cur ^ 1) * kMaxStates + ns] = best;
                sv[tt * t.Sp + ns] = (uint8_t)j;
            }
            cur ^= 1;
            if (tt == kSurvChunk - 1 || i == cnt - 1) std::memcpy(surv + (c0 + i - tt) * t.Sp, sv.data(), (size_t)(tt + 1) * t.Sp / 4 * 4);
        }
    }
    // the final minimum: lane-strided scan, then the butterfly
    double d[64];
    int bs[64];
    for (int l = 0; l < 64; ++l) {
        d[l] = INFINITY, bs[l] = kMaxStates;
        for (int s = l; s < t.S; s += 64)
            if (pm[cur * kMaxStates + s] < d[l]) d[l] = pm[cur * kMaxStates + s], bs[l] = s;
    }
    for (int o = 32; o > 0; o >>= 1) {
        double d2[64];
        int s2[64];
        for (int l = 0; l < 64; ++l) d2[l] = d[l ^ o], s2[l] = bs[l ^ o];
        for (int l = 0; l < 64; ++l) argmin_merge(d[l], bs[l], d2[l], s2[l]);
    }
    fin_metric = d[0];
    const int fin_state = bs[0] < t.S ? bs[0] : 0;

    const long long nchunks = (n + kSurvChunk - 1) / kSurvChunk;
    for (long long ch = 0; ch < nchunks; ++ch) {          // step 1: the maps
        const long long n0 = ch * kSurvChunk;
        const int cnt = n - n0 < kSurvChunk ? (int)(n - n0) : kSurvChunk;
        for (int e = 0; e < t.S; ++e) {
            int s = e;
            for (int tt = cnt - 1; tt >= 0; --tt) s = step_back(t, surv + (n0 + tt) * t.Sp, s);
            maps[ch * t.S + e] = (uint16_t)s;
        }
    }
    const long long per = kComposeLds / t.S;              // step 2: the composition, a staged block at a time
    std::vector<uint16_t> buf(kComposeLds);
    int state = fin_state;
    for (long long hi = nchunks; hi > 0; hi -= per) {
        const long long lo = hi > per ? hi - per : 0;
        std::memcpy(buf.data(), maps + lo * t.S, (size_t)(hi - lo) * t.S * sizeof(uint16_t));
        for (long long ch = hi - 1; ch >= lo; --ch) {
            ends[ch] = state;
            state = buf[(ch - lo) * t.S + state];
        }
    }
    for (long long ch = 0; ch < nchunks; ++ch) {          // step 3: the walkers
        const long long n0 = ch * kSurvChunk;
        const int cnt = n - n0 < kSurvChunk ? (int)(n - n0) : kSurvChunk;
        int s = ends[ch];
        for (int tt = cnt - 1; tt >= 0; --tt) {
            const int j = surv[(n0 + tt) * t.Sp + s];
            const int k = decided_symbol(t, s, j);
            out[((n0 + tt) * cols + col) * W] = c[2 * k];
            if (CX) out[((n0 + tt) * cols + col) * W + 1] = c[2 * k + 1];
            s = predecessor(t, s, j);
        }
    }
}

static std::vector<double> autocorr(const double *x, long long n, int nTaps) {
    const int nb = ac_blocks(n);
    const long long tpb = ac_tiles_per_block(n, nb);
    std::vector<double> part((size_t)nb * nTaps, 0.0), w(kAcMaxTaps - 1 + kAcTile), r(nTaps);
    for (int b = 0; b < nb; ++b) {
        std::vector<double> acc(kAcMaxTaps, 0.0);
        for (long long ti = 0; ti < tpb; ++ti) {
            const long long t0 = ((long long)b * tpb + ti) * kAcTile;
            if (t0 >= n) break;
            const int cnt = n - t0 < kAcTile ? (int)(n - t0) : kAcTile;
            for (int i = 0; i < kAcMaxTaps - 1 + cnt; ++i) {
                const long long s = t0 - (kAcMaxTaps - 1) + i;
                w[i] = s >= 0 ? x[s] : 0.0;
            }
            for (int k = 0; k < nTaps; ++k) {             // lag k belongs to wavefront k % 4
                double v[64];
                for (int lane = 0; lane < 64; ++lane) v[lane] = ac_lane_sum(w.data(), k, lane, t0, cnt);
                acc[k] += wave_sum_down(v);
            }
        }
        for (int k = 0; k < nTaps; ++k) part[(size_t)b * nTaps + k] = acc[k];
    }
    for (int k = 0; k < nTaps; ++k) {                     // br::wave_sum_partials, then the division
        double a[64];
        for (int l = 0; l < 64; ++l) {
            a[l] = 0.0;
            for (int b = l; b < nb; b += 64) a[l] += part[(size_t)b * nTaps + k];
        }
        r[k] = wave_sum_down(a) / (double)(n - k);
    }
    return r;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[9];
    double sigma2;
    if (std::fread(head, sizeof(long long), 9, f) != 9 || std::fread(&sigma2, sizeof(double), 1, f) != 1) return 2;
    const long long mode = head[0], n = head[1];
    const int cols = (int)head[2], cx = (int)head[3], M = (int)head[4], taps = (int)head[5], rule = (int)head[6], nTaps = (int)head[7];
    const int reps = head[8] > 0 ? (int)head[8] : 1, W = cx ? 2 : 1;
    auto read = [&](size_t count) {
        std::vector<double> v(count);
        if (count && std::fread(v.data(), sizeof(double), count, f) != count) std::exit(2);
        return v;
    };
    std::vector<double> res;
    if (mode == 0) {
        if (M < 1 || M > kMaxM || taps < 1 || taps > kMaxTaps || states_of(M, taps - 1) == 0 || cols < 1 || cols > kMaxCols || n < 1) return 3;
        const std::vector<double> h = read(2 * (size_t)taps), c = read(2 * (size_t)M), y = read((size_t)n * cols * W);
        const Trellis t = trellis_of(M, taps, cx);
        const long long nchunks = (n + kSurvChunk - 1) / kSurvChunk, colstride = (n * t.Sp + 15) / 16 * 16;
        std::vector<uint8_t> surv((size_t)colstride);
        std::vector<uint16_t> maps((size_t)nchunks * t.S);
        std::vector<int> ends((size_t)nchunks);
        std::vector<double> out((size_t)n * cols * W), fin(cols);
        double best = 1e300;
        for (int rep = 0; rep < reps; ++rep) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int col = 0; col < cols; ++col) {
                if (cx) mlse_column<true>(t, h.data(), c.data(), y.data(), n, cols, col, surv.data(), maps.data(), ends.data(), out.data(), fin[col]);
                else mlse_column<false>(t, h.data(), c.data(), y.data(), n, cols, col, surv.data(), maps.data(), ends.data(), out.data(), fin[col]);
            }
            const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            best = s < best ? s : best;
        }
        res = out;
        res.insert(res.end(), fin.begin(), fin.end());
        const double info[5] = {(double)t.S, t.S <= 64 ? 0.0 : 1.0, (double)kSurvChunk, (double)colstride * cols, best};
        res.insert(res.end(), info, info + 5);
    } else if (mode == 1) {
        if (M < 1 || M > kMaxM || n < 1) return 3;
        const std::vector<double> c = read(2 * (size_t)M), lp = read((size_t)M), r = read((size_t)n * W);
        res.assign((size_t)n * W + n, 0.0);
        for (long long i = 0; i < n; ++i) {
            const int m = detect(c.data(), lp.data(), M, rule, sigma2, r[i * W], cx ? r[i * W + 1] : 0.0);
            res[i * W] = c[2 * m];
            if (cx) res[i * W + 1] = c[2 * m + 1];
            res[(size_t)n * W + i] = m;
        }
    } else {
        if (nTaps < 1 || nTaps > kAcMaxTaps || n < nTaps) return 3;
        const std::vector<double> x = read((size_t)n);
        res = autocorr(x.data(), n, nTaps);
    }
    std::fclose(f);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(res.data(), sizeof(double), res.size(), o) != res.size()) return 2;
    std::fclose(o);
    return 0;
}
