// ssf_internal.h -- shared host-side declarations for libssf_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ssf.h"
#include "ssf_copy.h"
#include "ssf_derived.h"
#include "ssf_snapshots.h"

namespace ssf {

// Host-side trace accumulation shared by the engines.
struct TraceSink {
    ssf_trace *t = nullptr;
    int maxIter = 1;
    void begin(ssf_trace *tr, int mi) {
        t = tr;
        maxIter = mi > 0 ? mi : 1;
    }
    void step(double hz, int iters, const double *lims) {
        if (!t) return;
        if (t->count < t->capacity) {
            const int64_t i = t->count;
            if (t->hz) t->hz[i] = hz;
            if (t->iters) t->iters[i] = iters;
            if (t->lims)
                for (int k = 0; k < maxIter; ++k) t->lims[i * maxIter + k] = k < iters && lims ? lims[k] : NAN;
        }
        t->count++;
    }
};

// comm_rccl.hip: device-buffer all-gather on the caller's stream (no synchronisation)
int comm_allgather_on(ssf_comm *c, const void *send_dev, void *recv_dev, size_t bytes_per_rank, hipStream_t st);
int comm_nranks(const ssf_comm *c);
int comm_device(const ssf_comm *c);
const char *comm_error(const ssf_comm *c);

class Engine {
  public:
    virtual ~Engine() {}
    virtual int upload(const void *field, bool aos) = 0;
    virtual int execute(const ssf_params &p, int span_first, int span_last, const void *noise,
                        ssf_stats *stats, ssf_trace *trace) = 0;
    virtual int download(void *field, int which, bool aos) = 0;      // which: -1 current, >= 0 snapshot
    virtual int n_snapshots() const = 0;
    virtual int linear_channel(double Fs, double Fc, double alpha, double D, double L) = 0;
    virtual int id() const = 0;
    virtual int pipeline() const { return SSF_PIPE_DEVICE; }
    virtual int unit_stats(int, ssf_stats *) { return SSF_ERR_UNSUPPORTED; }
    virtual int set_lanes(int) { return SSF_OK; }
    virtual int set_coupling(ssf_reduce_fn, void *) { return SSF_ERR_UNSUPPORTED; }
    virtual int set_coupling_comm(ssf_comm *) { return SSF_ERR_UNSUPPORTED; }
    virtual int set_profiling(int) { return SSF_ERR_UNSUPPORTED; }
    virtual int kernel_times(ssf_kernel_times *) { return SSF_ERR_UNSUPPORTED; }
};

}  // namespace ssf

// the Tanner graph of ssf_ldpc_graph_create on its device: one allocation, four int32 arrays inside it
struct ssf_ldpc_graph {
    int device = 0, m = 0, n = 0, E = 0, max_dc = 0;
    int *d_all = nullptr, *d_co = nullptr, *d_ev = nullptr, *d_vo = nullptr, *d_ve = nullptr;
};

// the matrices of ssf_ldpc_encoder_create on their device: the parity rows as words (dense), or the CSR of A (sparse)
struct ssf_ldpc_encoder {
    int device = 0, form = 0, k = 0, rows = 0, W = 0, systematic = 0;
    uint64_t *d_P = nullptr;
    int *d_ptr = nullptr, *d_idx = nullptr;   // one allocation
};

struct ssf_plan {
    int device = 0;
    int64_t N = 0;
    int nrows = 0;
    int units = 1;               // rows form `units` independent fields (ssf_plan_set_units)
    int lanes = 1;               // plans sharing this GPU concurrently (ssf_plan_set_lanes)
    bool coupled = false;        // a coupling communicator / reducer is attached (ssf_set_coupling[_comm]): the engine must stay
    int precision = SSF_C128;
    int engine_id = 0;
    hipStream_t stream = nullptr;
    ssf::Engine *engine = nullptr;
    ssf_stats stats{};
    std::string err;
    bool has_field = false;
    ssf::Stager stager;
    ssf::SnapshotSink sink;      // destination of streamed snapshots (ssf_set_snapshot_sink), inactive by default
};

namespace ssf {

// Engine factories (engine_rocfft.hip, engine_fused.hip).  Return nullptr and fill
// plan->err on failure.
Engine *make_rocfft_engine(ssf_plan *plan);
Engine *make_fused_engine(ssf_plan *plan);
bool fused_supports(int64_t N, int nrows, int precision);
int fused_couple_reduce_selftest(int nranks, int npart, const double *parts, double *out5, std::string *err);
int fused_overlap_save(int device, int64_t sigLen, int nrows, int precision, int log2nfft, int K, const void *Hfft,
                        const void *in, void *out, std::string *err);

// Circular convolution of every row of an (nrows, M) block with one of two fixed kernels, M = 2^m, on the fused kernels
// (column FWD, row FFT . multiplier-array . IFFT, column INV: three launches on the plan's stream).  The general-length
// engine builds its length-N transforms from it (Bluestein): any N the reference accepts runs on the hand-written kernels.
class FusedConv {
  public:
    virtual ~FusedConv() {}
    virtual void *work() = 0;                                        // the (nrows, M) block, convolved in place
    virtual int set_kernel(int which, const void *b_host) = 0;       // M complex values (already scaled by 1 / M)
    virtual int run(int which) = 0;
    virtual std::string error() const = 0;
};
FusedConv *make_fused_conv(ssf_plan *plan, int64_t M, int nrows);

// FFT . H . IFFT of every row of an (nrows, N) block in ONE launch, N = 2^a 3^b 5^c small enough for a row to live in LDS
// (mixed_fft.h, at most 8192 values): the linear step of the general-length engine at the short notebook lengths
// (1500, 3000, 6000 ...), which the column x row split does not take (fewer than four factors of two) and a Bluestein
// convolution serves with three launches of two to four times the length.
class FusedRows {
  public:
    virtual ~FusedRows() {}
    // out = ifft(fft(in) * exp((lin_a + j lin_b w^2) hzh)) * scale * N, w = w_scale * fftfreq(N) (in may be out)
    virtual int lin(const void *in, void *out, double hzh, double lin_a, double lin_b, double w_scale, double scale) = 0;
    virtual std::string error() const = 0;
};
FusedRows *make_fused_rows(ssf_plan *plan, int64_t N, int nrows);      // nullptr: this length is not served
bool fused_rows_supports(int64_t N);
// general-length engine with its transforms on the fused kernels (Bluestein) instead of rocFFT; nullptr if N is out of range
Engine *make_general_engine(ssf_plan *plan);
bool general_supports(int64_t N, int nrows, int precision);

// receiver front-end (engine_rx.hip)
int rx_run(int device, int mode, int64_t N, int nmodes, const ssf_rx_params *p, const void *in0, const void *lo,
           const double *un, void *out, std::string *err);
int rx_fir(int device, int64_t sigLen, int ncols, int ntaps, const void *taps, const void *in, void *out, std::string *err);
int rx_axpy(int device, int64_t n, double alpha, const void *x, void *y, std::string *err);
int rx_fir_long(int device, int64_t inLen, int64_t outLen, int ncols, int64_t ntaps, const void *taps, int64_t shift, const void *in,
                void *out, std::string *err);
int rx_overlap_save(int device, int64_t sigLen, int ncols, int nfft, int K, const void *Hfft, const void *in, void *out,
                    std::string *err);
int rx_delay(int device, int64_t N, double delay, double Fs, const void *in, void *out, std::string *err);
int rx_chain(int device, int64_t N, const ssf_rx_params *p, const void *Es, const void *Elo, const void *taps, int ntaps, int SpSin,
             int decFactor, const void *edcH, int edcK, int edc_nfft, void *out, int32_t *sampDelay, std::string *err);
enum { kOptEdfa = 0, kOptPbs = 1, kOptHybrid = 2 };      // (= rx_kernels.h: OPT_EDFA / OPT_PBS / OPT_HYBRID)
int rx_optics(int device, int op, int64_t n, int ncols, double p0, double p1, unsigned long long seed, unsigned row0, const void *a,
              const void *b, void *o0, void *o1, std::string *err);
int mk_nlin_phase(int device, int64_t n, double gamma, const void *Ex, const void *Ey, const double *Pch, double *phi,
                  std::string *err);
int mk_convergence(int device, int64_t n, const void *xfd, const void *yfd, const void *xc, const void *yc, double *lim,
                   std::string *err);
int tx_wdm(int device, const ssf_tx_params *p, const void *symbols, const double *taps, const double *phi, const double *amp,
           const double *deltaF, void *out, double *power_out, std::string *err);
// the IM/DD transmitter and the AWGN channel (imddtx_kernels.h; arguments already checked by ssf_api.hip)
int tx_pam(int device, int64_t nSymbols, int SpS, int nPolModes, int ntaps, const double *symbols, const double *taps, double mzmScale,
           double Vpi, double Vb, double ER, double amp, void *out, std::string *err);
int tx_modulate(int device, int kind, int64_t n, int u_cx, const void *u, const void *Ei, double ei_re, double ei_im, double Vpi, double VbI,
                double VbQ, double Vphi, double ERI, double ERQ, void *out, std::string *err);
int ch_awgn(int device, int64_t n, int ncols, int in_cx, int out_cx, int cnoise, double FsB, double snr_lin, const void *x, const void *un,
            unsigned long long seed, void *out, std::string *err);
int tx_stuff(int device, int64_t rows, int w, int factor, double scale, const void *in, void *out, std::string *err);
int rx_decimate(int device, int64_t N, int ncols, int SpSin, int decFactor, const void *in, void *out, int32_t *sampDelay,
                std::string *err);
// engine_metrics.hip (arguments already checked by ssf_api.hip)
int metrics_run(int device, const ssf_metrics_params *p, const void *rx, const void *tx, const double *const_raw,
                const double *const_norm, const double *px, const float *evm_w32, ssf_metrics_result *out, std::string *err);
int metrics_pnorm(int device, int64_t count, int dtype, const void *x, void *y, std::string *err);
int metrics_power(int device, int64_t count, int64_t rows, int dtype, const void *x, double *out, std::string *err);
int metrics_demod(int device, int64_t count, int dtype, int M, const double *const_raw, const void *symb, int32_t *bits_out,
                  std::string *err);
// engine_theory.hip (arguments already checked by ssf_api.hip)
int theory_mi(int device, int M, int nS, const double *const_tab, const double *px, const double *sigma, double *mi_out, std::string *err);
int theory_calc_mi(int device, int64_t n, int dtype, int M, double sigma2, const double *const_tab, const double *px, const void *rx,
                   const void *tx, double *mi_out, std::string *err);
// engine_cpr.hip (arguments already checked by ssf_api.hip)
int cpr_run(int device, const ssf_cpr_params *p, const double *table, const void *x, void *sig_out, double *phase_out, double *fo_out,
            std::string *err);
int cpr_bps(int device, int64_t n, int nModes, int dtype, int Nh, int B, int M, const double *table, const void *x, double *phase_out,
            std::string *err);
int cpr_foe(int device, int64_t n, int nModes, int dtype, int P, double Fs, const void *x, void *sig_out, double *fo_out,
            std::string *err);
// engine_sync.hip (arguments already checked by ssf_api.hip)
int sync_run(int device, const ssf_sync_params *p, const void *rx, const void *tx, void *out, ssf_sync_result *res, std::string *err);
int sync_finddelay(int device, int64_t nx, int64_t ny, int x_dtype, int y_dtype, const void *x, const void *y, int64_t *delay_out,
                   std::string *err);
int sync_transform_time(int device, int64_t L, int nseq, int nslots, int nslots2, int reps, double *seconds_out, std::string *err);
// engine_eq.hip (arguments already checked by ssf_api.hip)
int eq_run(int device, const ssf_eq_params *p, const ssf_eq_stage *stages, const double *table, const double *radii, void *H_inout,
           const void *x, const void *ref, void *sig_out, double *errsq_out, std::string *err);
// engine_siso.hip (arguments already checked by ssf_api.hip)
int siso_run(int device, ssf_siso_params *p, const double *table, void *coef_inout, const void *x, const void *ref, void *sig_out,
             double *mse_out, std::string *err);
// engine_seqdet.hip (arguments already checked by ssf_api.hip)
int64_t mlse_survivor_bytes(int64_t n, int cols, int M, int taps);
int mlse_run(int device, ssf_mlse_params *p, const double *h, const double *const_tab, const void *y, void *out, double *final_metric,
             std::string *err);
int detector_run(int device, int64_t n, int dtype, int M, int rule, double sigma2, const double *const_tab, const double *logpx, const void *r,
                 void *decided, int64_t *ind, std::string *err);
int autocorr_run(int device, int64_t n, int nTaps, const void *x, double *r_out, std::string *err);
// engine_syncdata.hip (arguments already checked by ssf_api.hip)
int syncdata_tile(int device, const ssf_sync_tile_params *p, const void *rx, const void *tx, void *rx_out, void *tx_out, std::string *err);
int syncdata_real_part(int device, int64_t count, const void *x, void *out, std::string *err);
int syncdata_copy_columns(int device, int64_t n, int width, int src_cols, int src_first, int dst_cols, int dst_first, const void *src, void *dst,
                          std::string *err);
int syncdata_extract(int device, int64_t n, int modes, int64_t n_out, int out_dtype, int normalize, const void *x, void *out, int64_t *kept,
                     std::string *err);
int syncdata_moving_average(int device, int64_t n, int cols, int N, int dtype, const void *x, void *out, std::string *err);
int syncdata_bert(int device, int64_t n, const void *irx, const void *bits, double *scal_out, std::string *err);
// engine_fec.hip (arguments already checked by ssf_api.hip)
int fec_calc_llr(int device, int64_t n, int dtype, int M, double sigma2, const double *table, const int32_t *bitmap, const double *px,
                 const void *x, double *llr_out, std::string *err);
int fec_graph_create(int device, int m, int n, int E, const int32_t *co, const int32_t *ev, const int32_t *vo, const int32_t *ve,
                     int max_dc, ssf_ldpc_graph **out, std::string *err);
int fec_graph_destroy(ssf_ldpc_graph *g, std::string *err);
int fec_decode(int device, const ssf_ldpc_graph *g, const ssf_ldpc_params *p, const void *llr_in, void *llr_out, int8_t *bits_out,
               int8_t *fail_out, uint32_t *iter_out, std::string *err);

// engine_enc.hip (arguments already checked by ssf_api.hip)
int enc_create(int device, const ssf_ldpc_encoder_desc *d, const uint64_t *block1, const uint64_t *block2, const int32_t *indptr,
               const int32_t *indices, ssf_ldpc_encoder **out, std::string *err);
int enc_destroy(ssf_ldpc_encoder *e, std::string *err);
int enc_encode(int device, const ssf_ldpc_encoder *e, const ssf_ldpc_encode_params *p, const void *bits_in, void *cw_out, std::string *err);
int enc_modulate(int device, int64_t nsymb, int M, const double *table, const void *bits, void *symb_out, std::string *err);

// engine_ofdm.hip (arguments and tables already checked by ssf_api.hip)
int ofdm_modulate(int device, const ssf_ofdm_params *p, const int32_t *src_map, const void *symb, void *out, std::string *err);
int ofdm_demodulate(int device, const ssf_ofdm_params *p, const int32_t *bin_carrier, const int32_t *data_carriers,
                    const int32_t *pilot_carriers, const int32_t *pilot_hi, const void *sig, void *symb_out, void *H_out,
                    std::string *err);

// engine_nlin.hip (arguments and tables already checked by ssf_api.hip)
int nlin_run(int device, const ssf_nlin_params *p, const int32_t *pass, const double *coef, const int32_t *nidx, const int32_t *phase_m,
             const double *phase_c, const void *x, const void *y, void *out0, void *out1, void *out2, void *out3, std::string *err);

// engine_clock.hip (arguments already checked by ssf_api.hip)
int clock_interp(int device, const ssf_clock_params *p, const void *x, const double *t_re, const double *t_im, void *out,
                 std::string *err);
int clock_quantize(int device, int64_t count, int dtype, double qmin, double qdelta, int64_t levels, const void *x, double *out,
                   std::string *err);
int clock_clip(int device, int64_t count, int dtype, double lo, double hi, const void *x, void *out, std::string *err);
int clock_minmax(int device, int64_t count, int dtype, const void *x, double *out2, std::string *err);
int clock_scale_add(int device, int64_t count, double scale, int has_scale, const double *x, const double *noise, double *out,
                    std::string *err);
int clock_gardner(int device, const ssf_gardner_params *p, const void *x, void *sig_out, double *t_out, int64_t *last_n,
                  std::string *err);
int clock_drift(int device, int64_t n, int ncols, int per_column, const double *t, double *ppm_out, std::string *err);

// engine_array.hip (arguments already checked by ssf_api.hip)
int array_copy(int device, const ssf_array_desc *sdesc, const void *src, const ssf_array_desc *ddesc, void *dst, std::string *err);
int array_take(int device, int64_t n_src, int64_t n_idx, int64_t inner, int itemsize, int idx_itemsize, const void *idx, const void *src,
               void *dst, std::string *err);
int array_transpose(int device, int64_t rows, int64_t cols, int itemsize, const void *src, void *dst, std::string *err);
int array_fill(int device, int64_t count, int itemsize, const void *value, void *dst, std::string *err);
int array_binary(int device, const ssf_array_binary_params *p, const void *a, const void *b, void *out, std::string *err);
int array_unary(int device, int op, int in_dtype, int out_dtype, int64_t count, const void *x, void *out, std::string *err);
int array_reduce(int device, int op, int dtype, int64_t rows, int cols, const double *center, const void *x, double *out, int64_t *arg_out,
                 std::string *err);
int array_freq_shift(int device, int64_t n, int ncols, int dtype, double deltaF, double Fs, const void *x, void *out, std::string *err);

inline int fail(ssf_plan *p, int code, const std::string &msg) {
    if (p) p->err = msg;
    return code;
}

#define SSF_HIP(plan, call)                                                                  \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess)                                                               \
            return ssf::fail((plan), e__ == hipErrorOutOfMemory ? SSF_ERR_OOM : SSF_ERR_HIP, \
                             std::string(#call) + ": " + hipGetErrorString(e__));            \
    } while (0)

}  // namespace ssf
