/* ssf.h -- C ABI of the MI355X-native split-step Fourier fiber-propagation library
 * (libssf_hip.so).  POD types only, no C++ exceptions cross this boundary, every
 * entry point returns an ssf_status (0 = OK, negative = error) unless stated.
 *
 * What each entry point replaces in the reference (paths relative to the
 * OptiCommPy checkout; the reference has no FFI, its "plugin API" is the set of
 * Python functions a notebook imports from optic.models.modelsGPU):
 *
 *   ssf_device_count / ssf_device_info   optic/dsp/coreGPU.py:11-24   (checkGPU)
 *   ssf_plan_create / ssf_plan_destroy   implicit cupy allocations + cuFFT plan cache,
 *                                        optic/models/modelsGPU.py:404,450-451 (manakovSSF)
 *   ssf_upload                           cp.asarray(Ei).astype(prec)      modelsGPU.py:216,404
 *   ssf_execute  (model NLSE)            ssfm hot loop                    modelsGPU.py:241-269
 *                                        == optic/models/channels.py:215-238
 *   ssf_execute  (model MANAKOV, +1)     manakovSSF span/step/iteration loops
 *                                        modelsGPU.py:420-498 == channels.py:380-456
 *   ssf_execute  (model MANAKOV, -1)     manakovDBP                       modelsGPU.py:564-772
 *                                        == optic/dsp/equalization.py:1087-1160
 *   ssf_download                         cp.asnumpy(...)                  modelsGPU.py:271,501-509
 *   ssf_set_snapshot_sink / ssf_sync_snapshots   Ech_spans[:, 2*indRecSpan:...] = ...   channels.py:453-456
 *   ssf_run                              one whole reference call (upload+execute+download)
 *   ssf_mgpu_run                         (no reference equivalent) independent fields
 *                                        sharded over the GPUs of one node, SURVEY.md 8e
 *   ssf_plan_set_units                   (no reference equivalent) several independent fields per launch
 *   ssf_plan_set_lanes                   (no reference equivalent) this plan shares the GPU with others
 *   ssf_set_coupling[_comm]              np.max(phiRot) / scipy.linalg.norm over ALL rows of a K > 1 batch
 *                                        (channels.py:394, 517-519) when the rows live in several plans
 *   ssf_couple_reduce_selftest           (test aid) the rank-order reduction behind ssf_set_coupling_comm
 *   ssf_comm_*                           (no reference equivalent) one process per GPU: RCCL
 *                                        broadcast / scatter / gather of parameters, inputs and
 *                                        results of independent units, SURVEY.md 8e
 *   ssf_linear_channel                   linearFiberChannel               channels.py:30-109
 *   ssf_overlap_save                     blockwiseFFTConv as used by edc  optic/dsp/core.py:973-1046,
 *                                                                          optic/dsp/equalization.py:113-117
 *   ssf_nlin_phase_rot                   nlinPhaseRot                     channels.py:471-493
 *   ssf_convergence_condition            convergenceCondition             channels.py:496-519
 *   ssf_fir_filter / ssf_fir_long / ssf_delay_signal / ssf_decimate / ssf_rx_run   receiver side, see below
 *   ssf_device_malloc / ssf_device_free / ssf_device_memcpy / ssf_device_axpy   device-resident arrays, see below
 *   ssf_wdm_tx                           simpleWDMTx signal path          optic/models/tx.py:178-217
 *   ssf_pam_tx                           pamTransmitter signal path       optic/models/tx.py:317-342
 *   ssf_modulate_optical                 pm, mzm, iqm                     optic/models/devices.py:56-220
 *   ssf_awgn                             awgn                             optic/models/channels.py:522-565
 *   ssf_upsample                         upsample, voa                    optic/dsp/core.py:395-432, devices.py:263-286
 *   ssf_mlse                             mlse                             optic/comm/modulation.py:582-680
 *   ssf_detector                         detector                         optic/comm/modulation.py:412-481
 *   ssf_autocorr                         autocorr                         optic/dsp/core.py:1194-1227
 *   ssf_sync_tile / ssf_sync_extract / ssf_real_part / ssf_copy_columns   the glue of syncDataSequences   optic/dsp/synchronization.py:30-170
 *   ssf_moving_average                   movingAverage                    optic/dsp/core.py:829-880
 *   ssf_bert                             bert                             optic/comm/metrics.py:37-105
 *   ssf_device_copy_bandwidth            (no reference equivalent) measured memory ceiling
 *   ssf_set_profiling / ssf_get_kernel_times   time.time() pairs around calls in
 *                                        examples/benchmarck_GPU_processing.ipynb:389-395
 *
 * Data layout at the boundary: struct-of-arrays.  A "row" is one column of the
 * reference's (N, ncols) field, stored contiguously: rows = [x0, y0, x1, y1, ...]
 * for the Manakov model (nrows = 2K), or independent scalar fields for NLSE.
 * Complex samples are interleaved (re, im) float (SSF_C64) or double (SSF_C128).
 *
 * Ownership: the caller owns every host buffer it passes, for the duration of
 * the call only.  The library owns all device memory, FFT plans and its HIP
 * stream inside the opaque plan handle.  A plan is NOT thread-safe: use one
 * plan per (thread, device).  All calls are synchronous at return.
 */
#ifndef SSF_H
#define SSF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ssf_plan ssf_plan;

typedef enum {
    SSF_OK = 0,
    SSF_ERR_BAD_ARG = -1,
    SSF_ERR_HIP = -2,
    SSF_ERR_OOM = -3,
    SSF_ERR_FFT = -4,
    SSF_ERR_NO_DEVICE = -5,
    SSF_ERR_UNSUPPORTED = -6,
    SSF_ERR_STATE = -7,
    SSF_ERR_COMM = -8          /* RCCL: library missing or a collective failed                */
} ssf_status;

enum { SSF_C64 = 0, SSF_C128 = 1 };                       /* field precision            */
enum { SSF_MODEL_NLSE = 0, SSF_MODEL_MANAKOV = 1 };       /* ssfm | manakovSSF/DBP      */
enum { SSF_AMP_NONE = 0, SSF_AMP_IDEAL = 1, SSF_AMP_EDFA = 2 };
enum { SSF_ENGINE_AUTO = 0, SSF_ENGINE_ROCFFT = 1, SSF_ENGINE_FUSED = 2 };

/* Raw physical parameters exactly as the reference's parameters object holds them
 * (channels.py:305-322); every derived constant (alpha [1/km], beta2, lambda,
 * G_lin, nsp, p_noise) is computed inside the library with scipy's literals
 * c = 299792458.0, h = 6.62607015e-34. */
typedef struct {
    int32_t model;            /* SSF_MODEL_*                                             */
    int32_t direction;        /* +1 forward (ssfm, manakovSSF); -1 back-propagation      */
    double  Fs;               /* sampling rate [Hz]                                      */
    double  Fc;               /* carrier [Hz]                                            */
    double  alpha;            /* [dB/km]                                                 */
    double  D;                /* [ps/nm/km]                                              */
    double  gamma;            /* [1/W/km]                                                */
    double  Lspan;            /* [km]                                                    */
    int32_t Nspans;           /* floor(Ltotal/Lspan)                                     */
    int32_t maxIter;          /* Manakov: max fixed-point iterations per step            */
    double  hz;               /* [km] fixed step (also the cap-less nominal step)        */
    double  tol;              /* Manakov: convergence tolerance                          */
    int32_t nlprMethod;       /* Manakov: 1 = adaptive step from max nonlinear phase     */
    int32_t amp;              /* SSF_AMP_*                                               */
    double  maxNlinPhaseRot;  /* [rad]                                                   */
    double  NF;               /* EDFA noise figure [dB]                                  */
    int32_t n_save;           /* number of entries of save_spans (0 = final field only)  */
    int32_t rng_row_offset;   /* device ASE noise: row r of this plan draws stream row      */
                              /* rng_row_offset + r (ranks holding parts of one coupled     */
                              /* batch, Monte-Carlo units sharing a seed: distinct offsets  */
                              /* give independent noise); 0 for a stand-alone call          */
    const int32_t *save_spans;/* 1-based span indexes to snapshot (reference saveSpanN)  */
    int64_t rng_seed;         /* amp == EDFA and no host noise given: != 0 -> ASE noise is */
                              /* generated on the device (Philox4x32-10 keyed by rng_seed, */
                              /* counter = sample / rng_row_offset + row / span); 0 -> gain */
                              /* only                                                       */
} ssf_params;

typedef struct {
    int64_t steps;               /* passes of `while z_current < Lspan` / inner `for`    */
    int64_t iterations;          /* Manakov fixed-point iterations, summed               */
    int64_t transforms;          /* length-N FFT/IFFTs of one row, summed                */
    int64_t nonconverged_steps;  /* steps that hit maxIter (reference logs a warning)    */
    double  device_ms;           /* HIP-event time of the propagation on the plan stream */
    double  bytes_algorithmic;   /* transforms * 2 * sizeof(complex) * N      */
    int32_t engine;              /* SSF_ENGINE_* actually used                           */
    int32_t n_snapshots;         /* snapshots captured so far                            */
    int64_t decided_ahead;       /* fused engine: iterations whose convergence test was  */
                                 /*   evaluated one iteration in advance (all but the    */
                                 /*   first of every step)                               */
    int64_t rebuilt_iterates;    /* fused engine: iterates rebuilt as final (lim_0<tol)  */
    int64_t recovered_fields;    /* fused engine: step-start fields recovered from E_hd  */
                                 /*   for an exact lim_0 (three launches each)           */
} ssf_stats;

/* Optional per-step trace (for parity checks of the data-dependent control flow).
 * Arrays are caller-owned; the library writes at most `capacity` steps. */
typedef struct {
    int64_t  capacity;        /* in: number of steps the arrays can hold                 */
    int64_t  count;           /* out: steps written                                      */
    double  *hz;              /* [capacity]            step size of each step            */
    int32_t *iters;           /* [capacity]            iterations of each step           */
    double  *lims;            /* [capacity * maxIter]  convergence values (NaN = unused) */
} ssf_trace;

typedef struct {
    char     name[128];
    char     arch[32];           /* e.g. "gfx950"                                        */
    int32_t  compute_units;
    int32_t  reserved;
    int64_t  total_mem_bytes;
    int64_t  lds_per_block_bytes;
} ssf_device_info_t;

/* ---- discovery --------------------------------------------------------------------- */
int  ssf_device_count(void);                                /* >= 0, or negative status */
int  ssf_device_info(int device, ssf_device_info_t *out);
const char *ssf_version(void);

/* ---- plan life cycle ---------------------------------------------------------------- */
/* N samples per row, nrows rows (2K for Manakov), precision SSF_C64/SSF_C128,
 * engine SSF_ENGINE_AUTO picks the fused radix-2^n pipeline when N is a supported
 * power of two and the rocFFT pipeline otherwise. */
int  ssf_plan_create(int device, int64_t N, int32_t nrows, int32_t precision,
                     int32_t engine, ssf_plan **out);
int  ssf_plan_destroy(ssf_plan *plan);
const char *ssf_last_error(const ssf_plan *plan);           /* never NULL; plan may be NULL */

/* ---- staged execution (field stays resident in HBM between calls) ------------------- */
int  ssf_upload(ssf_plan *plan, const void *field_soa);     /* (nrows, N) complex        */
/* Propagate spans [span_first, span_last] (1-based, inclusive) of `params`.
 * noise: NULL, or host array (span_last-span_first+1, nrows, N) complex added after
 *        the span gain when amp == SSF_AMP_EDFA (row r of span s at
 *        ((s-span_first)*nrows + r)*N); NULL with EDFA = device-generated noise when
 *        params->rng_seed != 0, gain only otherwise.
 * stats/trace may be NULL; stats accumulate until ssf_upload resets them. */
int  ssf_execute(ssf_plan *plan, const ssf_params *params, int32_t span_first,
                 int32_t span_last, const void *noise, ssf_stats *stats, ssf_trace *trace);
int  ssf_download(ssf_plan *plan, void *field_soa);         /* (nrows, N) complex        */
int  ssf_download_snapshots(ssf_plan *plan, void *snap_soa);/* (n_snapshots, nrows, N)   */
/* Streamed snapshots.  With a sink set, the snapshots of the following ssf_execute calls are
 * not kept in device memory: capture number i (i = first_index, first_index + 1, ... in capture order) of the
 * (nrows, N) field is written to columns [i * nrows, (i + 1) * nrows) of the row-major (N, ld) complex array at
 * `dst` -- the reference's Ech_spans[:, 2 * indRecSpan : 2 * indRecSpan + 2] (optic/models/channels.py:453-456,
 * modelsGPU.py:497-498).  dst on the device: written in place by the conversion kernel.  dst on the host: moved by
 * a copy thread on its own stream while the next span propagates; ssf_sync_snapshots returns when every captured
 * snapshot has arrived (ssf_execute does not wait for them).  dst = NULL detaches the sink (and waits). */
int  ssf_set_snapshot_sink(ssf_plan *plan, void *dst, int64_t ld, int32_t first_index);
int  ssf_sync_snapshots(ssf_plan *plan);
/* Same transfers in the reference's own array layout: (N, nrows) row-major, i.e. the C-contiguous
 * numpy field with columns [x0, y0, x1, y1, ...]; the AoS <-> SoA conversion runs on the device
 * (Ei_[:, 0::2].T / Ech[:, 0::2] = Ech_x.T in the reference, modelsGPU.py:406-407, 506-509).
 * which = -1: the current field; which >= 0: snapshot number `which`. */
int  ssf_upload_aos(ssf_plan *plan, const void *field_aos);
int  ssf_download_aos(ssf_plan *plan, int32_t which, void *field_aos);

/* ---- one-shot: upload + execute all spans + download -------------------------------- */
int  ssf_run(ssf_plan *plan, const ssf_params *params, const void *field_in_soa,
             void *field_out_soa, void *snapshots_soa, const void *noise,
             ssf_stats *stats, ssf_trace *trace);

/* ---- multi-GPU: independent units sharded over devices (one host thread per device) -- */
/* n_units fields of (rows_per_unit, N) each, contiguous in in/out; unit u runs on
 * device dev_ids[u * n_dev / n_units ...] (contiguous blocks).  stats: [n_units]. */
int  ssf_mgpu_run(int32_t n_dev, const int32_t *dev_ids, int32_t n_units, int64_t N,
                  int32_t rows_per_unit, int32_t precision, int32_t engine,
                  const ssf_params *params, const void *fields_in, void *fields_out,
                  ssf_stats *stats);

/* ---- multi-GPU, one process per GPU: RCCL over xGMI ------------------------------------------
 * The same partitioning as ssf_mgpu_run (unit u of U belongs to rank u*G/U ... contiguous blocks), for launchers that
 * start one process per GPU (torchrun, mpirun, srun).  Only inputs and results of INDEPENDENT units and the
 * parameter block cross the links; there is no per-step communication.  librccl.so is opened with
 * dlopen by the first ssf_comm_get_id / ssf_comm_create call; without it these calls return SSF_ERR_COMM and
 * everything else keeps working.  Every buffer may be a host pointer (staged through device memory inside the
 * library) or a device pointer of ssf_device_malloc.  All calls are collective where RCCL's are, blocking at return.
 *   ssf_comm_get_id     rank 0 draws the 128-byte rendezvous id (ncclGetUniqueId) and hands it to the other
 *                       ranks by any out-of-band means (opticommpy_amd.mgpu: a file next to the launcher's port)
 *   ssf_comm_create     ncclCommInitRank on `device`
 *   ssf_comm_bcast      parameter block / launch powers                      (ncclBroadcast, in place)
 *   ssf_comm_send/recv  inputs from the root to the owner of a unit, results back   (ncclSend / ncclRecv)
 *   ssf_comm_allgather  results of every rank's block to every rank          (ncclAllGather)
 *   ssf_comm_allreduce  op 0 = sum, 1 = max, in place: timings and checksums (ncclAllReduce)
 *   ssf_comm_barrier    an 8-byte all-reduce */
typedef struct ssf_comm ssf_comm;
#define SSF_COMM_ID_BYTES 128
int  ssf_comm_get_id(void *id);
int  ssf_comm_create(int device, int32_t nranks, int32_t rank, const void *id, ssf_comm **out);
int  ssf_comm_destroy(ssf_comm *comm);
int  ssf_comm_rank(const ssf_comm *comm);
int  ssf_comm_size(const ssf_comm *comm);
int  ssf_comm_barrier(ssf_comm *comm);
int  ssf_comm_allreduce(ssf_comm *comm, double *values, int32_t n, int32_t op);
int  ssf_comm_bcast(ssf_comm *comm, void *buf, int64_t bytes, int32_t root);
int  ssf_comm_send(ssf_comm *comm, const void *buf, int64_t bytes, int32_t peer);
int  ssf_comm_recv(ssf_comm *comm, void *buf, int64_t bytes, int32_t peer);
int  ssf_comm_allgather(ssf_comm *comm, const void *send, void *recv, int64_t bytes_per_rank);
const char *ssf_comm_last_error(const ssf_comm *comm);       /* never NULL; comm may be NULL */

/* ---- coupled batch across plans (the caveat row) ------------------------------------------------
 * A (N, 2K) batch passed to ONE reference call is coupled: the adaptive step uses max(phi) over ALL rows
 * (optic/models/channels.py:394) and convergenceCondition the Frobenius norms over ALL rows (channels.py:517-519).  To
 * reproduce that call with the pairs spread over several plans (GPUs, processes), give each plan a reducer: the
 * general-length engine (host-driven control flow: plans created with SSF_ENGINE_ROCFFT) hands it the partial results it
 * is about to use -- op 0: values[0..n) are sums (sum |E_fd - E_conv|^2, sum |E_conv|^2), op 1: maxima (max phi) -- and
 * continues with what the reducer leaves in `values`: with an all-reduce over the participating plans every plan takes
 * the step sizes and iteration counts of the single coupled call.  reduce = NULL detaches.  Returns SSF_ERR_UNSUPPORTED
 * on the fused engine (its control flow lives on the device; independent units need no coupling). */
typedef int (*ssf_reduce_fn)(void *ctx, double *values, int32_t n, int32_t op);
int  ssf_set_coupling(ssf_plan *plan, ssf_reduce_fn reduce, void *ctx);
/* The same coupling for the device-resident pipeline (SSF_PIPE_DEVICE: natively split lengths on the fused engine), host out
 * of the loop: between the column launch that leaves the partial sums / maxima and the row launch that uses them the plan's stream
 * carries one ncclAllGather of 40 bytes over `comm` and every rank reduces the gathered values in rank order (identical bits, hence
 * identical step sizes and iteration counts, on every rank).  Every rank of `comm` must run the same call with its own pairs.
 * comm = NULL detaches.  SSF_ERR_UNSUPPORTED on the host-driven pipelines (use ssf_set_coupling there) and for plans of
 * independent units; SSF_ERR_BAD_ARG if the communicator lives on another device. */
int  ssf_set_coupling_comm(ssf_plan *plan, ssf_comm *comm);

/* ---- which pipeline a plan runs on (ssf_stats.engine says SSF_ENGINE_FUSED for everything on the hand-written kernels) ----
 *   SSF_PIPE_DEVICE     natively split length: device-resident control flow, no host synchronisation inside a span
 *   SSF_PIPE_ROWS       short 2^a 3^b 5^c length: host-driven step loop, FFT . H . IFFT of a row in one LDS launch
 *   SSF_PIPE_BLUESTEIN  any other length: host-driven step loop, every transform a Bluestein convolution on the fused kernels
 *   SSF_PIPE_ROCFFT     host-driven step loop on rocFFT transforms (the cross-check engine)
 * The host-driven ones read 16 bytes back per iteration: a bench or roofline record should not file them under the
 * device-resident pipeline.  Returns the code (>= 0) or a negative status. */
enum { SSF_PIPE_DEVICE = 0, SSF_PIPE_ROWS = 1, SSF_PIPE_BLUESTEIN = 2, SSF_PIPE_ROCFFT = 3 };
int  ssf_plan_pipeline(const ssf_plan *plan);

/* ---- independent units in one plan (no reference equivalent: the reference runs one field per call) ----------------
 * Small fields are latency-bound one at a time: a launch is one chain of load -> transform -> store of ~10 us whatever its
 * size.  ssf_plan_set_units(plan, n) declares the plan's rows to be n independent fields ("units") of nrows / n rows each,
 * rows [u * nrows / n, (u + 1) * nrows / n) = unit u (an even number of rows per unit for the Manakov models).  Every
 * launch of ssf_execute then carries all units (grid.y = n), and every unit keeps its OWN device-resident control block,
 * partial sums, step sizes and convergence decisions: the result is bit-equal to n separate plans, unlike one coupled
 * K > 1 call (which shares max(phi) and the norms over all rows, channels.py:394, 517-519).  ssf_stats counts are sums
 * over the units; traces are not recorded (SSF_ERR_BAD_ARG with a trace).  Device noise: row r draws stream row
 * rng_row_offset + r, i.e. unit u sees what a stand-alone call with rng_row_offset + u * nrows / n would.  Call it before
 * ssf_upload (the engine is rebuilt, an uploaded field is dropped).  Natively split lengths of the fused engine only
 * (SSF_ERR_UNSUPPORTED otherwise: the caller falls back to one call per unit). */
int  ssf_plan_set_units(ssf_plan *plan, int32_t n_units);
/* steps / iterations / transforms / nonconverged_steps / decided_ahead / rebuilt_iterates / recovered_fields of ONE unit since the last upload
 * (the Manakov models; the other fields of *out are those of the plan). */
int  ssf_get_unit_stats(ssf_plan *plan, int32_t unit, ssf_stats *out);

/* ---- lanes: several plans sharing one GPU concurrently (no reference equivalent) ------------------------------------
 * ssf_mgpu_run / mgpu.run_sharded / bench.py --config 4 | 5 keep two plans (own stream, own host thread) busy per GPU so that one
 * unit's launches fill the other's load / store phases.  A hint that this plan is one of n_lanes such plans: the kernels
 * then leave the issue priorities alone (with one field on the GPU, priority by phase is worth +3 %; with two fields
 * interleaving it costs 4 %: profiles/r3_lanes_prio_wt.txt).  Default 1; may be called at any time between executes. */
int  ssf_plan_set_lanes(ssf_plan *plan, int32_t n_lanes);

/* ---- the device-side reduction of a coupled batch by itself (test aid) ------------------------
 * ssf_set_coupling_comm reduces every rank's per-workgroup partials on the device, all-gathers five doubles per rank and reduces
 * those in rank order, so that every rank takes identical decisions (channels.py:394, 517-519 evaluated over ALL rows).  This
 * entry runs exactly that arithmetic on synthetic partials, without a communicator: `parts` = [nranks][5][npart] doubles, per rank
 * the arrays (max phi, sum lim_i numerator, denominator, lim_0 numerator, denominator) of npart workgroups; out5 = (sum num0, sum
 * den0, sum num, sum den, max) as the row stage of every rank would read them. */
int  ssf_couple_reduce_selftest(int device, int32_t nranks, int32_t npart, const double *parts, double *out5);

/* ---- per-kernel timing (measurement aid; fused engine only) ------------------------------ */
/* With profiling enabled every kernel launch of ssf_execute is bracketed by HIP events on the
 * plan's stream (costs a few microseconds per launch: do not enable for the headline timing).
 * Totals accumulate until ssf_upload.  Kernel classes of the fused pipeline:
 *   row   = (convergence decision,) FFT_rows . H . IFFT_rows   (one transform-equivalent per row)
 *   col   = Manakov column stage: inverse/forward column FFTs around the time-domain work
 *   other = scalar-NLSE / linear-channel column stages
 * The Manakov column stage runs as stage-specialised kernels where the field fills the chip (H: half-dispersed field out + first
 * rotation; ADV: a non-final iterate -> the next one; FIN: the final iterate, observed and stored; launches whose stage the state
 * did not ask for do nothing and are counted where they were enqueued); col_* are included in col_ms / col_n, which also hold
 * the general kernel's launches (span start, short fields, ragged tiles).                    */
typedef struct {
    double  row_ms, col_ms, other_ms;
    int64_t row_n, col_n, other_n;
    double  col_h_ms, col_adv_ms, col_fin_ms;
    int64_t col_h_n, col_adv_n, col_fin_n;
    int64_t outliers;       /* launches whose events were more than 8 x the median of their class apart (the stream was held up: a clock
                               transition, the profiler, another process): counted here, left out of the sums above */
} ssf_kernel_times;
int  ssf_set_profiling(ssf_plan *plan, int32_t enable);
int  ssf_get_kernel_times(ssf_plan *plan, ssf_kernel_times *out);

/* ---- measured memory ceiling ("also report against an empirically measured
 * device-copy bandwidth from the same run").  Launches a kernel with the memory shape of the
 * fused row stage and no arithmetic: every 256-thread workgroup fetches 16 x 16 B per thread
 * in one burst and stores them again, `bytes` in and `bytes` out per launch, ping-ponging between
 * two buffers.  *gbs = (read + written bytes) / average launch time.  No reference equivalent. */
int  ssf_device_copy_bandwidth(int device, int64_t bytes, int32_t launches, double *gbs);

/* ---- linear channel (gamma = 0 closed form): one FFT . H . IFFT over the whole length.  field_in_soa == NULL: the field the plan
 * already holds (ssf_upload / ssf_upload_aos -- the reference's own (N, ncols) layout, host or device pointer); field_out_soa ==
 * NULL: the result stays in the plan (ssf_download / ssf_download_aos).  Reference: optic/models/channels.py:30-109. */
int  ssf_linear_channel(ssf_plan *plan, double Fs, double Fc, double alpha, double D,
                        double L, const void *field_in_soa, void *field_out_soa);

/* ---- overlap-save FFT convolution: the engine of edc -------------------------------------- */
/* Replaces blockwiseFFTConv(x, h, NFFT, freqDomainFilter=True) as edc calls it, once per mode
 * (optic/dsp/equalization.py:113-117, optic/dsp/core.py:973-1046), for all modes at once.
 * sig_in / sig_out: (sigLen, nrows) row-major complex (the reference's sigIn layout).
 * Hfft: nfft complex values = fft(zero-padded impulse response) (core.py:1020); nfft = 2^m,
 * 16 <= nfft <= 8192 (SSF_C128) / 16384 (SSF_C64), K = filter length <= nfft. */
int  ssf_overlap_save(int device, int64_t sigLen, int32_t nrows, int32_t precision, int32_t nfft,
                      int32_t K, const void *Hfft, const void *sig_in, void *sig_out);

/* ---- device-resident arrays: chaining calls without crossing PCIe -----------------------------
 * The reference's cupy twin converts to numpy at every function boundary (cp.asnumpy,
 * optic/models/modelsGPU.py:271, 501-509; optic/dsp/coreGPU.py:72), so a channel -> receiver -> DBP
 * chain crosses the bus five times.  Here every `const void *` / `void *` array argument of this ABI
 * (fields, signals, LO, noise, snapshots; NOT the small filter / parameter arrays: Hfft, taps,
 * save_spans, trace) may also be a device pointer obtained from ssf_device_malloc on the same
 * device: the library recognises it (hipPointerGetAttributes) and copies device to device.
 * Layouts and sizes are unchanged.  ssf_device_memcpy copies between any two host / device
 * buffers and is synchronous at return. */
int  ssf_device_malloc(int device, int64_t bytes, void **ptr);
int  ssf_device_free(int device, void *ptr);
int  ssf_device_memcpy(int device, void *dst, const void *src, int64_t bytes);
/* y += alpha * x on n float64 values, host or device pointers (a device y is updated in place): balancedPD's i1 - i2
 * (optic/models/devices.py:456-458) when the two photocurrents are device arrays */
int  ssf_device_axpy(int device, int64_t n, double alpha, const double *x, double *y);

/* ---- receiver side of the channel: FIR filtering, fractional delay,
 * decimation and the coherent front-end.  All arrays are host buffers, complex128 interleaved,
 * (samples, columns) row-major exactly as the reference passes them; every call uploads its
 * inputs once, keeps all intermediate stages in device memory and downloads the result.
 *
 *   ssf_fir_filter       firFilter            optic/dsp/core.py:87-125 (GPU twin optic/dsp/coreGPU.py:27-78)
 *   ssf_delay_signal     delaySignal          optic/dsp/core.py:880-922
 *   ssf_decimate         decimate             optic/dsp/core.py:435-491
 *   ssf_rx_run           photodiode / balancedPD / coherentReceiver / pdmCoherentReceiver / iqMixing
 *                                             optic/models/devices.py:289-668, optic/dsp/core.py:925-970 */

/* 'same'-mode convolution of every column with `ntaps` complex taps (1 <= ntaps <= 4096) */
int  ssf_fir_filter(int device, int64_t sigLen, int32_t ncols, int32_t ntaps, const void *taps,
                    const void *sig_in, void *sig_out);
/* FIR of ANY length, evaluated on the device: sig_out[n, m] = sum_t taps[t] * sig_in[n + shift - t, m] for n in [0, outLen),
 * sig_in (inLen samples per column) extended with zeros on both sides; `shift` of either sign.  What it replaces:
 * blockwiseFFTConv's result (optic/dsp/core.py:973-1046; shift = (ntaps - 1) / 2, outLen = inLen) for filters of more than
 * 4096 taps -- edc over long links (optic/dsp/equalization.py:85-117), delaySignal with NFFT != 1024 (core.py:880-922: its
 * zero padding, np.roll(-1) and [:N] cut are shift + 1 and outLen = N), firFilter with long responses.  The impulse response is
 * cut into segments of 4096 taps, one overlap-save launch each, added in place: ceil(ntaps / 4096) passes over the signal.
 * Host or device pointers; a device signal never leaves the device. */
int  ssf_fir_long(int device, int64_t inLen, int64_t outLen, int32_t ncols, int64_t ntaps, const void *taps, int64_t shift,
                  const void *sig_in, void *sig_out);
/* one column delayed by `delay` seconds (NFFT = 1024 as the reference's default) */
int  ssf_delay_signal(int device, int64_t N, double delay, double Fs, const void *sig_in, void *sig_out);
/* The two helpers of the Manakov step the reference exports on their own (inside ssf_execute they are fused into
 * the column kernel).  n = number of samples of each array, complex128 interleaved, host or device pointers.
 *   ssf_nlin_phase_rot         nlinPhaseRot          optic/models/channels.py:471-493 (modelsGPU.py:514-535)
 *       phi[i] = (8/9) gamma (Pch[i] + |Ex[i]|^2 + |Ey[i]|^2) / 2     (Pch: the real part, n doubles)
 *   ssf_convergence_condition  convergenceCondition  optic/models/channels.py:496-519 (modelsGPU.py:538-561)
 *       *lim = sqrt(|Ex_fd - Ex_conv|^2 + |Ey_fd - Ey_conv|^2) / sqrt(|Ex_conv|^2 + |Ey_conv|^2)  (Frobenius norms) */
int  ssf_nlin_phase_rot(int device, int64_t n, double gamma, const void *Ex, const void *Ey, const double *Pch,
                        double *phi);
int  ssf_convergence_condition(int device, int64_t n, const void *Ex_fd, const void *Ey_fd, const void *Ex_conv,
                               const void *Ey_conv, double *lim);
/* maximum-variance sampling phase per column, then every decFactor-th sample; N % SpSin == 0,
 * ncols <= 8; sig_out: (ceil(N / decFactor), ncols); sampDelay (may be NULL): ncols phases */
int  ssf_decimate(int device, int64_t N, int32_t ncols, int32_t SpSin, int32_t decFactor,
                  const void *sig_in, void *sig_out, int32_t *sampDelay);

/* ---- the amplifier and the passive optics by themselves: element-wise device passes, complex128, host or device pointers (a
 * device array never leaves the device; an in-place ssf_edfa -- field_out == field_in -- is allowed).
 *   ssf_edfa                edfa              optic/models/devices.py:671-726 (GPU twin optic/models/modelsGPU.py:56-114)
 *       field_out = field_in * sqrt(G_lin) + noise over `n` complex values laid out (samples, ncols) row-major.  noise != NULL:
 *       the caller's n complex values (the reference's seeded np.random draws, draw for draw); noise == NULL and rng_seed != 0:
 *       CN(0, p_noise) from Philox4x32-10 (counter = sample, rng_row_offset + column), statistical parity like the span epilogue
 *       of ssf_execute; both absent: gain only.  G_lin / p_noise as the reference derives them (devices.py:712-722).
 *   ssf_pbs                 pbs               optic/models/devices.py:223-260
 *       (Ex, Ey) = [ex, ey] @ [[cos t, -sin t], [sin t, cos t]] for a field of shape (N, 2), or (N,) taken as [ex, 0]
 *   ssf_optical_hybrid_2x4  opticalHybrid2x4  optic/models/devices.py:462-500
 *       Eo (4, N) = T @ [Es, 0, 0, Elo] with the 90-degree hybrid's transfer matrix T */
int  ssf_edfa(int device, int64_t n, int32_t ncols, double G_lin, double p_noise, int64_t rng_seed, int32_t rng_row_offset,
              const void *field_in, const void *noise, void *field_out);
int  ssf_pbs(int device, int64_t N, int32_t ncols, double theta, const void *E, void *Ex, void *Ey);
int  ssf_optical_hybrid_2x4(int device, int64_t N, const void *Es, const void *Elo, void *Eo);

typedef struct {
    double  Fs;
    /* pdmCoherentReceiver: paramFE.polRotation / pdl / polDelay (devices.py:649-662) */
    double  polRotation, pdl, polDelay;
    /* iqMixing per polarisation: index 0 = X or the only polarisation, 1 = Y (core.py:925-970) */
    double  ampImb[2], phaseImb[2], timeSkew[2];
    /* photodiode (devices.py:289-399); defaults are applied by the caller */
    double  R, Tc, Id, RL, B, IpdSat;
    int32_t N;                    /* filter taps (an even value is incremented, devices.py:361-365) */
    int32_t fType;                /* 0 'rect', 1 'gauss' */
    int32_t ideal, shotNoise, thermalNoise, currentSaturation, bandwidthLimitation;
    int32_t pad_;
    int64_t rng_seed;             /* device noise streams (Philox4x32-10; one counter row per pair of photodiodes, single-precision Box-Muller) */
    double  Fs_pd;                /* sampling rate of the photodiode model -- noise scale, low-pass design, the Fs >= 2 B check:
                                   * paramPD.Fs of the reference (devices.py:331-353, 562-563) -- when it differs from Fs
                                   * (paramFE.Fs: polarisation delay, IQ skew); 0 = Fs */
} ssf_rx_params;

enum ssf_rx_mode {
    SSF_RX_PHOTODIODE   = 0,      /* in0 (N, nmodes) field          -> out (N,) float64            */
    SSF_RX_BALANCED_PD  = 1,      /* in0 (N, 2) = [E1, E2]          -> out (N,) float64            */
    SSF_RX_COHERENT     = 2,      /* in0 (N,) signal, lo (N,)       -> out (N,) complex128         */
    SSF_RX_PDM_COHERENT = 3,      /* in0 (N, 2) signal, lo (N,)     -> out (N, 2) complex128       */
    SSF_RX_IQ_MIXING    = 4       /* in0 (N,) complex               -> out (N,) complex128         */
};
/* unit_normals: NULL = noise drawn on the device; otherwise [(pd * 2 + kind) * N + n] standard
 * normals, kind 0 = shot / 1 = thermal, pd = photodiode slot: photodiode 0; balanced pair 0, 1;
 * coherent receiver per polarisation p: 4p + {0: I+, 1: I-, 2: Q+, 3: Q-} (devices.py:562-563) */
int  ssf_rx_run(int device, int32_t mode, int64_t N, int32_t nmodes, const ssf_rx_params *params,
                const void *in0, const void *lo, const double *unit_normals, void *out);

/* ---- the receiver side of the coherent notebooks in ONE call: pdmCoherentReceiver -> firFilter (matched filter) -> decimate -> edc
 * (examples/test_WDM_transmission.ipynb cells 17 - 23; optic/models/devices.py:574-668, optic/dsp/core.py:87-125, 435-491,
 * optic/dsp/equalization.py:36-122), with the results of the four calls made one after the other.  What one call adds: the
 * stages' launches follow each other on the stream with one host wait at the end, decimate's variance search rides in the matched
 * filter's stores and its gather in the compensating filter's loads (no pass over the filtered signal of its own, the decimated
 * signal never materialised).
 *   Es (N, 2), Elo (N,) complex128, host or device;  taps: ntaps complex128 (<= 4096), host
 *   SpSin / decFactor as ssf_decimate (N % SpSin == 0)
 *   edc_Hfft: edc_nfft complex128 = fft(zero-padded impulse response) as ssf_overlap_save takes it, edc_K its taps, host
 *   sig_out ((N + decFactor - 1) / decFactor, 2) complex128, host or device;  sampDelay (may be NULL): the two sampling phases */
int  ssf_rx_chain(int device, int64_t N, const ssf_rx_params *params, const void *Es, const void *Elo, const void *taps,
                  int32_t ntaps, int32_t SpSin, int32_t decFactor, const void *edc_Hfft, int32_t edc_K, int32_t edc_nfft,
                  void *sig_out, int32_t *sampDelay);

/* ---- WDM transmitter: the signal path of simpleWDMTx, optic/models/tx.py:178-217.
 * For every channel and polarisation: zero-stuffing to SpS samples per symbol + pulse-shaping FIR
 * ('same' mode, one overlap-save launch), normalisation to unit peak, IQ modulator with the
 * reference's default bias and extinction (optic/models/devices.py:147-220), power normalisation to
 * amp^2, frequency shift to the channel's grid position, accumulation into the WDM field.  Symbol
 * sources, constellations, pulse taps and the LO phase-noise random walk are the caller's (they are
 * host-side numpy draws in the reference: optic/comm/sources.py:137-212, optic/dsp/core.py:792-826).
 *   symbols   (nChannels, nPolModes, nSymbols) complex128
 *   taps      ntaps float64 (<= 4096)
 *   phi       (nChannels, N) float64 LO phase per channel -- or (1, N), one walk shared by every channel, with params->phi_rows = 1
 *             (what a SEEDED reference run produces: tx.py:199 reseeds np.random with the same param.seed for every channel) --
 *             or NULL for an ideal laser; N = nSymbols * SpS
 *   amp       nChannels: sqrt(Pch / nPolModes);   deltaF: nChannels grid offsets [Hz]
 *   sig_out   (N, nPolModes) complex128 (host or device);  power_out (may be NULL): nChannels * nPolModes */
typedef struct {
    double  Fs, mzmScale;
    int64_t nSymbols;
    int32_t SpS, nChannels, nPolModes, ntaps;
    /* laser phase noise generated ON THE DEVICE (used when `phi` is NULL and pn_seed != 0): per channel a random walk
     * phi[0] = 0, phi[k] = phi[k - 1] + N(0, pn_sigma^2), pn_sigma = sqrt(2 pi linewidth / Fs) (optic/dsp/core.py:792-826), from
     * Philox4x32-10 keyed by pn_seed (statistical parity: what a call WITHOUT a seed can promise; with a seed the host passes the
     * reference's own np.random draws in `phi`).  No N-sample array crosses the bus then. */
    double   pn_sigma;
    uint64_t pn_seed;
    int32_t  phi_rows;   /* rows of `phi`: 0 or nChannels = one per channel; 1 = one row for all channels (uploaded once) */
    int32_t  reserved;
} ssf_tx_params;
int  ssf_wdm_tx(int device, const ssf_tx_params *params, const void *symbols, const double *taps, const double *phi,
                const double *amp, const double *deltaF, void *sig_out, double *power_out);

/* ---- IM/DD transmitter and AWGN channel.  Array arguments marked (host or device) may be device pointers; a device array never
 * leaves the device.  Every refusal is a status with a message (ssf_last_error(NULL)) before anything runs on the GPU.
 *   ssf_pam_tx            the signal path of pamTransmitter, optic/models/tx.py:317-342, for every polarisation mode: zero-stuffing +
 *       pulse-shaping FIR (one overlap-save launch), a peak pass, mzm(1, mzmScale * Vpi * sig / max|sig|, Vpi, Vb, ER) with the
 *       partial sums of its power, and sig_out[:, mode] = amp * pnorm(.): four launches per mode and one host wait at the end.
 *       symbols (nPolModes, nSymbols) float64 and taps (ntaps <= 4096) float64 on the host; Vb is the bias as calcMZM takes it
 *       (pamTransmitter passes -mzmVb); amp = sqrt(dBm2W(power)); sig_out (nSymbols * SpS, nPolModes) complex128 (host or device).
 *   ssf_modulate_optical  pm / mzm / iqm, optic/models/devices.py:56-220 (calcPM / calcMZM, optic/dsp/core.py:1076-1139), one
 *       element-wise launch.  kind: SSF_MOD_*; u: n values of u_dtype (SSF_M_F64 or SSF_M_C128; host or device) -- a
 *       complex drive is put through exp(1j * (z / Vpi) * pi) as written, iqm takes its real and imaginary parts; Ei: n complex128
 *       (host or device) or NULL for the scalar (Ei_re, Ei_im); pm reads Vpi; mzm reads Vpi, VbI, ERI; iqm reads all.  gamma is
 *       derived from the extinction ratios [dB] on the host in double precision, as calcMZM does.  out: n complex128.
 *   ssf_awgn              awgn, optic/models/channels.py:522-565, on n samples of ncols columns (row-major): sigma^2 = Fs_over_B *
 *       mean(|sig|^2 over every element) / snr_lin, out = sig + sqrt(sigma^2 / 2) * (zr + 1j zi); zi = 0 unless complex_noise.
 *       Two launches (fixed-order partial sums of the power; the noise pass adds them up itself) and no host wait in between.
 *       unit_normals != NULL (host or device): n * ncols float64 for zr, followed by as many for zi when complex_noise -- the
 *       caller's np.random.standard_normal draws; NULL and rng_seed != 0: Philox4x32-10 (counter = sample, row = column, a span
 *       tag of its own), statistical parity as in ssf_edfa.  in_dtype / out_dtype: SSF_M_F64 or SSF_M_C128; a
 *       float64 result needs a float64 signal and real noise.
 *   ssf_upsample          upsample, optic/dsp/core.py:395-432, and voa, optic/models/devices.py:263-286: out (rows * factor, w) =
 *       scale * in (rows, w) in the rows that are multiples of factor, zeros elsewhere, on rows of w 8-byte words (a float64 or
 *       complex64 column is one word, a complex128 column two).  scale == 1 copies the bits; any other scale multiplies float64
 *       values (float64 and complex128 arrays only). */
enum { SSF_MOD_PM = 0, SSF_MOD_MZM = 1, SSF_MOD_IQM = 2 };
int  ssf_pam_tx(int device, int64_t nSymbols, int32_t SpS, int32_t nPolModes, int32_t ntaps, const double *symbols,
                const double *taps, double mzmScale, double Vpi, double Vb, double ER, double amp, void *sig_out);
int  ssf_modulate_optical(int device, int32_t kind, int64_t n, int32_t u_dtype, const void *u, const void *Ei, double Ei_re,
                          double Ei_im, double Vpi, double VbI, double VbQ, double Vphi, double ERI, double ERQ, void *out);
int  ssf_awgn(int device, int64_t n, int32_t ncols, int32_t in_dtype, int32_t out_dtype, int32_t complex_noise, double Fs_over_B,
              double snr_lin, const void *sig_in, const void *unit_normals, int64_t rng_seed, void *sig_out);
int  ssf_upsample(int device, int64_t rows, int32_t w, int32_t factor, double scale, const void *in, void *out);

/* ---- link metrics: BER, SER, SNR, GMI, NGMI, MI and EVM of received against transmitted symbols, evaluated on the device
 * (optic/comm/metrics.py:111-195 fastBERcalc, 329-426 monteCarloGMI, 429-547 monteCarloMI, 572-637 calcEVM).  One call
 * normalises once and reads the symbols once per pass (statistics, decisions, soft demapping); `want` selects what is computed,
 * and a value is the same whatever else is asked for with it.  Sums are reduced in a fixed order: results repeat bit for bit.
 *   rx, tx      (n, nModes) row-major -- or (nModes, n) with transposed = 1 -- of `dtype`, host or device; never written
 *   const_raw   M (re, im) pairs: the Gray-ordered constellation as grayMapping stores it (single precision, widened)
 *   const_norm  M (re, im) pairs: const_raw / sqrt(Es) in double precision; with SSF_METRICS_EVM_BLIND the single-precision
 *               pnorm(table) the reference decides against
 *   px          M prior probabilities, NULL = uniform
 *   evm_w32     SSF_METRICS_EVM_BLIND only: float32 |c_m|^2 of that table (the reference averages it in float32)
 *   out         nModes results, host
 * Rows [discard, n - discard) are evaluated.  M is a power of two, 2 .. 1024; nModes <= 64.  SSF_METRICS_EVM_BLIND stands
 * alone and takes tx = NULL; every other selection needs tx. */
enum ssf_metrics_dtype { SSF_M_C128 = 0, SSF_M_C64 = 1, SSF_M_F64 = 2, SSF_M_F32 = 3 };
enum ssf_metrics_want {
    SSF_METRICS_BER = 1,          /* BER, SER, SNR and the error counts */
    SSF_METRICS_GMI = 2,          /* GMI, NGMI */
    SSF_METRICS_MI = 4,
    SSF_METRICS_EVM = 8,          /* data-aided */
    SSF_METRICS_EVM_BLIND = 16
};
typedef struct {
    int64_t n;                    /* symbols per mode */
    int64_t discard;
    int32_t nModes, M;
    int32_t dtype;                /* ssf_metrics_dtype of rx and tx */
    int32_t transposed;
    int32_t rotate;               /* 1 for 'qam' / 'psk': rx is rotated by mean(tx / rx) */
    int32_t want;
    double  Es;                   /* sum |const_raw|^2 px */
    double  H;                    /* source entropy, bits */
} ssf_metrics_params;
typedef struct {
    double  BER, SER, SNR, GMI, NGMI, MI, EVM;
    int64_t bit_errors, symbol_errors, n;
} ssf_metrics_result;
int  ssf_metrics(int device, const ssf_metrics_params *params, const void *rx, const void *tx, const double *const_raw,
                 const double *const_norm, const double *px, const float *evm_w32, ssf_metrics_result *out);
/* y = x / sqrt(mean |x|^2) over all `count` values (optic/dsp/core.py:701-717); y is complex128 for a complex dtype, float64
 * otherwise; x and y host or device */
int  ssf_pnorm(int device, int64_t count, int32_t dtype, const void *x, void *y);
/* out = sum |x|^2 / rows: the sum over the columns of their mean power (optic/dsp/core.py:69-85) */
int  ssf_signal_power(int device, int64_t count, int64_t rows, int32_t dtype, const void *x, double *out);
/* minimum-distance decisions of `count` symbols against const_raw, log2(M) bits each, most significant first
 * (optic/comm/modulation.py:369-408); bits_out: count * log2(M) int32, host or device */
int  ssf_demodulate(int device, int64_t count, int32_t dtype, int32_t M, const double *const_raw, const void *symb,
                    int32_t *bits_out);

/* ---- mutual information of a constellation on the circular AWGN channel (optic/comm/metrics.py:770-848 theoryMI, 497-547 calcMI).
 * ssf_theory_mi: by quadrature, for nS noise deviations in one call.
 *   const_tab   M (re, im) pairs, used as given;  px  M probabilities, finite and > 0;  sigma  nS deviations per dimension, > 0
 *   mi_out      nS values, host:  H(X) - sum_i px_i E[ log2( sum_j px_j e^{e_ij} ) - log2 px_i ],
 *               e_ij(t) = -(|d_ij|^2 + 2 sqrt(2) sigma Re(conj(d_ij) t)) / (2 sigma^2),  d_ij = x_i - x_j
 * The expectation over t (density e^{-|t|^2} / pi) is a uniform grid: spacing h = 0.1, |Re t|, |Im t| <= 6.5 (131 x 131 nodes),
 * weight e^{-|t|^2} h^2 / pi, not renormalised; the -log2 px_i term is multiplied by the grid's own weight sum, so a one-point table
 * gives exactly 0.  The rule is within 1e-10 of the integral (profiles/theory_quadrature.json).  Sums run in a fixed order: results
 * repeat bit for bit, and a value does not depend on which other deviations are asked for with it.  1 <= M <= 1024, 1 <= nS <= 4096.
 * ssf_calc_mi: the Monte-Carlo estimate over n symbol pairs, the reference's direct form in double.
 *   rx, tx      n values of `dtype` (ssf_metrics_dtype), host or device; never written
 *   mi_out      one value, host */
int  ssf_theory_mi(int device, int32_t M, int32_t nS, const double *const_tab, const double *px, const double *sigma, double *mi_out);
int  ssf_calc_mi(int device, int64_t n, int32_t dtype, int32_t M, double sigma2, const double *const_tab, const double *px,
                 const void *rx, const void *tx, double *mi_out);

/* ---- carrier phase recovery on the device: blind phase search with an optional 4th-power frequency offset estimation ahead of
 * it (optic/dsp/carrierRecovery.py:37-169 cpr, 172-223 bps, 333-371 fourthPowerFOE; optic/dsp/carrierRecoveryGPU.py bpsGPU).
 *   x           (n, nModes) row-major, complex128 (SSF_M_C128) or complex64 (SSF_M_C64), host or device; never written
 *   const_tab   M (re, im) pairs: the constellation the distances are taken to, as cpr normalises it (single precision, widened)
 *   sig_out     (n, nModes) complex128, host or device: pnorm(x e^{j phase}), the norm over all modes together
 *   phase_out   (n, nModes) float64, host or device, may be NULL (ssf_cpr): np.unwrap(4 phi, axis=0) / 4 of the raw test phases
 *   fo_out      nModes frequency offsets [Hz], host; may be NULL (ssf_cpr); written only with runFOE
 * For every mode, symbol k and test phase phi_b = b (pi/2) / B the search takes min_m |x_k e^{j phi_b} - c_m|^2, sums it over
 * symbols k - Nh .. k + Nh (symbols outside [0, n) enter as zeros, as the reference pads) and picks the first minimum over b.
 * The minimum distances stay in LDS; sums run in a fixed order, so results repeat bit for bit and do not depend on the tiling.
 * Limits: 2 <= M <= 1024, 1 <= B <= 1024, 0 <= Nh <= 1023, n >= 2, 1 <= nModes <= 64, 1 <= P <= 1024.  Arithmetic is double
 * whatever the input type (the reference rounds a complex64 signal back to single after the frequency offset compensation). */
typedef struct {
    int64_t n;                    /* symbols per mode */
    int32_t nModes, M;
    int32_t dtype;                /* SSF_M_C128 or SSF_M_C64 */
    int32_t B;                    /* test phases */
    int32_t Nh;                   /* half window: cpr passes N / 2 */
    int32_t runFOE;               /* 1: ssf_foe with (Fs, P) and the joint norm ahead of the search */
    int32_t P;                    /* power of the offset estimator: 4, or M for 'psk' */
    int32_t reserved;
    double  Fs;                   /* symbol rate 1 / Ts [Hz] */
} ssf_cpr_params;
int  ssf_cpr(int device, const ssf_cpr_params *params, const double *const_tab, const void *x, void *sig_out, double *phase_out,
             double *fo_out);
/* the raw test phase of every symbol: phase_out (n, nModes) float64, host or device */
int  ssf_bps(int device, int64_t n, int32_t nModes, int32_t dtype, int32_t Nh, int32_t B, int32_t M, const double *const_tab,
             const void *x, double *phase_out);
/* fourthPowerFOE: per mode fo = f[argmax |fft(x ** P)|] / P with f = fftshift(Fs fftfreq(n)), the first maximum in that order;
 * sig_out = x exp(-j 2 pi fo k / Fs), (n, nModes) complex128, host or device; fo_out: nModes, host */
int  ssf_foe(int device, int64_t n, int32_t nModes, int32_t dtype, int32_t P, double Fs, const void *x, void *sig_out,
             double *fo_out);

/* ---- sequence synchronisation on the device (optic/dsp/core.py:552-675 symbolSync, 678-698 finddelay), the stage between edc and
 * the equalizer: the transmitted symbols aligned to the received signal.
 *   rx          (n_rx, nModes) row-major, complex128 or complex64, host or device; never written.  With SpS > 1 it is first
 *               decimated to one sample per symbol as ssf_decimate does (n_rx % SpS == 0)
 *   tx          (n_tx, nModes) complex128 or complex64, host or device; never written
 *   out         (n_tx, nModes) of tx's type, host or device: column k is tx[:, swap[k]], times rot[k], conjugated if conj[k],
 *               rolled by -delay[k]
 *   result      host, may be NULL: the decisions as applied
 * SSF_SYNC_AMP correlates |tx_m| - mean with |rx_n| - mean for every pair, SSF_SYNC_REAL the complex tx_m with Re rx_n and then
 * tx[:, swap[k]] with Im rx_k; corrMatrix[m, n] is the largest magnitude, swap its column argmax (first maximum).  Correlations
 * are scipy's mode "full" through transforms of a power-of-two length >= n_tx + n_rx - 1; every argmax takes the lowest index.
 * All launches of a call follow each other without a host decision; only `result` is copied back.
 * Limits: 1 <= nModes <= 8, n_tx >= 2, n_rx / SpS >= 2, SpS >= 1, SpS * nModes <= 256. */
enum ssf_sync_mode { SSF_SYNC_AMP = 0, SSF_SYNC_REAL = 1 };
typedef struct {
    int64_t n_rx;                 /* rows of rx as passed */
    int64_t n_tx;
    int32_t nModes, SpS;
    int32_t mode;                 /* ssf_sync_mode */
    int32_t rx_dtype, tx_dtype;   /* SSF_M_C128 or SSF_M_C64 */
    int32_t reserved;
} ssf_sync_params;
typedef struct {
    int64_t delay[8];
    int32_t swap[8];
    int32_t rot[8];               /* 0: 1, 1: -1, 2: 1j, 3: -1j */
    int32_t conj[8];
    double  corrMatrix[64];       /* (nModes, nModes) row-major */
} ssf_sync_result;
int  ssf_symbol_sync(int device, const ssf_sync_params *params, const void *rx, const void *tx, void *out, ssf_sync_result *result);
/* finddelay: argmax |correlate(x, y)| - nx + 1 (y conjugated); x, y 1-D of any ssf_metrics_dtype, host or device; nx, ny >= 1 */
int  ssf_finddelay(int device, int64_t nx, int64_t ny, int32_t x_dtype, int32_t y_dtype, const void *x, const void *y,
                   int64_t *delay_out);
/* measurement aid (tools/bench_sync.py): the transforms of one ssf_symbol_sync call alone, on the engine's own buffers and plans --
 * nseq forward, nslots and then nslots2 inverse transforms of length L (a power of two) per round; seconds_out: device time per
 * round over `reps` rounds after one warm-up round */
int  ssf_sync_transform_time(int device, int64_t L, int32_t nseq, int32_t nslots, int32_t nslots2, int32_t reps, double *seconds_out);

/* ---- adaptive MIMO equalizer on the device (optic/dsp/equalization.py:125-351 mimoAdaptEqualizer, 354-516 coreAdaptEq and the
 * update rules nlmsUp, cmaUp, rdeUp, dardeUp, ddlmsUp), the stage between decimate / edc and cpr.
 *   x           (n, nModes) row-major, complex128 (SSF_M_C128) or complex64 (SSF_M_C64), host or device; never written.  The
 *               nTaps / 2 zeros the reference pads at both ends are not stored: the kernels supply them
 *   ref         (nref, nModes) of ref_dtype, host or device; NULL unless a stage is SSF_EQ_NLMS or SSF_EQ_DARDE; never written
 *   stages      nStages records, host: the stages are contiguous in one symbol index, stage 0 is repeated numIter times over
 *               its symbols (carrying H), symbols beyond the sum of the stage lengths stay zero
 *   const_tab   M (re, im) pairs, host: the decision constellation of SSF_EQ_DDLMS
 *   radii_tab   nRadii ascending radii, host: the decision radii of SSF_EQ_RDE
 *   H_inout     (nModes^2, nTaps) complex128, host or device, row k + N nModes filters input mode N into output mode k: the
 *               initial coefficients in, the final ones out
 *   sig_out     (total, nModes) complex128, host or device;  errsq_out (nModes, total) float64, host or device, may be NULL:
 *               |e|^2 of every symbol, 0 for a static stage and beyond the last stage
 * Symbol i reads the padded samples i SpS .. i SpS + nTaps - 1;  total = (n + 2 (nTaps / 2) - nTaps) / SpS + 1.
 * With y_k the output of mode k, x_N the window of input mode N and e the error:
 *   NLMS    e = ref_k - y_k,                        H += mu e conj(x_N) / ||x_N||^2
 *   DDLMS   e = c[argmin |y_k - c|] - y_k,          H += mu e conj(x_N)              (the first minimum)
 *   CMA     e = Rcma - |y_k|^2,                     H += mu e y_k conj(x_N)
 *   RDE     e = R[argmin |R - |y_k||]^2 - |y_k|^2,  the same update;   DARDE  e = |ref_k|^2 - |y_k|^2, the same update
 *   STATIC  outputs with H as the stage before left it, no update.
 * Row k + N nModes of H is driven by y_k alone: one wavefront per output mode walks the symbols with its nModes nTaps
 * coefficients in registers, no wave waits for another, sums run in a fixed order and results repeat bit for bit.
 * Limits: 1 <= nModes <= 4, 1 <= nTaps <= 64, 1 <= SpS <= 8, n >= nTaps, 2 <= M <= 1024, 1 <= nRadii <= 1024.  Arithmetic is
 * double whatever the input types. */
typedef enum { SSF_EQ_NLMS = 0, SSF_EQ_CMA = 1, SSF_EQ_RDE = 2, SSF_EQ_DARDE = 3, SSF_EQ_DDLMS = 4, SSF_EQ_STATIC = 5 } ssf_eq_alg;
typedef struct {
    int64_t L;                    /* output symbols of the stage, >= 1 */
    int32_t alg;                  /* ssf_eq_alg */
    int32_t reserved;
    double  mu;                   /* step size (the reference rounds it to single precision first) */
} ssf_eq_stage;
typedef struct {
    int64_t n;                    /* input samples per mode */
    int64_t total;                /* output symbols per mode (totalNumSymb) */
    int64_t nref;                 /* rows of ref */
    int32_t nModes, nTaps, SpS;
    int32_t dtype, ref_dtype;     /* SSF_M_C128 or SSF_M_C64 */
    int32_t nStages, numIter;
    int32_t M, nRadii;
    int32_t reserved;
    double  Rcma;                 /* mean |c|^4 / mean |c|^2 */
} ssf_eq_params;
int  ssf_mimo_eq(int device, const ssf_eq_params *params, const ssf_eq_stage *stages, const double *const_tab, const double *radii_tab,
                 void *H_inout, const void *x, const void *ref, void *sig_out, double *errsq_out);

/* ---- single-input adaptive equalizers of the direct-detection chain on the device (optic/dsp/equalization.py:1176-2143 dfe, ffe,
 * volterra and their cores; optic/dsp/core.py:720 anorm), the stage between pnorm and fastBERcalc.
 * One recursion covers the three equalizers: LMS over a regressor phi(k),  y = w . phi,  e = r - y,  w += mu_s e conj(phi), with r
 * the training symbol while k < nTrain and otherwise the nearest table point (the first minimum of |y - c| in table order); the
 * update happens while k < nTrain, or always with SSF_SISO_FULLTIME.
 *   SSF_SISO_FFE       phi = window (nTaps samples)
 *   SSF_SISO_DFE       phi = [window ; the last nFB references r, newest first, zeros at the start]
 *   SSF_SISO_VOLTERRA  phi = [window ; w[t2+i] w[t2+j] ; w[t3+i] w[t3+j] w[t3+l] (order 3)], steps mu, mu / 2, mu / 7,
 *                      t2 = (nTaps - n2) / 2, t3 = (nTaps - n3) / 2; real data only
 *   SSF_SISO_ANORM     sig_out = x / max |x| (n values, float64 or complex128); everything but n, dtype, x and sig_out is ignored
 *   x           n values of `dtype` (any ssf_metrics_dtype), host or device; never written.  The kernels divide by
 *               sqrt(mean |x|^2) and round to single precision where prec32 is set (volterra: then divide by the maximum modulus
 *               and round again) as they load; the nTaps / 2 zeros the reference pads at both ends are not stored
 *   ref         nref values of ref_dtype (real with real x, complex with complex x), host or device; normalised by its own mean
 *               power over all nref values; nref >= min(nTrain, N); may be NULL with nref = 0
 *   const_tab   M (re, im) pairs, host: the decision table as the caller normalised it
 *   coef_inout  ncoef values (float64, or complex128 for complex x), host: ffe f; dfe [f ; b]; volterra [h1 ; h2 row-major ;
 *               h3 row-major (order 3 only)] -- the initial coefficients in, the final ones out
 *   sig_out     N = n / SpS values, float64 or complex128, host or device (volterra: divided by sqrt(mean sig_out^2) at the end)
 *   mse_out     N float64, host or device: |e|^2 of every symbol
 * Symbol k of a pass reads stream[k SpS .. k SpS + nTaps): the padded input, whose SpS samples behind symbol k are zeros unless
 * k SpS + nTaps + SpS < n + 2 (nTaps / 2).  With preconvIters > 1 and nTrain < N every pass but the last ends behind symbol nTrain
 * and the next one starts from the window that pass ended with.
 * One wavefront walks every symbol that adapts or feeds a later decision with ncoef / 64 coefficients per lane in registers;
 * for SSF_SISO_FFE and SSF_SISO_VOLTERRA in SSF_SISO_DATA_AIDED mode the symbols of the last pass from nTrain on run one per
 * thread with the coefficients fixed.  On return serial_symbols, parallel_symbols and R say what ran.
 * Limits: ncoef <= 1536 (24 per lane), nTaps <= 256, nFB <= 256, 1 <= SpS <= 8, SpS <= nTaps, n2, n3 <= nTaps, 2 <= M <= 1024. */
typedef enum { SSF_SISO_FFE = 0, SSF_SISO_DFE = 1, SSF_SISO_VOLTERRA = 2, SSF_SISO_ANORM = 3 } ssf_siso_kind;
typedef enum { SSF_SISO_DATA_AIDED = 0, SSF_SISO_FULLTIME = 1 } ssf_siso_mode;
typedef struct {
    int64_t n;                    /* input samples */
    int64_t nref;                 /* values of ref */
    int64_t nTrain;
    int32_t kind;                 /* ssf_siso_kind */
    int32_t mode;                 /* ssf_siso_mode */
    int32_t dtype, ref_dtype;     /* ssf_metrics_dtype */
    int32_t prec32;               /* 1: normalised inputs are rounded to single precision */
    int32_t order;                /* volterra: 2 or 3 */
    int32_t nTaps;                /* nTaps, nTapsFF or n1Taps */
    int32_t nFB, n2, n3;
    int32_t SpS, M;
    int32_t preconvIters;
    int32_t ncoef;
    int32_t no_frozen;            /* measurement aid: 1 keeps every symbol with the serial kernel */
    int32_t R;                    /* out: coefficient slots per lane of the serial kernel, 0 if it did not run */
    double  mu;
    int64_t serial_symbols;       /* out: symbols the serial kernel walked, all passes */
    int64_t parallel_symbols;     /* out: symbols of the frozen kernel */
} ssf_siso_params;
int  ssf_siso_eq(int device, ssf_siso_params *params, const double *const_tab, void *coef_inout, const void *x, const void *ref,
                 void *sig_out, double *mse_out);

/* ---- sequence and symbol detection on the device (optic/comm/modulation.py:412-481 detector, 582-680 mlse) and the
 * autocorrelation behind estimateWhiteningFilter (optic/dsp/core.py:1194-1227).
 *
 * ssf_mlse: maximum-likelihood sequence estimation by the Viterbi algorithm over the impulse response h, one independent sequence
 * per column.  All path metrics start at zero; the branch metric is |y[n] - expected|^2 with the expected outputs summed in the
 * reference's order; the survivor is the candidate with the smallest metric, the lowest predecessor state among equal ones; the
 * final state is the lowest-index minimum.  Arithmetic is double.
 *   y             (n, cols) row-major, float64 (SSF_M_F64) or complex128 (SSF_M_C128), host or device; never written
 *   h             taps (re, im) pairs, host;  const_tab: M (re, im) pairs, host (imaginary parts are ignored for float64 y)
 *   out           (n, cols) of y's type, host or device: const_tab[k] of the decided symbols
 *   final_metric  cols float64, host: the smallest path metric after the last step
 * One workgroup per column runs the forward pass with one lane per state; the traceback is three launches (per-chunk end-state
 * maps, their composition, one walker per chunk).  The host waits once.  On return states, kernel, chunk and survivor_bytes say
 * what ran; with timing = 1 fwd_ms and tb_ms hold the device time of the forward pass and of the traceback.
 * Limits: 1 <= M <= 64, 1 <= taps <= 11, M^(taps - 1) <= 1024, 1 <= cols <= 64, n >= 1, survivor memory (cols rows of n
 * max(4, states rounded up to 4) bytes, each column rounded up to 16) at most 2^31 bytes. */
typedef struct {
    int64_t n;                    /* symbols per column */
    int32_t cols;
    int32_t dtype;                /* SSF_M_F64 or SSF_M_C128 */
    int32_t M, taps;
    int32_t timing;               /* 1: measure fwd_ms and tb_ms with events */
    int32_t states;               /* out: M^(taps - 1) */
    int32_t kernel;               /* out: 0 the one-wavefront forward kernel, 1 the one of several wavefronts */
    int32_t chunk;                /* out: steps per survivor chunk */
    int64_t survivor_bytes;       /* out */
    double  fwd_ms, tb_ms;        /* out */
} ssf_mlse_params;
int  ssf_mlse(int device, ssf_mlse_params *params, const double *h, const double *const_tab, const void *y, void *out,
              double *final_metric);

/* ssf_detector: symbol-by-symbol decisions.  rule SSF_DET_ML: the first index of the smallest |r - c|^2; SSF_DET_MAP: the first
 * index of the largest -|r - c|^2 / sigma2 + logpx.
 *   r           n values of `dtype` (SSF_M_F64 or SSF_M_C128), host or device; never written
 *   const_tab   M (re, im) pairs, host;  logpx: M float64, host: the log priors (-inf for a zero prior); may be NULL for SSF_DET_ML
 *   decided     n values of r's type, host or device;  ind: n int64, host or device
 * Limits: 1 <= M <= 64, n >= 1, sigma2 > 0 for SSF_DET_MAP. */
typedef enum { SSF_DET_ML = 0, SSF_DET_MAP = 1 } ssf_detector_rule;
int  ssf_detector(int device, int64_t n, int32_t dtype, int32_t M, int32_t rule, double sigma2, const double *const_tab,
                  const double *logpx, const void *r, void *decided, int64_t *ind);

/* ssf_autocorr: r_out[k] = sum_{i >= k} x[i] x[i - k] / (n - k) for k = 0 .. nTaps - 1, one launch for all lags and a fixed-order
 * sum of the workgroups' partials.
 *   x           n float64, host or device; never written;  r_out: nTaps float64, host
 * Limits: 1 <= nTaps <= 256, nTaps <= n. */
int  ssf_autocorr(int device, int64_t n, int32_t nTaps, const void *x, double *r_out);

/* ---- the glue of syncDataSequences, movingAverage and bert (optic/dsp/synchronization.py:30-170, optic/dsp/core.py:829-880,
 * optic/comm/metrics.py:37-105; engine_syncdata.hip).  Array arguments are host or device pointers unless said otherwise; inputs
 * are never written; no atomics: a second call repeats the first bit for bit.
 *
 * ssf_sync_tile: tx_out[i, m] = tx[(i / SpS) mod n_tx, m] where i mod SpS == 0, else 0, and rx_out[i, m] = rx[i, m] for i < n_rx,
 * else 0; both (n_pad, nModes) complex128, rx and tx of any of complex128 / complex64 / float64.
 * Limits: 1 <= nModes <= 8, SpS >= 1, n_rx >= 1, n_tx >= 1, n_rx <= n_pad <= 2^31. */
typedef struct {
    int64_t n_rx, n_tx, n_pad;
    int32_t nModes, SpS;
    int32_t rx_dtype, tx_dtype;   /* SSF_M_C128, SSF_M_C64 or SSF_M_F64 */
} ssf_sync_tile_params;
int  ssf_sync_tile(int device, const ssf_sync_tile_params *params, const void *rx, const void *tx, void *rx_out, void *tx_out);
/* ssf_sync_extract: per column of x ((n, nModes) complex128) the non-zero samples in their order, written from row 0 of out
 * ((n_out, nModes) of out_dtype: SSF_M_C128, or SSF_M_F64 for the real parts), zeros below them; with `normalize` each column is
 * divided by the root mean square of its kept samples.  kept: nModes int64, host.  Samples whose rank is n_out or more are dropped.
 * Limits: 1 <= nModes <= 8, 1 <= n <= 2^31, n_out >= 1. */
int  ssf_sync_extract(int device, int64_t n, int32_t nModes, int64_t n_out, int32_t out_dtype, int32_t normalize, const void *x, void *out,
                      int64_t *kept);
/* ssf_real_part: out[i] = Re x[i]; x count complex128, out count float64 */
int  ssf_real_part(int device, int64_t count, const void *x, void *out);
/* ssf_copy_columns: dst[i, dst_first + j] = src[i, src_first + j] for i < n, j < width; src (n, src_cols) and dst (n, dst_cols)
 * complex128 device arrays, not the same one; the other columns of dst are left as they are.  How syncDataSequences hands decimate
 * at most six columns at a time and puts the results side by side. */
int  ssf_copy_columns(int device, int64_t n, int32_t width, int32_t src_cols, int32_t src_first, int32_t dst_cols, int32_t dst_first,
                      const void *src, void *dst);
/* ssf_moving_average: out[i, c] = (1 / N) sum_{j = i - N/2}^{i + (N-1)/2} x[j, c], zeros outside [0, n); x (n, cols) of complex128,
 * complex64 or float64; out float64 for float64 x and complex128 otherwise.  Limits: 2 <= N <= 2048, n >= 1, 1 <= cols <= 65535. */
int  ssf_moving_average(int device, int64_t n, int32_t cols, int32_t N, int32_t dtype, const void *x, void *out);
/* ssf_bert: the statistics of bert over n float64 samples and n bits (one byte each: a bit is 1 where its byte equals 1, any other value counts as 0).  scal_out: 10 float64, host:
 * n1, n0, I1, I0, std1, std0 (population), Id, Q, the number of decisions (Irx > Id) that differ from the bit, 0.  With an empty
 * class the call succeeds and the caller reads n1 or n0 == 0 (the other values are then not numbers).  Limit: n >= 1. */
int  ssf_bert(int device, int64_t n, const void *irx, const void *bits, double *scal_out);

/* ---- soft-decision FEC on the device: the soft demapper and the LDPC belief-propagation decoder that end the reference's chain
 * (optic/comm/metrics.py:198-239 calcLLR; optic/comm/fec.py:347-758 sumProductAlgorithm, minSumAlgorithm, decodeLDPC).
 *
 * ssf_calc_llr: llr_out[i b + j] = log p0 - log p1 of bit j of symbol i, b = log2 M, with p0 / p1 the sums over the constellation
 * points m (ascending) whose bit j is 0 / 1 of exp(-|x_i - c_m|^2 / sigma2) px_m.  Arithmetic is double; an underflowed sum gives
 * +-inf as in the reference.
 *   x           n values of `dtype` (SSF_M_C128 or SSF_M_C64), host or device; never written
 *   const_tab   M (re, im) pairs, host;  px: M priors, host;  bitmap: (M, b) row-major int32 of 0 / 1, host
 *   llr_out     n b float64, host or device
 * M is a power of two, 2 .. 1024; sigma2 > 0. */
int  ssf_calc_llr(int device, int64_t n, int32_t dtype, int32_t M, double sigma2, const double *const_tab, const int32_t *bitmap,
                  const double *px, const void *x, double *llr_out);

/* The Tanner graph of a parity-check matrix H (m x n, E ones), uploaded once and used by any number of decodes.  The four arrays are
 * those fec.py:388-411 builds, all int32, host:
 *   check_offsets   m + 1: the edges of check c are check_offsets[c] .. check_offsets[c + 1] - 1 (edge id = position in H's CSR)
 *   edge_var        E: the variable of every edge (H's CSR column indices, ascending inside a check)
 *   var_offsets     n + 1;  var_edge_indices  E: the edge ids of variable v, ascending check index
 * Checked here, before anything is uploaded: offsets start at 0, rise and end at E; every index in range; every check has
 * 1 .. 64 edges and every variable at most 64; var_edge_indices lists, for every variable, exactly its own edges. */
typedef struct ssf_ldpc_graph ssf_ldpc_graph;
int  ssf_ldpc_graph_create(int device, int32_t m, int32_t n, int32_t E, const int32_t *check_offsets, const int32_t *edge_var,
                           const int32_t *var_offsets, const int32_t *var_edge_indices, ssf_ldpc_graph **out);
int  ssf_ldpc_graph_destroy(ssf_ldpc_graph *graph);

/* ssf_ldpc_decode: flooding belief propagation, SPA or MSA, of numCodewords codewords at once.
 *   llr_in      (n_, numCodewords) row-major -- or (numCodewords, n_) with transposed = 1 -- of in_dtype, host or device; never
 *               written.  Clipped to +-200 on load; with n_ < n the variables n_ .. n - 1 are punctured (LLR 0) and not returned
 *   llr_out     the posterior LLRs in the same orientation, of `prec`;  bits_out int8 in the same orientation: llr_out < 0
 *   fail_out    numCodewords int8: 0 where the hard decisions satisfied every check at some iteration, else 1
 *   iter_out    numCodewords uint32, may be NULL: the index of that iteration, or maxIter - 1
 *   all four host or device
 * Per codeword: V->C messages start at the LLR; an iteration is check update, variable update, posterior and parity test; the
 * codeword stops at the first iteration that satisfies every check and keeps that iteration's posterior.  A variable sums
 * llr + its C->V messages in ascending check index and sends that sum minus the edge's own message.  MSA: first minimum, second
 * minimum and the product of signs (val >= 0 -> +1).  SPA: tanh(x / 2) once per edge, leave-one-out products from prefix and
 * suffix products, clip to +-0.999999, 2 atanh.
 * Engines: SSF_FEC_LDS runs one workgroup per codeword through all iterations in one launch with messages, LLRs, posteriors and
 * decisions in LDS (graphs with ((E + E / 32 + 1) + 2 n) sizeof(prec) + n + 32 bytes <= 160 KiB); SSF_FEC_GLOBAL keeps them in device
 * memory and launches twice per iteration over all codewords, skipping converged ones by a device-side flag; SSF_FEC_AUTO takes
 * the first when the graph fits.  Both run the same node bodies in the same edge order: results are identical between them and
 * repeat bit for bit.  sync_every > 0 (global engine): the host reads the flags every sync_every iterations and stops when every
 * codeword has converged; 0 never reads them. */
enum ssf_fec_alg { SSF_FEC_SPA = 0, SSF_FEC_MSA = 1 };
enum ssf_fec_prec { SSF_FEC_F64 = 0, SSF_FEC_F32 = 1 };
enum ssf_fec_engine { SSF_FEC_AUTO = 0, SSF_FEC_LDS = 1, SSF_FEC_GLOBAL = 2 };
typedef struct {
    int32_t n_;                   /* rows of llr_in per codeword, 1 .. n */
    int32_t numCodewords;
    int32_t maxIter;              /* >= 1 */
    int32_t alg;                  /* ssf_fec_alg */
    int32_t prec;                 /* ssf_fec_prec: message and output precision */
    int32_t in_dtype;             /* ssf_fec_prec: type of llr_in */
    int32_t transposed;
    int32_t engine;               /* ssf_fec_engine */
    int32_t sync_every;
    int32_t reserved;
} ssf_ldpc_params;
int  ssf_ldpc_decode(int device, const ssf_ldpc_graph *graph, const ssf_ldpc_params *params, const void *llr_in, void *llr_out,
                     int8_t *bits_out, int8_t *fail_out, uint32_t *iter_out);

/* ---- the transmit side of the coded link: LDPC encoding and Gray mapping (optic/comm/fec.py:153-344 encodeLDPC, encodeDVBS2,
 * encoder, 1019-1072 encodeTriang; optic/comm/modulation.py:334-366 modulateGray).  Arithmetic is GF(2) and a table lookup: the
 * results are the reference's, bit for bit, and repeat.
 *
 * An encoder is one code's matrices on one device, uploaded once and used by any number of encodes.  Two forms:
 *   SSF_ENC_DENSE    up to two parity blocks of m1 and m2 rows (m2 may be 0), each row (k + 63) / 64 little-endian 64-bit words, bit l
 *                    of word w multiplying message bit 64 w + l; bits beyond k must be 0.  Parity i of a codeword is the GF(2) dot
 *                    product of row i (block1's rows, then block2's) with the message.  With `systematic` the codeword is the k
 *                    message bits followed by the m1 + m2 parities (P1 and P2 of a triangularised H, or the parity part of a
 *                    systematic G); without, it is the m1 + m2 products alone (the rows of G^T).
 *   SSF_ENC_SPARSE   the DVB-S2 accumulator: indptr (m1 + 1) and indices (nnz) are the CSR of A = H[:, :k], int32; the codeword is the
 *                    message followed by cw[k + i] = (XOR of the message bits in row i of A) ^ cw[k + i - 1].  Rows may be empty.
 * Checked before anything is uploaded: 1 <= k, 1 <= m1 (dense: k <= 32 768, sparse: k <= 131 072 and m1 <= 262 144), indptr rises from 0 to nnz,
 * every index is in 0 .. k - 1. */
enum ssf_enc_form { SSF_ENC_DENSE = 0, SSF_ENC_SPARSE = 1 };
typedef struct {
    int32_t form;                 /* ssf_enc_form */
    int32_t k;                    /* message bits */
    int32_t m1, m2;               /* dense: rows of block1 and block2; sparse: m1 checks, m2 = 0 */
    int32_t systematic;           /* dense only */
    int32_t nnz;                  /* sparse only */
} ssf_ldpc_encoder_desc;
typedef struct ssf_ldpc_encoder ssf_ldpc_encoder;
int  ssf_ldpc_encoder_create(int device, const ssf_ldpc_encoder_desc *desc, const uint64_t *block1, const uint64_t *block2,
                             const int32_t *indptr, const int32_t *indices, ssf_ldpc_encoder **out);
int  ssf_ldpc_encoder_destroy(ssf_ldpc_encoder *encoder);
/* bits_in (k, numCodewords) row-major -- or (numCodewords, k) with transposed = 1 -- one byte per bit, taken as b & 1, host or
 * device, never written; codewords_out (n, numCodewords) or (numCodewords, n) bytes of 0 / 1, host or device: the first n rows of
 * the codeword (n below its full length punctures it, as the reference crops to param.n).  1 <= numCodewords <= 65 535.
 * One launch per call: a workgroup packs its messages into LDS and then owns 256 parity rows of 16 codewords (dense), or the whole
 * scan of one codeword (sparse). */
typedef struct {
    int32_t numCodewords;
    int32_t n;                    /* rows returned per codeword, 1 .. the codeword's length */
    int32_t transposed;
    int32_t reserved;
} ssf_ldpc_encode_params;
int  ssf_ldpc_encode(int device, const ssf_ldpc_encoder *encoder, const ssf_ldpc_encode_params *params, const void *bits_in,
                     void *codewords_out);
/* symb_out[i] = const_tab[sum_j (bits[i b + j] & 1) << (b - 1 - j)], b = log2 M: nsymb complex128 values, host or device;
 * bits: nsymb b bytes, host or device; const_tab: M (re, im) pairs in the order of their labels, host.  M a power of two, 2 .. 1024 */
int  ssf_modulate(int device, int64_t nsymb, int32_t M, const double *const_tab, const void *bits, void *symb_out);

/* ---- OFDM (optic/comm/ofdm.py: modulateOFDM, demodulateOFDM) -------------------------------------------------------------------------
 * A frame has Nfft carriers, of which the first Ns are used (Ns = Nfft, or Nfft / 2 - 1 with Hermitian symmetry): Ni of them carry
 * data, Np the pilot, the rest nothing.  The caller describes the carrier plan with small host tables of int32 (the library checks
 * every entry: the kernels index with them); all arithmetic is double, complex64 is widened on load and rounded once on store.
 * Transforms of 16 .. 8192 points with a power-of-two length run in registers and LDS, one launch; every other length goes through
 * a batched rocFFT between two element-wise kernels (route = SSF_OFDM_ROCFFT asks for that at any length).
 * plan_key: 0, or a number the caller gives to ONE set of tables for as long as the process lives -- a call that repeats the key
 * (and the geometry) of the call before it on the same device reuses the tables that are there and uploads none. */
enum ssf_ofdm_route { SSF_OFDM_AUTO = 0, SSF_OFDM_ROCFFT = 1 };
typedef struct {
    int64_t nframes;              /* >= 1; nframes * SpS * Nfft below 2^31 */
    int32_t Nfft;                 /* 4 .. 2^20 */
    int32_t G;                    /* cyclic prefix, 0 .. Nfft */
    int32_t SpS;                  /* modulator: samples per symbol, 1 .. 64 (the demodulator takes one sample per symbol) */
    int32_t Ns, Ni, Np;           /* carriers in use; data carriers >= 1; pilots (0, or >= 2) */
    int32_t in_dtype, out_dtype;  /* SSF_C64 / SSF_C128 (the demodulator's output has in_dtype) */
    int32_t route;                /* ssf_ofdm_route */
    int32_t reserved;
    double  pilot_re, pilot_im;   /* the pilot symbol (the modulator rounds it to single precision, as the reference's frame does) */
    uint64_t plan_key;
} ssf_ofdm_params;
/* src_map: SpS * Nfft codes, one per input k of the inverse transform (after zero padding and fftshift): 0 nothing,
 * 1 + 8 d data symbol d of the frame, 2 the pilot, + 4 the conjugate of that.  symb: nframes * Ni values of in_dtype, host or device,
 * never written (rounded to single precision where it is complex128: the reference's frame is complex64).  out: nframes *
 * SpS * (Nfft + G) samples of out_dtype, host or device: ifft * sqrt(SpS * Nfft) with the last SpS * G samples in front. */
int  ssf_ofdm_modulate(int device, const ssf_ofdm_params *params, const int32_t *src_map, const void *symb, void *out);
/* sig: nframes * (Nfft + G) samples of in_dtype, host or device, never written.  bin_carrier: Nfft entries, the carrier 0 .. Ns - 1
 * that bin k of fft(frame) is after fftshift (and the Hermitian slice), or -1.  data_carriers: Ni carriers in output order.
 * With Np > 0: pilot_carriers, Np strictly rising, and pilot_hi, Ns entries in 1 .. Np - 1: carrier c lies on the line through the
 * pilots pilot_hi[c] - 1 and pilot_hi[c] (the end segments run on).  The channel is the mean over the frames of |Y / pilot| and of
 * its angle at the pilots, each joined by those lines; every frame is divided by it.  symb_out: nframes * Ni values of in_dtype;
 * H_out: Ns complex128 values or NULL (not written when Np = 0); host or device. */
int  ssf_ofdm_demodulate(int device, const ssf_ofdm_params *params, const int32_t *bin_carrier, const int32_t *data_carriers,
                         const int32_t *pilot_carriers, const int32_t *pilot_hi, const void *sig, void *symb_out, void *H_out);

/* ---- first-order perturbation model of the intrachannel NLIN (optic/models/perturbation.py: calcNLINperturbation,
 * calcNLINperturbationSimplified, perturbationNLIN) ------------------------------------------------------------------------------
 * With m = j - L, n = L - i and the symbols zero outside 0 .. n - 1 the reference's sum over its (2L+1)^2 window is
 *     dx[t] = sum_m x[t+m] sum_n C_ifwm[L-n, L+m] P[t+n, m] + x[t] sum_n C_ixpm[L-n, L] |y[t+n]|^2,   P[s, m] = x[s] conj(x[s+m]) + y[s] conj(y[s+m])
 * (dy with x and y exchanged).  The caller describes the coefficients as a plan of host tables (the library checks every entry):
 *   pass      npass x {kind, m, first, count}: one inner sum over n.  kind 0: the line P[., m], the result times x[t+m] to dx and
 *             times y[t+m] to dy; kind 1: the line |y|^2, times x[t] to dx; kind 2: the line |x|^2, times y[t] to dy (m = 0 for both).
 *             Its coefficients are coef[first .. first + count).  dense: count = 2L+1 and coefficient k belongs to n = k - L;
 *             else to n = nidx[first + k], -L .. L, rising strictly within the pass (so count <= 2L+1 either way).
 *   coef      ncoef (re, im) pairs;  nidx: ncoef int32 (not read when dense, may be NULL)
 *   phase_m, phase_c   nphase values of m, -L .. L, and (re, im) coefficients:
 *             phi_x[t] = sum_k Im(phase_c[k]) (2 |x[t+m_k]|^2 + |y[t+m_k]|^2) + Im(ispm) (|x[t+o]|^2 + |y[t+o]|^2), o = ispm_offset
 * entry SSF_NLIN_CALC: x, y are n values of in_dtype each; each is divided by the root of its mean power (rounded to single precision
 * where in_dtype or prec is SSF_C64); out0 = dx, out1 = dy: n values of prec; out2 = phi_x, out3 = phi_y: n doubles.
 * entry SSF_NLIN_FIELD: x is the (n, 2) field of in_dtype, y NULL; every column is normalised to unit power and then as above;
 * out0 = nlin, (n, 2) of in_dtype: sqrt(P) E (e^{j P phi} - 1) + P^{3/2} d e^{j P phi} with P = peak_power, E the column after the
 * first normalisation; out1 .. out3 NULL.  All arrays host or device, inputs never written.  All sums run in double in a fixed
 * order.  plan_key: 0, or a number the caller gives to ONE set of tables for as long as the process lives -- a call that names a
 * key the device still holds (the last 8, with the same L and counts; they live as long as the process) uploads no table. */
enum ssf_nlin_entry { SSF_NLIN_CALC = 0, SSF_NLIN_FIELD = 1 };
typedef struct {
    int64_t n;                    /* symbols, 1 .. 2^32 */
    int32_t L;                    /* matrix order, 1 .. 128 */
    int32_t npass, ncoef, nphase; /* >= 0; npass <= 2L + 3, ncoef <= (2L + 3)(2L + 1), nphase <= 2L + 1 */
    int32_t dense;                /* 0 / 1 */
    int32_t entry;                /* ssf_nlin_entry */
    int32_t in_dtype, prec;       /* SSF_C64 / SSF_C128 */
    int32_t ispm_offset;          /* -L .. L */
    int32_t reserved;
    double  ispm_re, ispm_im;     /* C_ispm */
    double  peak_power;           /* SSF_NLIN_FIELD: half the launch power [W] */
    uint64_t plan_key;
} ssf_nlin_params;
int  ssf_pert_nlin(int device, const ssf_nlin_params *params, const int32_t *pass, const double *coef, const int32_t *nidx,
                   const int32_t *phase_m, const double *phase_c, const void *x, const void *y, void *out0, void *out1, void *out2,
                   void *out3);

/* ---- the sampling clock on the device: the converters that put a clock offset on a signal and the stage that takes it off
 * (optic/dsp/core.py:272-349 clockSamplingInterp, quantizer; optic/models/devices.py:793-1022 adc, dac; optic/dsp/clockRecovery.py
 * gardnerClockRecovery, calcClockDrift).  Arrays are (rows, ncols) row-major, host or device; inputs are never written.  Arithmetic
 * is double, single-precision data are widened on load and rounded on store; the converters give numpy's results bit for bit.
 *
 * ssf_clock_interp: np.interp(tout, tin, x) per column with tin[j] = j inTs and tout[i] = i outTs, or the caller's n_out times
 * t_re (host or device; NULL: computed).  form SSF_CLOCK_REAL: real data, numpy's real rule (the slope is a quotient);
 * SSF_CLOCK_COMPLEX: complex data, numpy's complex rule (the slope is a product with a reciprocal), one time per output;
 * SSF_CLOCK_COMPONENTS: complex data, each component by the real rule, the imaginary parts at the times t_im (NULL: t_re).
 * Then, in the same pass: clip != 0: np.clip to [lo, hi] (complex data: to lo + 1j lo .. hi + 1j hi in numpy's lexicographic order
 * of complex numbers); quantize != 0: every component to the nearest of qmin + i qdelta, i < qlevels (the first on a tie).
 * out has x's dtype, or float64 / complex128 with quantize. */
enum ssf_clock_form { SSF_CLOCK_REAL = 0, SSF_CLOCK_COMPLEX = 1, SSF_CLOCK_COMPONENTS = 2 };
typedef struct {
    int64_t n_in, n_out;          /* rows of x and of out; 1 <= n_in, 0 <= n_out */
    int32_t ncols;
    int32_t dtype;                /* ssf_metrics_dtype of x */
    int32_t form;                 /* ssf_clock_form */
    int32_t clip, quantize;       /* 0 / 1 */
    int32_t reserved;
    double  inTs, outTs;          /* > 0 */
    double  lo, hi;               /* clip */
    double  qmin, qdelta;         /* quantize: qdelta > 0 */
    int64_t qlevels;              /* >= 1 */
} ssf_clock_params;
int  ssf_clock_interp(int device, const ssf_clock_params *params, const void *x, const double *t_re, const double *t_im, void *out);
/* out[i] (float64) = the level nearest to x[i], count values of `dtype`; of a complex value the real part is quantised */
int  ssf_quantize(int device, int64_t count, int32_t dtype, double qmin, double qdelta, int64_t qlevels, const void *x, double *out);
/* np.clip(x, lo, hi) over count values of `dtype` (complex: the lexicographic clip above); out has x's dtype */
int  ssf_clip(int device, int64_t count, int32_t dtype, double lo, double hi, const void *x, void *out);
/* out2 (host) = {min, max} over the real and imaginary parts of count values; NaNs are passed over */
int  ssf_minmax(int device, int64_t count, int32_t dtype, const void *x, double *out2);
/* out = (x + noise) scale over count doubles; noise may be NULL; has_scale == 0: no product */
int  ssf_clock_scale_add(int device, int64_t count, double scale, int32_t has_scale, const double *x, const double *noise, double *out);
/* ssf_gardner: Gardner clock recovery with a PI loop filter, one wavefront per mode.  x: (n, nModes) complex128 or complex64, taken
 * as followed by lpad rows of zeros.  sig_out: (Ln, nModes) complex64, t_out: (Ln, nModes) float64, both zero where the loop did
 * not write; last_n (host): per mode the output index the loop ended at.  The arithmetic is the one tests/clock_restatement.py
 * states (double state, outputs rounded to single, the detector on the rounded outputs).  SSF_ERR_UNSUPPORTED if a mode's loop falls
 * back further behind its furthest output than the kernel keeps in LDS. */
typedef struct {
    int64_t n, lpad, Ln;          /* n >= 1, lpad >= 0, 1 <= Ln */
    int32_t nModes;               /* 1 .. 65535 */
    int32_t dtype;                /* SSF_M_C128 or SSF_M_C64 */
    int32_t nyquist;              /* 1: gardnerTEDnyquist, 0: gardnerTED */
    int32_t reserved;
    double  kp, ki;
} ssf_gardner_params;
int  ssf_gardner(int device, const ssf_gardner_params *params, const void *x, void *sig_out, double *t_out, int64_t *last_n);
/* calcClockDrift: per column of t (n, ncols) float64 the peaks of |diff(t - mean)| of height >= 0.5 (scipy.signal.find_peaks' rule)
 * -> ppm_out[col] (host) = sign(mean) 1e6 (count - 1) / (last - first), NaN with fewer than two peaks.  The mean is taken over the
 * whole array (per_column == 0, the reference's 2-D call) or over the column (the reference's call per 1-D column). */
int  ssf_clock_drift(int device, int64_t n, int32_t ncols, int32_t per_column, const double *t, double *ppm_out);

/* ---- the general array layer of DeviceArray (engine_array.hip, array_kernels.h): what stands between two stages of a notebook --
 * indexing, transposes, concatenation, element-wise arithmetic, dtype conversion, reductions -- with numpy as the definition.
 * Array data (src, dst, a, x, out, and b unless it is a row) are DEVICE pointers: a host pointer there is SSF_ERR_BAD_ARG.  The
 * small operands -- the index of ssf_array_take, a row operand, the centre of a reduction, the fill value -- may be host memory;
 * reduction results are written to host memory.  No entry point writes its operands or works in place.  A call of zero elements
 * returns SSF_OK without a launch.  Every entry point has finished its work when it returns: a result may be handed to any other
 * engine's stream.  dtype arguments are ssf_metrics_dtype.  Arithmetic is double, single-precision data are widened on load and
 * rounded once on store; a real operand beside a complex one is promoted to (re, +0) as numpy's casts do. */
#define SSF_ARRAY_MAX_DIM 4
typedef struct {
    int32_t ndim;                 /* 0 .. SSF_ARRAY_MAX_DIM */
    int32_t itemsize;             /* 1, 2, 4, 8 or 16 bytes */
    int64_t offset;               /* of element (0, 0, ..) from the pointer, in elements */
    int64_t extent;               /* elements of the allocation behind the pointer: every element reached lies in [0, extent) */
    int64_t shape[SSF_ARRAY_MAX_DIM];
    int64_t stride[SSF_ARRAY_MAX_DIM];    /* in elements, any sign */
} ssf_array_desc;
/* dst[dst_desc] = src[src_desc]: same ndim, shape and itemsize on both sides, elements taken in C order of the shape.  Serves
 * slices with any step, integer indices, concatenate and stack.  Contiguous, 16-byte aligned sides move 16 bytes per lane. */
int  ssf_array_copy(int device, const ssf_array_desc *src_desc, const void *src, const ssf_array_desc *dst_desc, void *dst);
/* dst (n_idx, inner) = src (n_src, inner)[idx]: idx holds n_idx int32 or int64 (idx_itemsize 4 or 8), host or device.  Negative
 * entries wrap; an entry still out of range is CLAMPED to the first or last row (the host checks what it can see). */
int  ssf_array_take(int device, int64_t n_src, int64_t n_idx, int64_t inner, int32_t itemsize, int32_t idx_itemsize, const void *idx,
                    const void *src, void *dst);
/* dst (cols, rows) = src (rows, cols) transposed, through a padded LDS tile */
int  ssf_array_transpose(int device, int64_t rows, int64_t cols, int32_t itemsize, const void *src, void *dst);
/* dst[0 .. count) = the itemsize bytes at value (host) */
int  ssf_array_fill(int device, int64_t count, int32_t itemsize, const void *value, void *dst);
enum ssf_array_binary_op { SSF_ARRAY_ADD = 0, SSF_ARRAY_SUB = 1, SSF_ARRAY_MUL = 2, SSF_ARRAY_DIV = 3 };
/* how the second operand meets the first: element for element; one value (scalar_re, scalar_im; b is ignored); a row of `inner`
 * values along the last axis (host or device); a column: one value per `inner` consecutive elements of a (device) */
enum ssf_array_bcast { SSF_ARRAY_SAME = 0, SSF_ARRAY_SCALAR = 1, SSF_ARRAY_ROW = 2, SSF_ARRAY_COLUMN = 3 };
typedef struct {
    int32_t op;                   /* ssf_array_binary_op */
    int32_t swap;                 /* 1: b op a (the reflected operators) */
    int32_t a_dtype, b_dtype, out_dtype;      /* out_dtype is complex exactly if a_dtype or b_dtype is */
    int32_t kind;                 /* ssf_array_bcast */
    int64_t count;                /* elements of a and of out */
    int64_t inner;                /* SSF_ARRAY_ROW, SSF_ARRAY_COLUMN: divides count */
    double  scalar_re, scalar_im; /* SSF_ARRAY_SCALAR, taken as of b_dtype's kind */
} ssf_array_binary_params;
/* out = a op b.  Complex products are re = ar br - ai bi, im = ar bi + ai br; complex quotients are Smith's form, as numpy's loop. */
int  ssf_array_binary(int device, const ssf_array_binary_params *params, const void *a, const void *b, void *out);
/* REAL, IMAG, ABS, ABS2 (re^2 + im^2) and ANGLE give a real out_dtype; NEG, CONJ and EXP keep the kind; SQRT is for real arrays;
 * CONVERT goes between any two dtypes except from complex to real.  ABS of a complex value is hypot: finite where the value is. */
enum ssf_array_unary_op { SSF_ARRAY_NEG = 0, SSF_ARRAY_CONJ = 1, SSF_ARRAY_REAL = 2, SSF_ARRAY_IMAG = 3, SSF_ARRAY_ABS = 4,
                          SSF_ARRAY_ABS2 = 5, SSF_ARRAY_ANGLE = 6, SSF_ARRAY_EXP = 7, SSF_ARRAY_SQRT = 8, SSF_ARRAY_CONVERT = 9 };
int  ssf_array_unary(int device, int32_t op, int32_t in_dtype, int32_t out_dtype, int64_t count, const void *x, void *out);
/* per column of x (rows, cols) over its rows (the whole array: cols = 1), accumulated in double:
 * SUM -> out[2 c], out[2 c + 1] = the sums of the real and imaginary parts; SUMSQDEV -> out[2 c] = sum |x - centre[c]|^2 with
 * centre (cols, 2) doubles; MIN / MAX (real dtypes) -> out[c] and arg_out[c], numpy's rule: a NaN wins, ties go to the lowest row.
 * At most 256 partial results per column, added in index order by one lane: a result repeats bit for bit. */
enum ssf_array_reduce_op { SSF_ARRAY_SUM = 0, SSF_ARRAY_SUMSQDEV = 1, SSF_ARRAY_MIN = 2, SSF_ARRAY_MAX = 3 };
int  ssf_array_reduce(int device, int32_t op, int32_t dtype, int64_t rows, int32_t cols, const double *center, const void *x, double *out,
                      int64_t *arg_out);
/* freqShift (optic/dsp/core.py:1050-1072): out (n, ncols) complex128 = x exp(1j ((2 pi) deltaF) (k (1 / Fs))) with k the row, the
 * phasor formed in the kernel.  x and out may be host or device memory. */
int  ssf_freq_shift(int device, int64_t n, int32_t ncols, int32_t dtype, double deltaF, double Fs, const void *x, void *out);

#ifdef __cplusplus
}
#endif
#endif /* SSF_H */
