"""ctypes binding of libssf_hip.so (C ABI: include/ssf.h).  No fallback: if the
shared library is missing, importing a propagation function still works but the
first call raises RuntimeError telling the user to build it."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SSF_LIB", os.path.join(_HERE, "libssf_hip.so"))

SSF_C64, SSF_C128 = 0, 1
MODEL_NLSE, MODEL_MANAKOV = 0, 1
AMP_NONE, AMP_IDEAL, AMP_EDFA = 0, 1, 2
ENGINE_AUTO, ENGINE_ROCFFT, ENGINE_FUSED = 0, 1, 2
ENGINE_NAMES = {ENGINE_AUTO: "auto", ENGINE_ROCFFT: "rocfft", ENGINE_FUSED: "fused"}
PIPELINE_NAMES = {0: "fused-device", 1: "fused-rows", 2: "fused-bluestein", 3: "rocfft"}      # ssf_plan_pipeline

STATUS = {0: "OK", -1: "bad argument", -2: "HIP error", -3: "out of device memory", -4: "FFT error",
          -5: "no device", -6: "unsupported", -7: "bad call order", -8: "RCCL error"}


class Params(C.Structure):
    _fields_ = [("model", C.c_int32), ("direction", C.c_int32), ("Fs", C.c_double), ("Fc", C.c_double),
                ("alpha", C.c_double), ("D", C.c_double), ("gamma", C.c_double), ("Lspan", C.c_double),
                ("Nspans", C.c_int32), ("maxIter", C.c_int32), ("hz", C.c_double), ("tol", C.c_double),
                ("nlprMethod", C.c_int32), ("amp", C.c_int32), ("maxNlinPhaseRot", C.c_double),
                ("NF", C.c_double), ("n_save", C.c_int32), ("rng_row_offset", C.c_int32),
                ("save_spans", C.POINTER(C.c_int32)), ("rng_seed", C.c_int64)]


class Stats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("iterations", C.c_int64), ("transforms", C.c_int64),
                ("nonconverged_steps", C.c_int64), ("device_ms", C.c_double),
                ("bytes_algorithmic", C.c_double), ("engine", C.c_int32), ("n_snapshots", C.c_int32),
                ("decided_ahead", C.c_int64), ("rebuilt_iterates", C.c_int64),
                ("recovered_fields", C.c_int64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["engine"] = ENGINE_NAMES.get(d["engine"], str(d["engine"]))
        return d


class Trace(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("count", C.c_int64), ("hz", C.POINTER(C.c_double)),
                ("iters", C.POINTER(C.c_int32)), ("lims", C.POINTER(C.c_double))]


class KernelTimes(C.Structure):
    _fields_ = [("row_ms", C.c_double), ("col_ms", C.c_double), ("other_ms", C.c_double),
                ("row_n", C.c_int64), ("col_n", C.c_int64), ("other_n", C.c_int64),
                ("col_h_ms", C.c_double), ("col_adv_ms", C.c_double), ("col_fin_ms", C.c_double),
                ("col_h_n", C.c_int64), ("col_adv_n", C.c_int64), ("col_fin_n", C.c_int64), ("outliers", C.c_int64)]


class RxParams(C.Structure):
    """ssf_rx_params (include/ssf.h)."""
    _fields_ = [("Fs", C.c_double), ("polRotation", C.c_double), ("pdl", C.c_double), ("polDelay", C.c_double),
                ("ampImb", C.c_double * 2), ("phaseImb", C.c_double * 2), ("timeSkew", C.c_double * 2),
                ("R", C.c_double), ("Tc", C.c_double), ("Id", C.c_double), ("RL", C.c_double), ("B", C.c_double),
                ("IpdSat", C.c_double), ("N", C.c_int32), ("fType", C.c_int32), ("ideal", C.c_int32),
                ("shotNoise", C.c_int32), ("thermalNoise", C.c_int32), ("currentSaturation", C.c_int32),
                ("bandwidthLimitation", C.c_int32), ("pad_", C.c_int32), ("rng_seed", C.c_int64), ("Fs_pd", C.c_double)]


class TxParams(C.Structure):
    """ssf_tx_params (include/ssf.h)."""
    _fields_ = [("Fs", C.c_double), ("mzmScale", C.c_double), ("nSymbols", C.c_int64), ("SpS", C.c_int32),
                ("nChannels", C.c_int32), ("nPolModes", C.c_int32), ("ntaps", C.c_int32),
                ("pn_sigma", C.c_double), ("pn_seed", C.c_uint64), ("phi_rows", C.c_int32), ("reserved", C.c_int32)]


class MetricsParams(C.Structure):
    """ssf_metrics_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("discard", C.c_int64), ("nModes", C.c_int32), ("M", C.c_int32), ("dtype", C.c_int32),
                ("transposed", C.c_int32), ("rotate", C.c_int32), ("want", C.c_int32), ("Es", C.c_double), ("H", C.c_double)]


class MetricsResult(C.Structure):
    """ssf_metrics_result (include/ssf.h): one per mode."""
    _fields_ = [("BER", C.c_double), ("SER", C.c_double), ("SNR", C.c_double), ("GMI", C.c_double), ("NGMI", C.c_double),
                ("MI", C.c_double), ("EVM", C.c_double), ("bit_errors", C.c_int64), ("symbol_errors", C.c_int64), ("n", C.c_int64)]


class CprParams(C.Structure):
    """ssf_cpr_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("nModes", C.c_int32), ("M", C.c_int32), ("dtype", C.c_int32), ("B", C.c_int32), ("Nh", C.c_int32),
                ("runFOE", C.c_int32), ("P", C.c_int32), ("reserved", C.c_int32), ("Fs", C.c_double)]


class SyncParams(C.Structure):
    """ssf_sync_params (include/ssf.h)."""
    _fields_ = [("n_rx", C.c_int64), ("n_tx", C.c_int64), ("nModes", C.c_int32), ("SpS", C.c_int32), ("mode", C.c_int32),
                ("rx_dtype", C.c_int32), ("tx_dtype", C.c_int32), ("reserved", C.c_int32)]


class SyncResult(C.Structure):
    """ssf_sync_result (include/ssf.h)."""
    _fields_ = [("delay", C.c_int64 * 8), ("swap", C.c_int32 * 8), ("rot", C.c_int32 * 8), ("conj", C.c_int32 * 8),
                ("corrMatrix", C.c_double * 64)]


SYNC_MODES = {"amp": 0, "real": 1}                                                          # ssf_sync_mode
SYNC_ROT = (1, -1, 1j, -1j)                                                                 # ssf_sync_result.rot
SYNC_MAX_MODES = 8


class EqStage(C.Structure):
    """ssf_eq_stage (include/ssf.h)."""
    _fields_ = [("L", C.c_int64), ("alg", C.c_int32), ("reserved", C.c_int32), ("mu", C.c_double)]


class EqParams(C.Structure):
    """ssf_eq_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("total", C.c_int64), ("nref", C.c_int64), ("nModes", C.c_int32), ("nTaps", C.c_int32),
                ("SpS", C.c_int32), ("dtype", C.c_int32), ("ref_dtype", C.c_int32), ("nStages", C.c_int32), ("numIter", C.c_int32),
                ("M", C.c_int32), ("nRadii", C.c_int32), ("reserved", C.c_int32), ("Rcma", C.c_double)]


class LdpcParams(C.Structure):
    """ssf_ldpc_params (include/ssf.h)."""
    _fields_ = [("n_", C.c_int32), ("numCodewords", C.c_int32), ("maxIter", C.c_int32), ("alg", C.c_int32), ("prec", C.c_int32),
                ("in_dtype", C.c_int32), ("transposed", C.c_int32), ("engine", C.c_int32), ("sync_every", C.c_int32),
                ("reserved", C.c_int32)]


FEC_ALGS = {"SPA": 0, "MSA": 1}                                                             # ssf_fec_alg
FEC_PRECS = {"float64": 0, "float32": 1}                                                    # ssf_fec_prec
FEC_ENGINES = {"auto": 0, "lds": 1, "global": 2}                                            # ssf_fec_engine
FEC_MAX_DEGREE = 64        # largest check or variable degree (fec_kernels.h: kMaxDeg)
FEC_LDS_BUDGET = 160 * 1024    # bytes of LDS the one-workgroup decoder may use (fec_kernels.h: kLdsBudget)


def fec_lds_bytes(E, n, prec):
    """LDS the one-workgroup LDPC decoder needs for a graph of E edges and n variables (fec_kernels.h: lds_bytes)."""
    w = 8 if FEC_PRECS[prec] == 0 else 4
    return ((E + (E >> 5) + 1) + 2 * n) * w + 16 + ((n + 15) // 16) * 16


class EncoderDesc(C.Structure):
    """ssf_ldpc_encoder_desc (include/ssf.h)."""
    _fields_ = [("form", C.c_int32), ("k", C.c_int32), ("m1", C.c_int32), ("m2", C.c_int32), ("systematic", C.c_int32),
                ("nnz", C.c_int32)]


class EncodeParams(C.Structure):
    """ssf_ldpc_encode_params (include/ssf.h)."""
    _fields_ = [("numCodewords", C.c_int32), ("n", C.c_int32), ("transposed", C.c_int32), ("reserved", C.c_int32)]


ENC_DENSE, ENC_SPARSE = 0, 1                                                                # ssf_enc_form
ENC_TILE = 16              # codewords whose packed messages share a workgroup of the dense encoder (enc_kernels.h: kTile)
ENC_ROWS = 256             # parity rows per workgroup of the dense encoder, one per lane (kRows)
ENC_WAVE_SPAN = 64         # checks the accumulator scans with one ballot (kWave)
ENC_SPAN = 256             # checks whose parities a workgroup of the accumulator takes in one pass (kSpan)
ENC_CARRY_SPAN = 64 * 64   # checks whose 64 ballots get their carries from one ballot of totals (kWave * kWave)
ENC_BLOCK = 256            # lanes per workgroup of every encoder kernel, modulateGray's included (kBlock)
ENC_MAX_K_DENSE = 32768    # message bits of the dense form: 16 packed messages in 64 KiB of LDS (kMaxWordsDense)
ENC_MAX_K_SPARSE = 131072  # message bits of the sparse form (kMaxWordsSparse)
ENC_MAX_M_SPARSE = 262144  # checks of the sparse form (kMaxChecksSparse)


class OfdmParams(C.Structure):
    """ssf_ofdm_params (include/ssf.h)."""
    _fields_ = [("nframes", C.c_int64), ("Nfft", C.c_int32), ("G", C.c_int32), ("SpS", C.c_int32), ("Ns", C.c_int32), ("Ni", C.c_int32),
                ("Np", C.c_int32), ("in_dtype", C.c_int32), ("out_dtype", C.c_int32), ("route", C.c_int32), ("reserved", C.c_int32),
                ("pilot_re", C.c_double), ("pilot_im", C.c_double), ("plan_key", C.c_uint64)]


OFDM_ROUTES = {"auto": 0, "rocfft": 1}                                                       # ssf_ofdm_route
OFDM_SRC_ZERO, OFDM_SRC_DATA, OFDM_SRC_PILOT, OFDM_SRC_CONJ = 0, 1, 2, 4                     # the codes of src_map (ofdm_kernels.h)
OFDM_MIN_LDS, OFDM_MAX_LDS = 16, 8192      # power-of-two transform lengths that run in registers and LDS (kMinLg, kMaxLg)


def ofdm_lds_length(L):
    """Whether a transform of L points runs in registers and LDS (ofdm_kernels.h: lds_length); every other length is rocFFT's."""
    return OFDM_MIN_LDS <= L <= OFDM_MAX_LDS and L & (L - 1) == 0


def ofdm_frames_per_workgroup(L):
    """Frames a workgroup of the register-and-LDS kernels takes at L points (ofdm_kernels.h: frames_per_workgroup)."""
    return max(256, L // 16) // (L // 16)


class NlinParams(C.Structure):
    """ssf_nlin_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("L", C.c_int32), ("npass", C.c_int32), ("ncoef", C.c_int32), ("nphase", C.c_int32),
                ("dense", C.c_int32), ("entry", C.c_int32), ("in_dtype", C.c_int32), ("prec", C.c_int32), ("ispm_offset", C.c_int32),
                ("reserved", C.c_int32), ("ispm_re", C.c_double), ("ispm_im", C.c_double), ("peak_power", C.c_double),
                ("plan_key", C.c_uint64)]


NLIN_CALC, NLIN_FIELD = 0, 1                                                                 # ssf_nlin_entry
NLIN_MAX_ORDER = 128       # largest matrixOrder (nlin_kernels.h: kMaxL)
NLIN_OUT = 4               # consecutive outputs a lane of the main kernel holds (kOut)
NLIN_TILE = 256            # symbols per workgroup of the main kernel (kTile = kLanes kOut)
NLIN_MAX_SPLIT = 16        # most shares the passes of a plan are dealt into (kMaxSplit)
NLIN_TARGET_GROUPS = 2048  # workgroups the main kernel aims at (kTargetGroups)


def nlin_split(n, npass):
    """Shares the passes are dealt into for n symbols (nlin_kernels.h: split_for)."""
    tiles = (n + NLIN_TILE - 1) // NLIN_TILE
    return min((NLIN_TARGET_GROUPS + tiles - 1) // tiles, NLIN_MAX_SPLIT, npass)


class ClockParams(C.Structure):
    """ssf_clock_params (include/ssf.h)."""
    _fields_ = [("n_in", C.c_int64), ("n_out", C.c_int64), ("ncols", C.c_int32), ("dtype", C.c_int32), ("form", C.c_int32),
                ("clip", C.c_int32), ("quantize", C.c_int32), ("reserved", C.c_int32), ("inTs", C.c_double), ("outTs", C.c_double),
                ("lo", C.c_double), ("hi", C.c_double), ("qmin", C.c_double), ("qdelta", C.c_double), ("qlevels", C.c_int64)]


class GardnerParams(C.Structure):
    """ssf_gardner_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("lpad", C.c_int64), ("Ln", C.c_int64), ("nModes", C.c_int32), ("dtype", C.c_int32),
                ("nyquist", C.c_int32), ("reserved", C.c_int32), ("kp", C.c_double), ("ki", C.c_double)]


CLOCK_REAL, CLOCK_COMPLEX, CLOCK_COMPONENTS = 0, 1, 2                                        # ssf_clock_form
CLOCK_BLOCK = 256          # lanes per workgroup of the element-wise passes and the reductions (clock_kernels.h: kBlock)
CLOCK_MAX_BLOCKS = 4096    # workgroups of a grid-stride pass (kMaxBlocks)
CLOCK_CHUNK = 256          # input samples per staging chunk of the clock recovery kernel (kChunk)
CLOCK_RING = 256           # outputs of a column the clock recovery kernel holds in LDS (kRing)
CLOCK_FLUSH = 64           # outputs that leave in one store (kFlush)
CLOCK_LAG = 128            # ... once the loop is this far ahead of the first of them (kLag)


ARRAY_MAX_DIM = 4                                                                            # SSF_ARRAY_MAX_DIM


class ArrayDesc(C.Structure):
    """ssf_array_desc (include/ssf.h)."""
    _fields_ = [("ndim", C.c_int32), ("itemsize", C.c_int32), ("offset", C.c_int64), ("extent", C.c_int64),
                ("shape", C.c_int64 * ARRAY_MAX_DIM), ("stride", C.c_int64 * ARRAY_MAX_DIM)]


class ArrayBinaryParams(C.Structure):
    """ssf_array_binary_params (include/ssf.h)."""
    _fields_ = [("op", C.c_int32), ("swap", C.c_int32), ("a_dtype", C.c_int32), ("b_dtype", C.c_int32), ("out_dtype", C.c_int32),
                ("kind", C.c_int32), ("count", C.c_int64), ("inner", C.c_int64), ("scalar_re", C.c_double), ("scalar_im", C.c_double)]


ARRAY_BINARY = {"add": 0, "sub": 1, "mul": 2, "div": 3}                                      # ssf_array_binary_op
ARRAY_UNARY = {"neg": 0, "conj": 1, "real": 2, "imag": 3, "abs": 4, "abs2": 5, "angle": 6, "exp": 7, "sqrt": 8, "convert": 9}
ARRAY_SAME, ARRAY_SCALAR, ARRAY_ROW, ARRAY_COLUMN = 0, 1, 2, 3                               # ssf_array_bcast
ARRAY_SUM, ARRAY_SUMSQDEV, ARRAY_MIN, ARRAY_MAX = 0, 1, 2, 3                                 # ssf_array_reduce_op
ARRAY_BLOCK = 256          # lanes per workgroup of the array engine's kernels (array_kernels.h: kBlock)
ARRAY_MAX_BLOCKS = 4096    # workgroups of a grid-stride element-wise or movement pass (kMaxBlocks)
ARRAY_RED_BLOCKS = 256     # partial results per column of a reduction (kRedBlocks)
ARRAY_TILE = 32            # the transpose's LDS tile (kTile)

EQ_ALGS = {"nlms": 0, "cma": 1, "rde": 2, "da-rde": 3, "dd-lms": 4, "static": 5}             # ssf_eq_alg
EQ_CHUNK = 64              # output symbols the serial equalizer kernel stages per chunk (eq_kernels.h: kChunk)
EQ_STAGE_ELEMS = 1024      # ... unless ((c - 1) SpS + nTaps) nModes input values would exceed its staging buffer (kStageElems)


def eq_chunk(nModes, nTaps, SpS):
    """Output symbols per staging chunk of the serial equalizer kernel for a geometry (eq_kernels.h: chunk_symbols)."""
    return min(EQ_CHUNK, (EQ_STAGE_ELEMS // nModes - nTaps) // SpS + 1)


class SisoParams(C.Structure):
    """ssf_siso_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("nref", C.c_int64), ("nTrain", C.c_int64), ("kind", C.c_int32), ("mode", C.c_int32),
                ("dtype", C.c_int32), ("ref_dtype", C.c_int32), ("prec32", C.c_int32), ("order", C.c_int32), ("nTaps", C.c_int32),
                ("nFB", C.c_int32), ("n2", C.c_int32), ("n3", C.c_int32), ("SpS", C.c_int32), ("M", C.c_int32),
                ("preconvIters", C.c_int32), ("ncoef", C.c_int32), ("no_frozen", C.c_int32), ("R", C.c_int32), ("mu", C.c_double),
                ("serial_symbols", C.c_int64), ("parallel_symbols", C.c_int64)]


SISO_KINDS = {"ffe": 0, "dfe": 1, "volterra": 2, "anorm": 3}                                 # ssf_siso_kind
SISO_MODES = {"data-aided": 0, "fulltime": 1}                                                # ssf_siso_mode
SISO_MAX_COEFFS = 1536     # coefficients of one call: 24 per lane of the serial kernel (siso_kernels.h: kMaxCoeffs)
SISO_MAX_TAPS = 256        # nTaps, nTapsFF, n1Taps (kMaxTaps)
SISO_MAX_FB = 256          # nTapsFB (kMaxFb)
SISO_MAX_SPS = 8           # (kMaxSpS)
SISO_MAX_M = 1024          # points of the decision table the kernels stage (kMaxM)
SISO_CHUNK = 64            # symbols the serial kernel stages per chunk (kChunk)
SISO_TILE = 256            # symbols per workgroup of the frozen kernel (kTile)


class MlseParams(C.Structure):
    """ssf_mlse_params (include/ssf.h)."""
    _fields_ = [("n", C.c_int64), ("cols", C.c_int32), ("dtype", C.c_int32), ("M", C.c_int32), ("taps", C.c_int32), ("timing", C.c_int32),
                ("states", C.c_int32), ("kernel", C.c_int32), ("chunk", C.c_int32), ("survivor_bytes", C.c_int64), ("fwd_ms", C.c_double),
                ("tb_ms", C.c_double)]


SEQDET_MAX_M = 64          # constellation points of mlse and detector (seqdet_kernels.h: kMaxM)
SEQDET_MAX_STATES = 1024   # trellis states M ** (taps - 1) (kMaxStates)
SEQDET_MAX_TAPS = 11       # (kMaxTaps)
SEQDET_MAX_COLS = 64       # (kMaxCols)
SEQDET_SURV_CHUNK = 32     # T: steps per survivor chunk (kSurvChunk)
SEQDET_STAGE_CHUNK = 256   # C: samples of y staged at a time (kStageChunk)
SEQDET_MAX_SURVIVOR_BYTES = 1 << 31
SEQDET_KERNELS = ("forward_wave64", "forward_multiwave")                                     # ssf_mlse_params.kernel
SEQDET_RULES = {"ML": 0, "MAP": 1}                                                           # ssf_detector_rule
SEQDET_DET_BLOCK = 256     # detector: symbols per workgroup (kDetBlock)
SEQDET_AC_MAX_TAPS = 256   # autocorr (kAcMaxTaps)
SEQDET_AC_TILE = 4096      # samples per tile of autocorr (kAcTile)


class SyncTileParams(C.Structure):
    """ssf_sync_tile_params (include/ssf.h)."""
    _fields_ = [("n_rx", C.c_int64), ("n_tx", C.c_int64), ("n_pad", C.c_int64), ("nModes", C.c_int32), ("SpS", C.c_int32),
                ("rx_dtype", C.c_int32), ("tx_dtype", C.c_int32)]


SYNCDATA_BLOCK = 256       # lanes per workgroup of the syncDataSequences / movingAverage / bert kernels (syncdata_kernels.h: kBlock)
SYNCDATA_SPAN = 1024       # B: rows of a column one workgroup of the extraction scans (kSpan)
SYNCDATA_MA_TILE = 1024    # T: outputs of a column per workgroup of the windowed mean (kMaTile)
SYNCDATA_MA_MAX_N = 2048   # longest window (kMaMaxN)
SYNCDATA_BERT_BLOCKS = 1024                                                                  # most workgroups of bert's passes


def siso_slots(ncoef):
    """Coefficient slots per lane the serial kernel is compiled for (siso_kernels.h: slots_for)."""
    r = (ncoef + 63) // 64
    return next(v for v in (1, 2, 4, 8, 16, 24) if r <= v)


MOD_KINDS = {"pm": 0, "mzm": 1, "iqm": 2}                                                   # SSF_MOD_*
TX_BLOCK = 256             # lanes per workgroup of the IM/DD transmitter's and the AWGN channel's kernels (imddtx_kernels.h: kTxBlock)
TX_BLOCKS = 1024           # most workgroups of their reduction passes (kTxBlocks)
TX_EW_BLOCKS = 4096        # most workgroups of their element-wise passes: the grid-stride span is TX_EW_BLOCKS * TX_BLOCK elements
TX_MAX_TAPS = 4096         # pulse-shaping taps of one overlap-save launch (rx_pipeline.h: kMaxNfft / 2)

METRICS_DTYPES = {"complex128": 0, "complex64": 1, "float64": 2, "float32": 3}              # ssf_metrics_dtype
METRICS_BER, METRICS_GMI, METRICS_MI, METRICS_EVM, METRICS_EVM_BLIND = 1, 2, 4, 8, 16       # ssf_metrics_want


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("arch", C.c_char * 32), ("compute_units", C.c_int32),
                ("reserved", C.c_int32), ("total_mem_bytes", C.c_int64), ("lds_per_block_bytes", C.c_int64)]


# every symbol include/ssf.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "ssf_device_count": (C.c_int, []),
    "ssf_device_info": (C.c_int, [C.c_int, C.POINTER(DeviceInfo)]),
    "ssf_version": (C.c_char_p, []),
    "ssf_plan_create": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "ssf_plan_destroy": (C.c_int, [C.c_void_p]),
    "ssf_plan_set_units": (C.c_int, [C.c_void_p, C.c_int32]),
    "ssf_plan_pipeline": (C.c_int, [C.c_void_p]),
    "ssf_plan_set_lanes": (C.c_int, [C.c_void_p, C.c_int32]),
    "ssf_get_unit_stats": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Stats)]),
    "ssf_last_error": (C.c_char_p, [C.c_void_p]),
    "ssf_upload": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ssf_execute": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_int32, C.c_void_p,
                              C.POINTER(Stats), C.POINTER(Trace)]),
    "ssf_download": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ssf_download_snapshots": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ssf_set_snapshot_sink": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ssf_sync_snapshots": (C.c_int, [C.c_void_p]),
    "ssf_upload_aos": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ssf_download_aos": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "ssf_run": (C.c_int, [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.POINTER(Stats), C.POINTER(Trace)]),
    "ssf_mgpu_run": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                               C.c_int32, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "ssf_set_coupling": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_set_coupling_comm": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ssf_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "ssf_get_kernel_times": (C.c_int, [C.c_void_p, C.POINTER(KernelTimes)]),
    "ssf_overlap_save": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "ssf_device_malloc": (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_void_p)]),
    "ssf_device_free": (C.c_int, [C.c_int, C.c_void_p]),
    "ssf_device_memcpy": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    "ssf_fir_filter": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_couple_reduce_selftest": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ssf_device_axpy": (C.c_int, [C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]),
    "ssf_fir_long": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ssf_delay_signal": (C.c_int, [C.c_int, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "ssf_edfa": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_pbs": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_optical_hybrid_2x4": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_nlin_phase_rot": (C.c_int, [C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_convergence_condition": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_double)]),
    "ssf_decimate": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_int32)]),
    "ssf_rx_run": (C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_int32, C.POINTER(RxParams), C.c_void_p, C.c_void_p,
                             C.POINTER(C.c_double), C.c_void_p]),
    "ssf_rx_chain": (C.c_int, [C.c_int, C.c_int64, C.POINTER(RxParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                               C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "ssf_wdm_tx": (C.c_int, [C.c_int, C.POINTER(TxParams), C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_pam_tx": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                             C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "ssf_modulate_optical": (C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "ssf_awgn": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p,
                           C.c_void_p, C.c_int64, C.c_void_p]),
    "ssf_upsample": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "ssf_metrics": (C.c_int, [C.c_int, C.POINTER(MetricsParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(MetricsResult)]),
    "ssf_pnorm": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "ssf_signal_power": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_demodulate": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "ssf_theory_mi": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.POINTER(C.c_double)]),
    "ssf_calc_mi": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_cpr": (C.c_int, [C.c_int, C.POINTER(CprParams), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p,
                          C.POINTER(C.c_double)]),
    "ssf_bps": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_void_p,
                          C.c_void_p]),
    "ssf_foe": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                          C.POINTER(C.c_double)]),
    "ssf_symbol_sync": (C.c_int, [C.c_int, C.POINTER(SyncParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SyncResult)]),
    "ssf_finddelay": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "ssf_sync_transform_time": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "ssf_mimo_eq": (C.c_int, [C.c_int, C.POINTER(EqParams), C.POINTER(EqStage), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_siso_eq": (C.c_int, [C.c_int, C.POINTER(SisoParams), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p]),
    "ssf_mlse": (C.c_int, [C.c_int, C.POINTER(MlseParams), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                           C.POINTER(C.c_double)]),
    "ssf_detector": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_autocorr": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_sync_tile": (C.c_int, [C.c_int, C.POINTER(SyncTileParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_sync_extract": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int64)]),
    "ssf_real_part": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "ssf_copy_columns": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ssf_moving_average": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ssf_bert": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_calc_llr": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                               C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "ssf_ldpc_graph_create": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "ssf_ldpc_graph_destroy": (C.c_int, [C.c_void_p]),
    "ssf_ldpc_decode": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(LdpcParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "ssf_ldpc_encoder_create": (C.c_int, [C.c_int, C.POINTER(EncoderDesc), C.c_void_p, C.c_void_p, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "ssf_ldpc_encoder_destroy": (C.c_int, [C.c_void_p]),
    "ssf_ldpc_encode": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(EncodeParams), C.c_void_p, C.c_void_p]),
    "ssf_modulate": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.c_void_p, C.c_void_p]),
    "ssf_ofdm_modulate": (C.c_int, [C.c_int, C.POINTER(OfdmParams), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "ssf_ofdm_demodulate": (C.c_int, [C.c_int, C.POINTER(OfdmParams), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_pert_nlin": (C.c_int, [C.c_int, C.POINTER(NlinParams), C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_clock_interp": (C.c_int, [C.c_int, C.POINTER(ClockParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_quantize": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int64, C.c_void_p, C.c_void_p]),
    "ssf_clip": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "ssf_minmax": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_clock_scale_add": (C.c_int, [C.c_int, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_gardner": (C.c_int, [C.c_int, C.POINTER(GardnerParams), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "ssf_clock_drift": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]),
    "ssf_array_copy": (C.c_int, [C.c_int, C.POINTER(ArrayDesc), C.c_void_p, C.POINTER(ArrayDesc), C.c_void_p]),
    "ssf_array_take": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_array_transpose": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "ssf_array_fill": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "ssf_array_binary": (C.c_int, [C.c_int, C.POINTER(ArrayBinaryParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ssf_array_unary": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "ssf_array_reduce": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64)]),
    "ssf_freq_shift": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "ssf_device_copy_bandwidth": (C.c_int, [C.c_int, C.c_int64, C.c_int32, C.POINTER(C.c_double)]),
    "ssf_linear_channel": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.c_void_p, C.c_void_p]),
    "ssf_comm_get_id": (C.c_int, [C.c_void_p]),
    "ssf_comm_create": (C.c_int, [C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "ssf_comm_destroy": (C.c_int, [C.c_void_p]),
    "ssf_comm_rank": (C.c_int, [C.c_void_p]),
    "ssf_comm_size": (C.c_int, [C.c_void_p]),
    "ssf_comm_barrier": (C.c_int, [C.c_void_p]),
    "ssf_comm_allreduce": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int32]),
    "ssf_comm_bcast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ssf_comm_send": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ssf_comm_recv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    "ssf_comm_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "ssf_comm_last_error": (C.c_char_p, [C.c_void_p]),
}
COMM_ID_BYTES = 128
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.c_int32)     # ssf_reduce_fn

_lib = None


def load():
    """Load libssf_hip.so and bind every ABI symbol.  Raises RuntimeError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"HIP extension not built: {LIB_PATH} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C opticommpy_amd/csrc`. "
            "opticommpy_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)        # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def error_message(lib, handle, rc):
    msg = lib.ssf_last_error(handle)
    msg = msg.decode(errors="replace") if msg else ""
    return f"{STATUS.get(rc, rc)}: {msg}" if msg else str(STATUS.get(rc, rc))


def raise_for(lib, handle, rc):
    if rc == 0:
        return
    text = error_message(lib, handle, rc)
    if rc == -1:
        raise ValueError(text)
    if rc == -3:
        raise MemoryError(text)
    raise RuntimeError(text)
