"""The case table of tests/test_gpu_tx_shapes.py, shared with tests/test_tx_shapes_emu.py (which runs the rows marked for it through
the g++ emulator): simpleWDMTx (ssf_wdm_tx) at the block lengths, block edges, tap counts, stuffing factors, grids, alphabets and
phase walks at which opticommpy_amd/csrc/rx_pipeline.h (RxCore::wdm_tx), the zero-stuffed loads of fused_kernels.h (OlsArgs::in_up)
and the device walk of rx_kernels.h (pn_body) take another path, judged against oracle/tx_oracle.py.

Three kinds of row.  "seeded": param.seed is set, the oracle is used as it is.  "device_pn": no param.seed and a linewidth, so the
product generates the laser's walk on the device from a fixed key; the oracle runs with its module-level phaseNoise replaced by the
walk RESTATED here (device_walk: Philox4x32-10 and Box-Muller in numpy, extended precision, rounded once), one call per channel,
and np.random seeded globally with the same literal in front of the oracle and in front of the product, so that both draw the same
symbols.  "abi": ssf_wdm_tx / emu_wdm_tx called directly with the arrays simpleWDMTx would pass and a host phase array of phi_rows
rows, the oracle running with that row per channel; the refusals among them must return their error code without a launch.

The geometry restated here.  A K-tap pulse (K = len(pulseShape)) runs in blocks of fir_nfft(K) points (256 up to 32 taps, 512 up to
64, 1024 up to 128, 2048 up to 682, 4096 up to 2048, 8192 up to 4096, more taps are refused) that advance by d = nfft - K + 1;
numBlocks = ceil((N + K - 1) / d), N = nSymbols * SpS.  The device walk works in chunks of 4096 samples (kPnChunk), 16 consecutive
samples per lane, the chunks' sums scanned on the host.  Every row holds what its `claims` say (check_conditions).  No row has
N < K: the reference's firFilter ('same' relative to the signal) cannot form it.

Bounds: symbols, wdmFreqGrid and pmf bit for bit; the field max |got - want| <= 1e-12 max |want|, the bound of tests/test_gpu_tx.py
and tests/test_emu_tx.py, for every row.  A device-walk row keeps it because its linewidth is chosen (and asserted) such that
N * 32 * 2^-53 * sigma <= 1e-13: N increments of a few double roundings of sigma * g each, |g| <= 6.7."""
import collections
import contextlib
import functools
import math

import numpy as np

import opticommpy_amd as oa
from helpers import make_param
from opticommpy_amd import _lib
from oracle import tx_oracle as otx
from oracle.ssf_oracle import parameters as oparams

Row = collections.namedtuple("Row", "id kw kind emu raises claims x")
# kw: simpleWDMTx's keywords as sorted (name, value) pairs; kind: "seeded", "device_pn" or "abi"; raises: None, or the refusal the row
# must end in ("bad_arg", "unsupported": the test files pin the exception type / error code per backend); claims: what the row's
# name says, as sorted (name, value) pairs, asserted by check_conditions; x: the kind's own parameters (key, np_seed, phi_rows ...)

TOL = 1e-12
WALK_BUDGET = 1e-13             # N * 32 * 2^-53 * sigma of a device-walk row
RS = 32e9
K_PN_CHUNK, PN_PER_LANE = 4096, 16
ERR_CODE = {"bad_arg": -1, "unsupported": -6}                       # include/ssf.h: SSF_ERR_BAD_ARG, SSF_ERR_UNSUPPORTED


def _freeze(d):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in d.items()))


def _bits(M):
    return int(math.log2(M))


def _row(id, kind="seeded", raises=None, claims=None, x=None, nSymbols=None, **kw):
    kw.setdefault("M", 4)
    kw.setdefault("prgsBar", False)
    kw["nBits"] = nSymbols * _bits(kw["M"])
    return Row(id, _freeze(kw), kind, True, raises, _freeze(claims or {}), _freeze(x or {}))


def keywords(row):
    return {k: list(v) if isinstance(v, tuple) else v for k, v in row.kw}


def fir_nfft(K):
    """rx_pipeline.h: fir_nfft, restated."""
    nfft = 256
    while nfft < 8 * K and nfft < 2048:
        nfft *= 2
    while nfft < 3 * K and nfft < 4096:
        nfft *= 2
    while nfft < 2 * K and nfft < 8192:
        nfft *= 2
    while nfft < K:
        nfft *= 2
    return nfft


def n_taps(kw):
    """K of a keyword set without evaluating the pulse (pulseShape: 'rect', 'nrz', 'rrc', 'rc')."""
    SpS, kind = kw.get("SpS", 16), kw.get("pulseType", "rrc")
    return SpS + 2 * (SpS // 2) if kind == "rect" else 2 * SpS - 1 if kind == "nrz" else kw.get("nFilterTaps", 1024)


def geometry(kw):
    """-> (N, K, nfft, d, numBlocks)"""
    N = kw["nBits"] // _bits(kw["M"]) * kw.get("SpS", 16)
    K = n_taps(kw)
    nfft = fir_nfft(K)
    d = nfft - K + 1
    return N, K, nfft, d, -(-(N + K - 1) // d)


def sample_rate(kw):
    return 1 / ((1 / kw.get("Rs", RS)) / kw.get("SpS", 16))          # (as tx.py:106 rounds it)


def walk_sigma(kw):
    return float(np.sqrt(2 * np.pi * kw["laserLinewidth"] / sample_rate(kw)))


# ------------------------------------------------------------------------------------------------------- the walk, restated
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of 32-bit words held in uint64 -> four arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & _M32, np.uint64(k1) & _M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def device_walk(N, sigma, key, channel):
    """The device-generated laser phase walk of a channel, restated: counter (k >> 1, channel, 0x504E), key = the 64-bit seed, Box-Muller
    on words 0 and 1, the cosine branch for even k and the sine branch for odd k, phi[0] = 0, phi[k] = phi[k - 1] + sigma g_k -- in
    extended precision, rounded to double once."""
    L = np.longdouble
    k = np.arange(N, dtype=np.uint64)
    ctr = k >> np.uint64(1)
    v0, v1, _, _ = philox4x32_10(ctr & _M32, ctr >> np.uint64(32), np.uint64(channel), np.uint64(0x504E), int(key) & 0xFFFFFFFF, int(key) >> 32)
    u1, u2 = (v0.astype(L) + L(0.5)) / L(2 ** 32), (v1.astype(L) + L(0.5)) / L(2 ** 32)
    two_pi = 2 * (4 * np.arctan(L(1)))
    rad = np.sqrt(-2 * np.log(u1))
    g = np.where(k & np.uint64(1), rad * np.sin(two_pi * u2), rad * np.cos(two_pi * u2))
    inc = L(sigma) * g
    inc[0] = 0
    return np.cumsum(inc).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the table
def _edge(lo, hi, SpS, rem, blocks):
    """(nSymbols, nFilterTaps) with lo <= K <= hi (one class of fir_nfft) and N + K - 1 = blocks * d + rem, N = nSymbols * SpS >= K:
    the first found from the longest filter down."""
    for K in range(hi, lo - 1, -1):
        d = fir_nfft(K) - K + 1
        N = blocks * d + rem - K + 1
        if N >= K and N % SpS == 0:
            return N // SpS, K
    raise AssertionError((lo, hi, SpS, rem, blocks))


def _pn_linewidth(N, SpS, frac=0.5):
    """a linewidth whose sigma spends `frac` of the walk's error budget at N samples, at most 0.05 rad per step"""
    sigma = min(0.05, frac * WALK_BUDGET / (N * 32 * 2.0 ** -53))
    return sigma ** 2 * RS * SpS / (2 * np.pi)


def _rows():
    rows = []
    # 1. block lengths: the tap counts on either side of every threshold of fir_nfft, two blocks and a few samples each
    for i, (K, nfft) in enumerate(((32, 256), (33, 512), (64, 512), (65, 1024), (128, 1024), (129, 2048), (682, 2048), (683, 4096),
                                   (2048, 4096), (2049, 8192), (4096, 8192))):
        SpS = (2, 3, 4)[i % 3]
        nS = -(-(2 * (nfft - K + 1) + 5) // SpS)
        rows.append(_row(f"taps{K}-nfft{nfft}-sps{SpS}-n{nS * SpS}", seed=100 + i, nSymbols=nS, SpS=SpS, nFilterTaps=K, nChannels=1 + i % 2,
                         nPolModes=1 + (i // 2) % 2, M=16, claims=dict(K=K, nfft=nfft)))
    rows.append(_row("taps4097-refused", raises="unsupported", seed=120, nSymbols=2100, SpS=2, nFilterTaps=4097, nChannels=1, claims=dict(K=4097)))
    # 2. block edges on the stuffed path: (N + K - 1) mod d = d - 1, 0, 1 in the 256-, 2048- and 8192-point classes
    for i, (lo, hi, nfft, SpS, blocks) in enumerate(((2, 32, 256, 3, 9), (129, 682, 2048, 5, 3), (2049, 4096, 8192, 2, 2))):
        for j, rem in enumerate((-1, 0, 1)):
            nS, K = _edge(lo, hi, SpS, rem, blocks)
            rows.append(_row(f"edge-nfft{nfft}-rem{rem}-k{K}-sps{SpS}-n{nS * SpS}", seed=130 + 3 * i + j, nSymbols=nS, SpS=SpS, nFilterTaps=K,
                             nChannels=2, claims=dict(nfft=nfft, rem=rem, blocks=blocks + (rem == 1), K=K)))
    nS, K = _edge(2, 32, 5, 0, 1)
    rows.append(_row(f"edge-one-full-block-k{K}-sps5-n{nS * 5}", seed=140, nSymbols=nS, SpS=5, nFilterTaps=K, nChannels=1, claims=dict(nfft=256, rem=0, blocks=1)))
    nS, K = _edge(33, 64, 3, 1, 1)
    rows.append(_row(f"edge-one-sample-into-block-two-k{K}-sps3-n{nS * 3}", seed=141, nSymbols=nS, SpS=3, nFilterTaps=K, nChannels=1,
                     claims=dict(nfft=512, rem=1, blocks=2)))
    # 3. the smallest shapes
    rows.append(_row("n1-rect-sps1", seed=150, nSymbols=1, SpS=1, pulseType="rect", nChannels=1, claims=dict(N=1, K=1)))
    rows.append(_row("n2-2ch-2pol", seed=151, nSymbols=1, SpS=2, nFilterTaps=2, nChannels=2, nPolModes=2, claims=dict(N=2, K=2)))
    rows.append(_row("taps1-rrc-sps4-n64", seed=152, nSymbols=16, SpS=4, nFilterTaps=1, nChannels=1, claims=dict(K=1, N=64)))
    rows.append(_row("n33-equals-taps33", seed=153, nSymbols=11, SpS=3, nFilterTaps=33, nChannels=2, claims=dict(N=33, K=33)))
    rows.append(_row("n32-equals-taps32", seed=154, nSymbols=16, SpS=2, nFilterTaps=32, nChannels=2, claims=dict(N=32, K=32)))
    # 4. stuffing: SpS 1, 2, 3, 5, 16, 17 and the four pulse shapes
    rows.append(_row("sps1-rrc-taps65-n700", seed=160, nSymbols=700, SpS=1, nFilterTaps=65, nChannels=1, M=16, claims=dict(K=65)))
    rows.append(_row("sps2-rc-taps64-n1400", seed=161, nSymbols=700, SpS=2, pulseType="rc", pulseRollOff=0.5, nFilterTaps=64, nChannels=1, M=16))
    rows.append(_row("sps3-rect-n1500", seed=162, nSymbols=500, SpS=3, pulseType="rect", nChannels=2, claims=dict(K=5)))
    rows.append(_row("sps5-rect-n1500", seed=163, nSymbols=300, SpS=5, pulseType="rect", nChannels=1, nPolModes=2, claims=dict(K=9)))
    rows.append(_row("sps3-rc-taps100-n1500", seed=164, nSymbols=500, SpS=3, pulseType="rc", pulseRollOff=0.25, nFilterTaps=100, nChannels=1))
    rows.append(_row("sps16-rrc-taps257-n4096", seed=165, nSymbols=256, SpS=16, nFilterTaps=257, pulseRollOff=0.1, nChannels=2, M=16))
    rows.append(_row("sps17-nrz-n4097", seed=166, nSymbols=241, SpS=17, pulseType="nrz", nChannels=1, claims=dict(K=33, N=4097)))
    rows.append(_row("sps16-nrz-n2048", seed=167, nSymbols=128, SpS=16, pulseType="nrz", nChannels=2, claims=dict(K=31)))
    # 5. grid and powers
    for nCh in (1, 2, 3, 4, 5):
        rows.append(_row(f"grid-{nCh}ch-n1024", seed=170 + nCh, nSymbols=128, SpS=8, nFilterTaps=128, nChannels=nCh, M=16, wdmGridSpacing=37.5e9))
    rows.append(_row("grid-far-3ch-n8192", seed=176, nSymbols=2048, SpS=4, nFilterTaps=64, nChannels=3, wdmGridSpacing=40 * 4 * RS, claims=dict(arg=1e6)))
    rows.append(_row("powers-40dB-3ch-n2048", seed=177, nSymbols=256, SpS=8, nFilterTaps=128, nChannels=3, powerPerChannel=[-30, 10, -10], claims=dict(span_db=40)))
    rows.append(_row("powers-weak-alone-n2048", seed=177, nSymbols=256, SpS=8, nFilterTaps=128, nChannels=1, powerPerChannel=[-30]))
    # 6. modes and alphabets
    for nPol in (1, 2, 3):
        rows.append(_row(f"modes-{nPol}pol-n1024", seed=180 + nPol, nSymbols=128, SpS=8, nFilterTaps=96, nChannels=2, nPolModes=nPol, M=16))
    for i, (M, ct) in enumerate(((4, "pam"), (8, "psk"), (4, "qam"), (64, "qam"), (256, "qam"))):
        rows.append(_row(f"alphabet-{ct}{M}-n1000", seed=185 + i, nSymbols=250, SpS=4, nFilterTaps=40, nChannels=2, M=M, constType=ct))
    rows.append(_row("alphabet-qam64-maxwell-boltzmann-n1000", seed=190, nSymbols=250, SpS=4, nFilterTaps=40, nChannels=2, nPolModes=2, M=64,
                     probDist="maxwell-boltzmann", shapingFactor=0.05))
    for i, scale in enumerate((0.05, 1.0)):
        rows.append(_row(f"mzm-{scale}-n1000", seed=191 + i, nSymbols=250, SpS=4, nFilterTaps=40, nChannels=2, M=16, mzmScale=scale))
    # 7. the seeded walk: host draws, one row uploaded
    for i, (nCh, nPol) in enumerate(((1, 1), (3, 1), (1, 2), (3, 2))):
        rows.append(_row(f"walk-seeded-100kHz-{nCh}ch-{nPol}pol-n2048", seed=200 + i, nSymbols=256, SpS=8, nFilterTaps=64, nChannels=nCh, nPolModes=nPol,
                         M=16, laserLinewidth=100e3))
    rows.append(_row("walk-seeded-beyond-1e3rad-3ch-2pol-n2048", seed=205, nSymbols=256, SpS=8, nFilterTaps=64, nChannels=3, nPolModes=2, M=16,
                     laserLinewidth=400 * 8 * RS, claims=dict(phi_max=1e3)))
    rows.append(_row("walk-seeded-linewidth0-2ch-n2048", seed=206, nSymbols=256, SpS=8, nFilterTaps=64, nChannels=2, M=16, laserLinewidth=0))
    # 8. one grid round of the 256 x 256 reductions
    for i, N in enumerate((65535, 65536, 65537)):
        rows.append(_row(f"reduce-n{N}", seed=210 + i, nSymbols=N, SpS=1, pulseType="rect", nChannels=1, claims=dict(N=N)))
    # 9. the device walk: lane, chunk and multi-chunk borders; channels; polarisations; keys
    # (N, SpS, channels, polarisations, chunks, lanes at work in the last chunk)
    for i, (N, SpS, nCh, nPol, chunks, lanes) in enumerate(((1, 1, 1, 1, 1, 1), (2, 1, 2, 1, 1, 1), (16, 2, 1, 1, 1, 1), (17, 1, 3, 1, 1, 2), (65, 1, 1, 1, 1, 5),
                                                            (4095, 3, 2, 1, 1, 256), (4096, 4, 1, 2, 1, 256), (4097, 1, 2, 2, 2, 1), (8193, 3, 3, 1, 3, 1),
                                                            (12289, 1, 2, 2, 4, 1))):
        shape = dict(pulseType="rect") if SpS == 1 else dict(nFilterTaps=SpS * 4 - 1)
        rows.append(_row(f"walk-device-n{N}-{nCh}ch-{nPol}pol", kind="device_pn", nSymbols=N // SpS, SpS=SpS, nChannels=nCh, nPolModes=nPol, M=16,
                         laserLinewidth=_pn_linewidth(N, SpS), x=dict(key=0x5EED0000 + i, np_seed=300 + i),
                         claims=dict(N=N, chunks=chunks, lanes=lanes), **shape))
    for i, key in enumerate((0x0123456789ABCDEF, 0x0123456689ABCDEF)):                     # (the second differs in the key's high word only)
        rows.append(_row(f"walk-device-key{i}-n4100", kind="device_pn", nSymbols=1025, SpS=4, nFilterTaps=16, nChannels=2, laserLinewidth=_pn_linewidth(4100, 4),
                         x=dict(key=key, np_seed=320), claims=dict(chunks=2)))
    # 10. the C ABI: host phase of nChannels rows, of one row, and the refusals
    abi = dict(nSymbols=300, SpS=4, nFilterTaps=33, nChannels=3, nPolModes=2, M=16)
    rows.append(_row("abi-phi-3rows-phi_rows3", kind="abi", x=dict(np_seed=400, rows=3, phi_rows=3), **abi))
    rows.append(_row("abi-phi-3rows-phi_rows0", kind="abi", x=dict(np_seed=401, rows=3, phi_rows=0), **abi))
    rows.append(_row("abi-phi-1row-phi_rows1", kind="abi", x=dict(np_seed=402, rows=1, phi_rows=1), **abi))
    rows.append(_row("abi-no-phi", kind="abi", x=dict(np_seed=403, rows=0, phi_rows=0), **abi))
    for i, (name, field, value, code) in enumerate((("phi_rows2-of-3ch", "phi_rows", 2, "bad_arg"), ("nSymbols0", "nSymbols", 0, "bad_arg"),
                                                    ("SpS0", "SpS", 0, "bad_arg"), ("ntaps0", "ntaps", 0, "bad_arg"), ("Fs0", "Fs", 0.0, "bad_arg"),
                                                    ("ntaps4097", "ntaps", 4097, "unsupported"))):
        rows.append(_row(f"abi-refused-{name}", kind="abi", raises=code, x=dict(np_seed=410 + i, rows=3, phi_rows=3, field=field, value=value), **abi))
    # in one process the rows run in table order: large, small, large ... (workspace and filter-cache reuse)
    rows.sort(key=lambda r: (geometry(keywords(r))[0], r.id))
    half = (len(rows) + 1) // 2
    small, large = rows[:half], rows[half:][::-1]
    return [r for pair in zip(large + [None] * (half - len(large)), small) for r in pair if r is not None]


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
EMU_ROWS = [r for r in ROWS if r.emu]


# --------------------------------------------------------------------------------------------------------------- the oracle
@contextlib.contextmanager
def oracle_walks(walks):
    """oracle.tx_oracle.phaseNoise replaced: call c returns walks[c] (one call per channel, at indMode == 0) and draws nothing."""
    pending, real = list(walks), otx.phaseNoise

    def replay(lw, Nsamples, Ts, seed=None):
        w = pending.pop(0)
        assert len(w) == Nsamples, (len(w), Nsamples)
        return w

    otx.phaseNoise = replay
    try:
        yield
        assert not pending, len(pending)
    finally:
        otx.phaseNoise = real


@functools.lru_cache(maxsize=None)
def walks(row):
    """The phase walk of every channel of a device_pn / abi row (None: no phase), and the host array an abi row passes."""
    kw, x = keywords(row), dict(row.x)
    N, nCh = geometry(kw)[0], kw["nChannels"]
    if row.kind == "device_pn":
        return [device_walk(N, walk_sigma(kw), x["key"], ch) for ch in range(nCh)], None
    if not x["rows"]:
        return [np.zeros(N)] * nCh, None
    rng = np.random.default_rng(x["np_seed"])
    phi = np.ascontiguousarray(np.cumsum(rng.normal(size=(x["rows"], N)) * 0.05, axis=1))
    phi.setflags(write=False)
    return [phi[ch if x["rows"] > 1 else 0] for ch in range(nCh)], phi


Expected = collections.namedtuple("Expected", "sig symb grid pmf")


@functools.lru_cache(maxsize=None)
def expected(row):
    """The oracle's (field, symbols, wdmFreqGrid, pmf) of a row, computed once per process; for a refused abi row the inputs' source."""
    kw = keywords(row)
    if row.kind == "seeded":
        if row.raises:
            return None
        sig, symb, par = otx.simpleWDMTx(make_param(oparams, kw))
    else:
        with oracle_walks(walks(row)[0]):
            np.random.seed(dict(row.x)["np_seed"])
            sig, symb, par = otx.simpleWDMTx(make_param(oparams, kw))
    for a in (sig, symb):
        a.setflags(write=False)
    return Expected(sig, symb, par.wdmFreqGrid, par.pmf)


# ---------------------------------------------------------------------------------------------------------------- the calls
Got = collections.namedtuple("Got", "sig symb grid pmf")


def _refuse_host_walk(*a, **k):
    raise AssertionError("host phase-noise draw in a device-walk row")


def abi_arguments(row):
    """What simpleWDMTx would pass to ssf_wdm_tx for the row's keywords (wdm_tx.py), the phase array and phi_rows the row's own."""
    kw, x, want = keywords(row), dict(row.x), expected(row)
    N, K = geometry(kw)[:2]
    nCh, nPol = kw["nChannels"], kw.get("nPolModes", 1)
    pp = oa.parameters()
    pp.pulseType, pp.nFilterTaps, pp.rollOff, pp.SpS = kw.get("pulseType", "rrc"), kw.get("nFilterTaps", 1024), kw.get("pulseRollOff", 0.01), kw["SpS"]
    taps = np.zeros(max(K, 4097))                                                        # (room for the tap count a refusal row claims)
    taps[:K] = oa.pulseShape(pp)
    p = _lib.TxParams(Fs=sample_rate(kw), mzmScale=float(kw.get("mzmScale", 0.5)), nSymbols=N // kw["SpS"], SpS=kw["SpS"], nChannels=nCh, nPolModes=nPol,
                      ntaps=K, phi_rows=x["phi_rows"])
    if "field" in x:
        setattr(p, x["field"], x["value"])
    symbols = np.ascontiguousarray(np.transpose(want.symb, (2, 1, 0)))
    Pch = 10 ** (kw.get("powerPerChannel", -3) / 10) * 1e-3 * np.ones(nCh)
    return p, symbols, taps, walks(row)[1], np.sqrt(Pch / nPol), np.ascontiguousarray(want.grid, dtype=np.float64)


def call(row, api, device_output=False):
    """The row's call on `api`: simpleWDMTx (the package's, with its backend as the test file set it) and wdm_tx(p, symbols, taps, phi,
    amp, deltaF, out, power) -> the C ABI's return code, out a numpy array or a DeviceArray.  -> Got; an abi row that is refused
    returns its code in place of the field, having checked that nothing was written."""
    from opticommpy_amd import models, wdm_tx
    kw, x = keywords(row), dict(row.x)
    if row.kind == "abi":
        p, symbols, taps, phi, amp, deltaF = abi_arguments(row)
        N, nPol = geometry(kw)[0], p.nPolModes
        out = api.empty(device_output, (N, nPol))
        if not device_output:
            out.fill(np.nan)
        power = np.full(p.nChannels * nPol, np.nan)
        rc = api.wdm_tx(p, symbols, taps, phi, amp, deltaF, out, power)
        if row.raises:
            assert np.isnan(out).all() and np.isnan(power).all(), row.id
            return rc
        assert rc == 0, (row.id, rc)
        assert np.array_equal(power, np.repeat(amp * amp, nPol)), row.id
        return Got(out, None, None, None)
    if row.kind == "seeded":
        sig, symb, par = api.simpleWDMTx(make_param(oa.parameters, kw), device_output=device_output)
        return Got(sig, symb, par.wdmFreqGrid, par.pmf)
    real_seed, real_walk = models._device_seed, wdm_tx.phaseNoise
    models._device_seed, wdm_tx.phaseNoise = (lambda seed: x["key"]), _refuse_host_walk
    try:
        np.random.seed(x["np_seed"])
        sig, symb, par = api.simpleWDMTx(make_param(oa.parameters, kw), device_output=device_output)
    finally:
        models._device_seed, wdm_tx.phaseNoise = real_seed, real_walk
    return Got(sig, symb, par.wdmFreqGrid, par.pmf)


# ----------------------------------------------------------------------------------------------------------- the conditions
def check_conditions(row):
    """The row selects the path it is named for, and its bound is the one the docstring derives."""
    from opticommpy_amd import models
    kw, x, claims = keywords(row), dict(row.x), dict(row.claims)
    N, K, nfft, d, blocks = geometry(kw)
    assert N >= K >= 1, (row.id, N, K)
    if K <= 4096:
        pp = oa.parameters()
        pp.pulseType, pp.nFilterTaps, pp.rollOff, pp.SpS = kw.get("pulseType", "rrc"), kw.get("nFilterTaps", 1024), kw.get("pulseRollOff", 0.01), kw["SpS"]
        assert len(oa.pulseShape(pp)) == K, (row.id, K)
        assert models._ols_block(K) == nfft and nfft in (256, 512, 1024, 2048, 4096, 8192), (row.id, nfft)
    else:
        assert row.raises == "unsupported", row.id
    for name, have in (("N", N), ("K", K), ("nfft", nfft), ("blocks", blocks)):
        if name in claims:
            assert have == claims[name], (row.id, name, have)
    if "rem" in claims:
        assert (N + K - 1) % d == claims["rem"] % d and kw["SpS"] > 1, (row.id, (N + K - 1) % d, d)
    if "arg" in claims:
        grid = np.arange(-(kw["nChannels"] // 2), kw["nChannels"] // 2 + 1) * kw["wdmGridSpacing"]
        assert N <= 8192 and 2 * np.pi * np.max(np.abs(grid)) * (N - 1) / sample_rate(kw) >= claims["arg"], row.id
    if "span_db" in claims:
        assert max(kw["powerPerChannel"]) - min(kw["powerPerChannel"]) >= claims["span_db"], row.id
    if "phi_max" in claims:
        assert np.max(np.abs(otx.phaseNoise(kw["laserLinewidth"], N, 1 / sample_rate(kw), seed=kw["seed"]))) > claims["phi_max"], row.id
    if row.kind == "seeded":
        assert isinstance(kw["seed"], int), row.id
    else:
        assert "seed" not in kw and isinstance(x["np_seed"], int), row.id
    if row.kind == "device_pn":
        sigma = walk_sigma(kw)
        assert sigma > 0 and N * 32 * 2.0 ** -53 * sigma <= WALK_BUDGET, (row.id, sigma)
        assert -(-N // K_PN_CHUNK) == claims["chunks"] and 0 < x["key"] < 2 ** 64, row.id
        if "lanes" in claims:
            assert -(-((N - 1) % K_PN_CHUNK + 1) // PN_PER_LANE) == claims["lanes"], row.id
        w = walks(row)[0]
        assert all(np.max(np.abs(a - b)) > 1e-6 for i, a in enumerate(w) for b in w[:i]) or N == 1, row.id     # a walk per channel
    if row.kind == "abi":
        nCh = kw["nChannels"]
        assert x["rows"] in (0, 1, nCh) and (row.raises is not None) == ("field" in x), row.id
        if x["rows"] > 1:
            w = walks(row)[0]
            assert all(np.max(np.abs(a - b)) > 1e-3 for i, a in enumerate(w) for b in w[:i]), row.id
        if x.get("field") == "phi_rows":
            assert x["value"] not in (0, 1, nCh), row.id


def compare(row, got, label=""):
    """-> the field's distance in units of the largest expected sample"""
    want, tag = expected(row), f"{label} {row.id}"
    if row.kind != "abi":
        assert np.array_equal(got.symb, want.symb), tag
        assert np.array_equal(got.grid, want.grid) and np.array_equal(got.pmf, want.pmf), tag
    assert type(got.sig) is np.ndarray and got.sig.shape == want.sig.shape and got.sig.dtype == want.sig.dtype, (tag, got.sig.shape, got.sig.dtype)
    err, scale = np.max(np.abs(got.sig - want.sig)), np.max(np.abs(want.sig))
    print(f"[tx-shapes] {tag}: {err / scale:.2e}")
    assert err <= TOL * scale, (tag, err, scale)
    return err / scale
