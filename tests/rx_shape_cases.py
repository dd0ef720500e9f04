"""The case table of tests/test_gpu_rx_shapes.py, shared with tests/test_rx_shapes_emu.py (which runs the rows marked for it through
the g++ emulator): seeded inputs at the sizes and parameters at which the host code of opticommpy_amd/csrc/rx_pipeline.h takes
another path, judged against tests/rx_restatement.py (filters, delays, decimate) and oracle/rx_oracle.py (the receiver models).

The geometry restated here.  Overlap-save (fused_kernels.h: ols_launch): a K-tap filter runs in blocks of fir_nfft(K) points (256,
512, 1024 or 2048 up to 682 taps, 4096 up to 2048, 8192 above) that advance by d = nfft - K + 1; a thread holds 16 points, an even
column count up to 4096 points takes C = 2 columns side by side, a workgroup has max(256, C nfft / 16) threads = gpw block groups.
Filters of more than 4096 taps run segment by segment (fir_long).  decimate: nclass = SpSin * columns <= 256 classes, nthreads =
256 // nclass * nclass, one workgroup per 4 * nthreads elements, at most 512.  The receiver (run_coherent): polarisation-delay
filters [detection in their stores when nothing but element-wise work follows], low-pass filter or element-wise detection [IQ
imbalance in its stores when no skew follows], skew filters (one launch, or one per polarisation when their zero paddings
differ); iqMixing alone is its skew filter or one element-wise pass.  The chain (RxCore::chain) fuses decimate's statistics into
the matched filter's stores when that filter has a chain kernel (1024 ... 4096 points with two columns, 8192 with one) and
SpSin | nfft / 16, and decimate's gather into the compensating filter's loads when that filter has one.

Every row that takes a decimation decision must pass margin >= 1e-6 in the restatement (check_conditions), the two `tie` rows
aside: their variances are exact in double and the device must return the lowest tied phase."""
import collections
import functools
import math

import numpy as np

import rx_restatement as rr
from helpers import rel_l2, synth_field
from oracle import rx_oracle as orx
from oracle import ssf_oracle as orc
from sync_cases import MARGIN

Row = collections.namedtuple("Row", "id kind p seed emu launches raises")
# p: the kind's parameters as sorted (name, value) pairs; launches: kernel launches of the receiver plan the row selects, or of a
# filter of more than 4096 taps (None: not pinned); raises: the exception the call must end in

FS = 96e9                       # receiver rows
FS_FILT = 64e9                  # delaySignal rows
FIR_TOL, RX_TOL, CHAIN_TOL, F32_ATOL = 1e-13, 1e-12, 1e-11, 1e-6
DEVICE_ARGS = {"fir": ("x",), "delay": ("x",), "decimate": ("x",), "pdm": ("Es", "Elo", "un"), "coh": ("Es", "Elo", "un"),
               "iq": ("sig",), "pd": ("E", "un"), "bpd": ("E1", "E2"), "hybrid": ("Es", "Elo"), "chain": ("Es", "Elo")}


def _freeze(v):
    return tuple(sorted((k, _freeze(x)) for k, x in v.items())) if isinstance(v, dict) else v


def _row(id, kind, seed, emu=True, launches=None, raises=None, **p):
    return Row(id, kind, _freeze(p), seed, emu, launches, raises)


def params(row):
    return {k: dict(v) if isinstance(v, tuple) and k in ("fe", "pd") else v for k, v in row.p}


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


def ols_launch(nfft, ncols, numBlocks):
    """fused_kernels.h: ols_launch, restated -> (lg, C, gpw, jobs)."""
    lg = int(math.log2(nfft))
    lgk = lg if 8 <= lg <= 13 else 0
    C = 2 if lgk and lgk <= 12 and ncols % 2 == 0 else 1
    tpf = nfft // 16
    threads = max(256, C * tpf)
    return lgk, C, threads // (C * tpf), numBlocks * ncols // C


def num_blocks(N, K, nfft):
    return (N + K - 1 + nfft - K) // (nfft - K + 1)


def chain_kernel(lg, C):
    """rx_kernels.h: chain_ols_supported, restated."""
    return (10 <= lg <= 12 and C == 2) or (lg == 13 and C == 1)


def dec_launch(N, SpSin, cols):
    """RxCore::decimate's launch -> (nthreads, workgroups before the cap of 512)."""
    nclass = SpSin * cols
    nthreads = 256 // nclass * nclass
    return nthreads, max(1, -(-N * cols // (4 * nthreads)))


def _dec_N(SpSin, cols, above):
    per = 4 * dec_launch(SpSin, SpSin, cols)[0] // cols // SpSin
    return (per + 1 if above else per) * SpSin


def _dec_phases(SpSin, cols, turn):
    """a boosted phase per column: the first and the last among them, different between the columns while there are phases left"""
    order = [0, SpSin - 1] + [p for p in (SpSin // 2, 1, SpSin - 2, SpSin // 3, 2, SpSin - 3) if 0 < p < SpSin - 1]
    order = list(dict.fromkeys(order))
    return tuple(order[(c + turn) % len(order)] for c in range(cols))


# ------------------------------------------------------------------------------------------------------------------ the table
A = dict(polRotation=0.2, polDelay=2e-12)
IDEAL = dict(ideal=True)
BAND = dict(B=25e9, N=101, currentSaturation=True, IpdSat=6e-3)
FLAT = dict(B=25e9, bandwidthLimitation=False, currentSaturation=True, IpdSat=6e-3, shotNoise=False, thermalNoise=False)
IMB = dict(ampImbX=0.3, phaseImbX=-0.1, ampImbY=0.1, phaseImbY=0.05, pdl=0.7)
PLANS = {                        # name: (paramFE, paramPD, noise from unit normals, launches, the plan)
    "a": (A, IDEAL, False, 1, "delay+det+iqf"),
    "b": (dict(A, timeSkewX=1e-12, timeSkewY=-1e-12, **IMB), IDEAL, False, 3, "delay det skew"),
    "c": (dict(A, timeSkewX=1e-12, timeSkewY=30e-12, **IMB), BAND, True, 4, "delay lowpass skew skew"),
    "d": (dict(polRotation=-0.3, **IMB), BAND, True, 1, "lowpass+iqf"),
    "e": (dict(polRotation=-0.3, **IMB), FLAT, False, 1, "det+iqf"),
    "f": (dict(polRotation=-0.3, timeSkewX=2e-12, timeSkewY=2e-12, **IMB), FLAT, False, 2, "det skew"),
    "g": (dict(polRotation=-0.3, **IMB), dict(BAND, Fs=128e9), True, 1, "lowpass+iqf"),
    "h": (dict(polRotation=0.2, polDelay=1.5 / FS), IDEAL, False, 1, "delay+det+iqf"),          # each side delayed by 0.75 samples: padLen 1
    "h2": (dict(polRotation=0.2, polDelay=3.0 / FS), IDEAL, False, 1, "delay+det+iqf"),         # each side by 1.5 samples: padLen 2
}
COH = {k: ({n[:-1] if n[-1] == "X" else n: v for n, v in PLANS[k][0].items() if n[-1] != "Y" and n not in ("polRotation", "pdl")},) + PLANS[k][1:]
       for k in "def"}


def _rows():
    rows = []
    # 1. filters: the thresholds of fir_nfft and their neighbours, two blocks and five samples each
    for i, K in enumerate((1, 2, 32, 33, 64, 65, 128, 129, 682, 683, 2048, 2049, 4096)):
        d = fir_nfft(K) - K + 1
        rows.append(_row(f"fir-k{K}-n{2 * d + 5}x{i % 4 + 1}", "fir", 1000 + i, K=K, N=2 * d + 5, cols=i % 4 + 1))
    for i, K in enumerate((33, 255)):
        d = fir_nfft(K) - K + 1
        for j, N in enumerate((1, K - 1, K, d - 1, d, d + 1)):
            rows.append(_row(f"fir-k{K}-n{N}x2", "fir", 1020 + 10 * i + j, K=K, N=N, cols=2))
        for cols in (3, 4):                                         # a last workgroup with idle block groups
            rows.append(_row(f"fir-k{K}-n{2 * d + 5}x{cols}-ragged", "fir", 1040 + 10 * i + cols, K=K, N=2 * d + 5, cols=cols, ragged=1))
    for i, nfft in enumerate((256, 2048)):
        for j, K in enumerate((nfft, nfft - 1)):                    # blocks that advance by one and by two samples
            rows.append(_row(f"ols-nfft{nfft}-k{K}-n{nfft + 3}x2", "ols", 1060 + 2 * i + j, nfft=nfft, K=K, N=nfft + 3, cols=2))
    rows.append(_row("fir-k5-n5000-float32", "fir", 1070, K=5, N=5000, cols=0, dtype="float32"))
    # 2. long filters: one, two, three and four segments; a filter far longer than the signal; delaySignal's three routes
    for i, K in enumerate((4097, 8192, 8193, 12289)):               # (launches: one per segment that meets the signal)
        rows.append(_row(f"fir-k{K}-n9000x2", "fir", 1100 + i, launches=-(-K // 4096), K=K, N=9000, cols=2))
    rows.append(_row("fir-k9000-n100x2-zeros", "fir", 1104, launches=1, K=9000, N=100, cols=2))
    rows.append(_row("delay-nfftNone-n5000-d0", "delay", 1110, N=5000, delay=0.0, NFFT=None))
    rows.append(_row("delay-nfftNone-n5000-d2.5", "delay", 1111, N=5000, delay=2.5, NFFT=None))
    rows.append(_row("delay-nfft16384-n3000-d2.5", "delay", 1112, N=3000, delay=2.5, NFFT=16384))
    for i, N in enumerate((1, 1536, 1537, 1538)):
        for j, dl in enumerate((0.3, -3.2)):
            rows.append(_row(f"delay-n{N}-d{dl}", "delay", 1120 + 2 * i + j, N=N, delay=dl, NFFT=1024))
    # 3. decimate: thread counts of 256, 255, 224 and 129, one and two workgroups, the cap of 512
    for i, (si, so, cols) in enumerate(((2, 1, 1), (3, 1, 1), (16, 2, 4), (5, 1, 3), (7, 1, 8), (32, 2, 8), (129, 1, 1), (256, 2, 1),
                                        (5, 2, 3), (3, 2, 1))):
        for above in (0, 1):
            N = _dec_N(si, cols, above)
            seed = 1211 if (si, cols, above) == (32, 8, 0) else 1200 + 2 * i + above     # (four samples a phase: a seed whose boosted phases win)
            rows.append(_row(f"dec-{si}to{so}x{cols}-n{N}", "decimate", seed, SpSin=si, SpSout=so, cols=cols, N=N,
                             gen="boost", blocks=1 + above, phases=_dec_phases(si, cols, above)))
    rows.append(_row("dec-16to2x8-n65552-cap", "decimate", 1250, SpSin=16, SpSout=2, cols=8, N=65552, gen="boost", blocks=512,
                     phases=_dec_phases(16, 8, 0)))
    rows.append(_row("dec-16to2x4-n4096-offset", "decimate", 1251, SpSin=16, SpSout=2, cols=4, N=4096, gen="offset", blocks=16,
                     phases=_dec_phases(16, 4, 1)))
    rows.append(_row("dec-16to2x4-n1024-tie-all", "decimate", 1252, SpSin=16, SpSout=2, cols=4, N=1024, gen="tie_all", blocks=4, phases=(0, 0, 0, 0)))
    rows.append(_row("dec-16to2x4-n1024-tie-two", "decimate", 1253, SpSin=16, SpSout=2, cols=4, N=1024, gen="tie_two", blocks=4, phases=(3, 0, 5, 14),
                     second=(9, 15, 6, 15)))
    rows.append(_row("dec-33to1x8-refused", "decimate", 1254, raises="RuntimeError", SpSin=33, SpSout=1, cols=8, N=132, gen="boost", blocks=0, phases=(0,) * 8))
    rows.append(_row("dec-16to2x2-n100-refused", "decimate", 1255, raises="ValueError", SpSin=16, SpSout=2, cols=2, N=100, gen="boost", blocks=0, phases=(0, 0)))
    # 4. the launch plans of the receiver
    for i, (name, (fe, pd, noise, launches, plan)) in enumerate(PLANS.items()):
        rows.append(_row(f"pdm-{name}-n3000", "pdm", 1300 + i, launches=launches, N=3000, fe=fe, pd=pd, noise=noise, plan=plan))
    for i, N in enumerate((1, 17, 1536, 1537, 1538)):
        for j, name in enumerate("ac"):
            fe, pd, noise, launches, plan = PLANS[name]
            rows.append(_row(f"pdm-{name}-n{N}", "pdm", 1320 + 2 * i + j, launches=launches, N=N, fe=fe, pd=pd, noise=noise, plan=plan))
    for i, (name, (fe, pd, noise, launches, plan)) in enumerate(COH.items()):
        rows.append(_row(f"coh-{name}-n3000", "coh", 1340 + i, launches=launches, N=3000, fe=fe, pd=pd, noise=noise, plan=plan))
    rows.append(_row("iq-n3000", "iq", 1350, launches=1, N=3000, fe=dict(ampImb=0.4, phaseImb=0.2), pd={}, noise=False, plan="iqf"))
    rows.append(_row("iq-skew-n3000", "iq", 1351, launches=1, N=3000, fe=dict(ampImb=0.4, phaseImb=0.2, timeSkew=3e-12), pd={}, noise=False, plan="skew"))
    for modes in (1, 2, 3):
        rows.append(_row(f"pd-{modes}modes-band-n3000", "pd", 1360 + modes, launches=1, N=3000, modes=modes, pd=dict(B=25e9, N=101), noise=True))
        rows.append(_row(f"pd-{modes}modes-flat-n3000", "pd", 1370 + modes, launches=1, N=3000, modes=modes,
                         pd=dict(B=25e9, bandwidthLimitation=False, currentSaturation=True, IpdSat=5e-4), noise=True))
    rows.append(_row("pd-1modes-100taps-n3000", "pd", 1380, launches=1, N=3000, modes=1, pd=dict(B=25e9, N=100, fType="gauss"), noise=True))
    quiet = dict(B=25e9, N=101, shotNoise=False, thermalNoise=False)
    rows.append(_row("bpd-1d-n3000", "bpd", 1390, launches=1, N=3000, modes=0, pd=quiet, noise=False))
    rows.append(_row("bpd-2d-n3000", "bpd", 1391, launches=1, N=3000, modes=2, pd=quiet, noise=False))
    rows.append(_row("hybrid-n257", "hybrid", 1395, N=257))
    # 5. the chain: what the matched filter (ntaps) and the compensating filter (edc over L km) select
    for i, (ntaps, sps, L, N, what) in enumerate((
            (100, 16, 1200, 4096, dict(lg=10, stats=1, gather=1, idle=1)),
            (129, 16, 2000, 8192, dict(lg=11, stats=1, gather=1, dmod=0)),
            (130, 16, 2000, 8192, dict(lg=11, stats=1, gather=1, dodd=1)),
            (255, 8, 1000, 8192, dict(lg=11, stats=1, gather=1)),
            (1024, 16, 12000, 12288, dict(lg=12, stats=1, gather=1)),
            (2500, 16, 2000, 16384, dict(lg=13, stats=1, gather=1)),
            (129, 6, 400, 6144, dict(lg=11, stats=0, gather=1)),
            (129, 16, 800, 8192, dict(lg=11, stats=1, gather=0)),
            (33, 4, 5, 8192, dict(lg=9, stats=0, gather=0)))):
        rows.append(_row(f"chain-k{ntaps}-sps{sps}-L{L}-n{N}", "chain", 1400 + i, N=N, ntaps=ntaps, sps=sps, L=L, what=_freeze(what)))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
EMU_ROWS = [r for r in ROWS if r.emu]


# ------------------------------------------------------------------------------------------------------------------- inputs
def _cnormal(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _tie_values(rng, lo, hi, n):
    return rng.integers(lo, hi + 1, size=n) + 1j * rng.integers(lo, hi + 1, size=n)


def chain_case(N, ntaps, sps, L_edc, seed=81, pd=None, **fe_kw):
    """tests/test_round6.py: _chain_case."""
    E = synth_field(N, 2, seed, 0.0)
    lo = np.sqrt(5e-3) * np.exp(1j * 2 * np.pi * 2e8 * np.arange(N) / 64e9)
    fe = dict(Fs=64e9, polRotation=0.3, polDelay=2e-12, **fe_kw)
    pd = pd or dict(Fs=64e9, ideal=True)
    rng = np.random.default_rng(seed)
    h = rng.normal(size=ntaps) * np.hanning(ntaps)
    dec = dict(SpSin=sps, SpSout=2)
    edcp = dict(Fs=64e9 * 2 / sps, L=L_edc, D=16, Fc=193.1e12, Rs=32e9)
    return E, lo, fe, pd, h, dec, edcp


def _decimate_input(p, rng):
    N, sps, cols = p["N"], p["SpSin"], p["cols"]
    if p["gen"] in ("boost", "offset"):
        x = _cnormal(rng, (N, cols))
        for c, ph in enumerate(p["phases"]):
            x[ph::sps, c] *= 3
        return x + 1e6 if p["gen"] == "offset" else x
    M = N // sps
    x = np.empty((N, cols), dtype=np.complex128)
    for c in range(cols):
        base = _tie_values(rng, -4, 4, M)
        for ph in range(sps):
            if p["gen"] == "tie_all":                               # every phase holds the same values in another order
                x[ph::sps, c] = rng.permutation(base)
            else:                                                   # two phases hold the same large values, the others small ones
                x[ph::sps, c] = _tie_values(rng, -2, 2, M)
        if p["gen"] == "tie_two":
            big = rng.choice([-4, -3, 3, 4], size=M) + 1j * rng.choice([-4, -3, 3, 4], size=M)
            x[p["phases"][c]::sps, c] = rng.permutation(big)
            x[p["second"][c]::sps, c] = rng.permutation(big)
    return x


@functools.lru_cache(maxsize=None)
def _build(row):
    p, rng = params(row), np.random.default_rng(row.seed)
    kind = row.kind
    if kind in ("fir", "ols"):
        N, K, cols = p["N"], p["K"], p["cols"]
        if p.get("dtype") == "float32":
            s = dict(h=rng.normal(size=K) / K, x=rng.normal(size=N).astype(np.float32))
        else:
            s = dict(h=_cnormal(rng, K) / np.sqrt(K), x=_cnormal(rng, (N, cols)))
        if kind == "ols":
            s["H"] = np.ascontiguousarray(np.fft.fft(np.pad(s["h"], (0, p["nfft"] - K))))
    elif kind == "delay":
        s = dict(x=_cnormal(rng, p["N"]))
    elif kind == "decimate":
        s = dict(x=_decimate_input(p, rng))
    elif kind in ("pdm", "coh"):
        N, nm = p["N"], 2 if kind == "pdm" else 1
        Es = _cnormal(rng, (N, 2))[:, :nm] * 0.02
        s = dict(Es=np.ascontiguousarray(Es if nm == 2 else Es[:, 0]), Elo=np.sqrt(8e-3) * np.exp(1j * 2 * np.pi * 2e8 * np.arange(N) / FS),
                 un=rng.normal(size=(4 * nm, 2, N)) if p["noise"] else None)
    elif kind == "iq":
        s = dict(sig=_cnormal(rng, p["N"]) * 1e-3)
    elif kind == "pd":
        E = _cnormal(rng, (p["N"], p["modes"])) * 0.02
        s = dict(E=np.ascontiguousarray(E[:, 0]) if p["modes"] == 1 else E, un=rng.normal(size=(1, 2, p["N"])))
    elif kind == "bpd":
        shape = (p["N"], p["modes"]) if p["modes"] else p["N"]
        s = dict(E1=_cnormal(rng, shape) * 0.02, E2=_cnormal(rng, shape) * 0.02)
    elif kind == "hybrid":
        s = dict(Es=_cnormal(rng, p["N"]), Elo=_cnormal(rng, p["N"]) * 3)
    elif kind == "chain":
        E, lo, fe, pd, h, dec, edcp = chain_case(p["N"], p["ntaps"], p["sps"], p["L"], seed=row.seed)
        s = dict(Es=E, Elo=lo, h=h, fe=fe, pd=pd, dec=dec, edcp=edcp)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def signals(row):
    """The inputs of a row by name; arrays read-only, built once per process."""
    return _build(row)


def bag(cls, kw):
    o = cls()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _fe_pd(row):
    p = params(row)
    fe, pd = dict(Fs=FS, **p.get("fe", {})), dict(p.get("pd", {}))
    pd.setdefault("Fs", FS)
    return fe, pd


def _pd_noise(un, slot):
    return un[slot][0], un[slot][1]


def _pol_noise(un, b):
    """the oracle's layout: ((I pair: (PD1, PD2)), (Q pair: (PD1, PD2))), each PD = (shot, thermal)"""
    return (_pd_noise(un, b), _pd_noise(un, b + 1)), (_pd_noise(un, b + 2), _pd_noise(un, b + 3))


# ---------------------------------------------------------------------------------------------------------------- the calls
def call(row, api, sig=None):
    """The row's call on `api`: the package's functions, its parameters class and overlap_save(N, ncols, nfft, K, H, x) for the C
    ABI.  sig: the inputs, signals(row) or a copy of it with DeviceArrays in place of arrays."""
    s, p, P = sig or signals(row), params(row), api.parameters
    kind = row.kind
    if kind == "fir":
        return api.firFilter(s["h"], s["x"])
    if kind == "ols":
        return api.overlap_save(p["N"], p["cols"], p["nfft"], p["K"], s["H"], s["x"])
    if kind == "delay":
        return api.delaySignal(s["x"], p["delay"] / FS_FILT, FS_FILT) if p["NFFT"] == 1024 else api.delaySignal(s["x"], p["delay"] / FS_FILT, FS_FILT, p["NFFT"])
    if kind == "decimate":
        return api.decimate(s["x"], bag(P, dict(SpSin=p["SpSin"], SpSout=p["SpSout"])))
    if kind == "hybrid":
        return api.opticalHybrid2x4(s["Es"], s["Elo"])
    if kind == "chain":
        return api.pdmCoherentReceiverChain(s["Es"], s["Elo"], bag(P, s["fe"]), bag(P, s["pd"]), s["h"], bag(P, s["dec"]), bag(P, s["edcp"]))
    fe, pd = _fe_pd(row)
    if kind == "pdm":
        return api.pdmCoherentReceiver(s["Es"], s["Elo"], bag(P, fe), bag(P, pd), _unit_normals=s["un"])
    if kind == "coh":
        return api.coherentReceiver(s["Es"], s["Elo"], bag(P, fe), bag(P, pd), _unit_normals=s["un"])
    if kind == "iq":
        return api.iqMixing(s["sig"], bag(P, fe))
    if kind == "pd":
        return api.photodiode(s["E"], bag(P, pd), _unit_normals=s["un"])
    if kind == "bpd":
        return api.balancedPD(s["E1"], s["E2"], bag(P, pd))
    raise KeyError(kind)


def call_four(row, api, sig=None):
    """A chain row as the four calls it stands for."""
    s, P = sig or signals(row), api.parameters
    rx = api.pdmCoherentReceiver(s["Es"], s["Elo"], bag(P, s["fe"]), bag(P, s["pd"]))
    return api.edc(api.decimate(api.firFilter(s["h"], rx), bag(P, s["dec"])), bag(P, s["edcp"]))


@functools.lru_cache(maxsize=None)
def _matched(row):
    """A chain row's signal behind the matched filter, from the oracle."""
    s = signals(row)
    rx = orx.pdmCoherentReceiver(s["Es"], s["Elo"], bag(orc.parameters, s["fe"]), bag(orc.parameters, s["pd"]))
    return orx.firFilter(s["h"], rx)


@functools.lru_cache(maxsize=None)
def expected(row):
    """The expected output of a row, computed once per process (None for a row that must raise)."""
    s, p, kind, P = signals(row), params(row), row.kind, orc.parameters
    if row.raises:
        return None
    if kind in ("fir", "ols"):
        out = rr.convolve_same(s["h"], s["x"])
        out = out.real.astype(np.float32) if p.get("dtype") == "float32" else out.astype(np.complex128)
    elif kind == "delay":
        out = rr.delay_signal(s["x"], p["delay"] / FS_FILT, FS_FILT, p["NFFT"]).astype(np.complex128)
    elif kind == "decimate":
        out = rr.decimate(s["x"], p["SpSin"], p["SpSout"])[0]
    elif kind == "hybrid":
        out = orx.opticalHybrid2x4(s["Es"], s["Elo"])
    elif kind == "chain":
        out = orc.edc(orx.decimate(_matched(row), bag(P, s["dec"])), bag(P, s["edcp"]))
    else:
        fe, pd = _fe_pd(row)
        un = s.get("un")
        if kind == "pdm":
            out = orx.pdmCoherentReceiver(s["Es"], s["Elo"], bag(P, fe), bag(P, pd), noise=None if un is None else (_pol_noise(un, 0), _pol_noise(un, 4)))
        elif kind == "coh":
            out = orx.coherentReceiver(s["Es"], s["Elo"], bag(P, fe), bag(P, pd), noise=None if un is None else _pol_noise(un, 0))
        elif kind == "iq":
            out = orx.iqMixing(s["sig"], bag(P, fe))
        elif kind == "pd":
            out = orx.photodiode(s["E"], bag(P, pd), noise=_pd_noise(un, 0))
        else:
            out = orx.balancedPD(s["E1"], s["E2"], bag(P, pd))
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------------- the conditions
def plan(kind, fe, pd):
    """RxCore::run_coherent's branches restated -> (the launches in order, their number)."""
    iq_only = kind == "iq"
    quiet = bool(pd.get("ideal", False))
    lowpass = not iq_only and not quiet and pd.get("bandwidthLimitation", True)
    noisy = not iq_only and not quiet and (pd.get("shotNoise", True) or pd.get("thermalNoise", True))
    skews = [fe.get("timeSkewX", 0), fe.get("timeSkewY", 0)] if kind == "pdm" else [fe.get("timeSkew", 0)]
    skew = any(s != 0 for s in skews)
    steps, detected = [], iq_only
    if kind == "pdm" and fe.get("polDelay", 0) != 0:
        detected = not lowpass and not skew and not noisy
        steps.append("delay+det+iqf" if detected else "delay")
    if not detected:
        steps.append(("lowpass" if lowpass else "det") + ("" if skew else "+iqf"))
    if skew:
        pads = {math.ceil(abs(s / 2 * fe["Fs"])) for s in skews}
        steps += ["skew"] * (1 if len(pads) == 1 else len(skews))
    elif iq_only:
        steps.append("iqf")
    return " ".join(steps), len(steps)


def check_conditions(row):
    """The row cannot pass or fail by rounding, and it selects the path it is named for."""
    p, kind = params(row), row.kind
    if kind in ("fir", "ols"):
        K, N, cols = p["K"], p["N"], max(p["cols"], 1)
        nfft = p["nfft"] if kind == "ols" else fir_nfft(K)
        if K <= 4096:
            lg, C, gpw, jobs = ols_launch(nfft, cols, num_blocks(N, K, nfft))
            if p.get("ragged"):
                assert jobs % gpw != 0 or (gpw == 1 and (K, cols) == (255, 4)), (row.id, jobs, gpw)     # (two columns of 2048 points fill a workgroup)
        else:
            segs = [(p0, min(4096, K - p0)) for p0 in range(0, K, 4096)]
            met = [min(N + (K - 1) // 2 - p0, N + Kp - 1) > max(0, (K - 1) // 2 - p0) for p0, Kp in segs]
            assert len(segs) == -(-K // 4096) and all(met) != row.id.endswith("zeros") and sum(met) == row.launches, (row.id, met)
    elif kind == "delay":
        pad = math.ceil(abs(p["delay"]))
        nfft = p["NFFT"] or 2 ** math.ceil(math.log2(p["N"] + pad))
        assert (nfft // 2 > 4096) == (p["NFFT"] == 16384) and (pad == 0) == (p["delay"] == 0.0), row.id
    elif kind == "decimate":
        nclass = p["SpSin"] * p["cols"]
        if row.raises:
            assert (nclass > 256) != (p["N"] % p["SpSin"] != 0), row.id
            return
        nthreads, blocks = dec_launch(p["N"], p["SpSin"], p["cols"])
        assert min(blocks, 512) == p["blocks"] and (blocks > 512) == row.id.endswith("cap"), (row.id, nthreads, blocks)
        _, delay, margin = rr.decimate(signals(row)["x"], p["SpSin"], p["SpSout"])
        assert tuple(delay) == p["phases"], (row.id, delay)
        if p["gen"].startswith("tie"):
            x = signals(row)["x"]
            var = np.var(x.reshape(-1, p["SpSin"], p["cols"]), axis=0)                   # exact in double: small Gaussian integers, 2^k of them
            for c in range(p["cols"]):
                tied = np.flatnonzero(var[:, c] == var[:, c].max())
                assert list(tied) == (list(range(p["SpSin"])) if p["gen"] == "tie_all" else [p["phases"][c], p["second"][c]]), (row.id, c, tied)
        else:
            assert margin >= MARGIN, (row.id, margin)
    elif kind in ("pdm", "coh", "iq"):
        fe, pd = _fe_pd(row)
        assert plan(kind, fe, pd) == (p["plan"], row.launches), (row.id, plan(kind, fe, pd))
        if row.id.startswith("pdm-h"):
            assert math.ceil(abs(fe["polDelay"] / 2 * FS)) == (2 if row.id.startswith("pdm-h2") else 1), row.id
        if row.id.startswith("pdm-g"):
            assert pd["Fs"] != fe["Fs"], row.id
    elif kind == "chain":
        from opticommpy_amd import models
        s, what = signals(row), dict(p["what"])
        N, ntaps, sps = p["N"], p["ntaps"], p["sps"]
        nfft = fir_nfft(ntaps)
        assert nfft == models._ols_block(ntaps)
        lg, C, gpw, jobs = ols_launch(nfft, 2, num_blocks(N, ntaps, nfft))
        stats = chain_kernel(lg, C) and (nfft // 16) % sps == 0 and 2 * sps <= 256
        K, _, _ = models._edc_filter(bag(orc.parameters, s["edcp"]), s["edcp"]["Fs"])
        dec = int(s["dec"]["SpSin"] / s["dec"]["SpSout"])
        enfft = models._ols_block(K)
        elg, eC, _, _ = ols_launch(enfft, 2, num_blocks(-(-N // dec), K, enfft))
        gather = chain_kernel(elg, eC)
        assert (int(math.log2(nfft)), bool(stats), bool(gather)) == (what["lg"], bool(what["stats"]), bool(what["gather"])), (row.id, nfft, stats, K, gather)
        assert (K >= 65) == gather, (row.id, K)
        d = nfft - ntaps + 1
        if "dmod" in what:
            assert d % sps == what["dmod"], (row.id, d)
        if "dodd" in what:
            assert d % 2 == 1, (row.id, d)
        if "idle" in what:
            assert jobs % gpw != 0, (row.id, jobs, gpw)
        margin = rr.decimate(_matched(row), s["dec"]["SpSin"], s["dec"]["SpSout"])[2]
        assert margin >= MARGIN, (row.id, margin)


def compare(row, out, label=""):
    want, p, kind = expected(row), params(row), row.kind
    tag = f"{label} {row.id}"
    assert type(out) is np.ndarray and out.shape == want.shape and out.dtype == want.dtype, (tag, out.shape, out.dtype, want.shape, want.dtype)
    if kind in ("decimate", "hybrid"):
        assert out.tobytes() == want.tobytes(), tag
    elif p.get("dtype") == "float32":
        np.testing.assert_allclose(out, want, rtol=0, atol=F32_ATOL, err_msg=tag)
    elif kind in ("fir", "ols", "delay"):
        assert rel_l2(out, want) <= FIR_TOL, (tag, rel_l2(out, want))
    else:
        tol = CHAIN_TOL if kind == "chain" else RX_TOL
        err, scale = np.max(np.abs(out - want)), np.max(np.abs(want))
        assert err <= tol * scale, (tag, err, scale)
