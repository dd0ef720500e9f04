#!/usr/bin/env python3
"""Generate the sampling-clock fixtures tests/golden/clock/*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_sync.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity,
``prange`` = range), and one for ``tqdm`` if that is missing.  No bytecode is written.  Data only; every file stays under MAX_BYTES.

    interp_*   x, inFs, outFs, jitter, seed -> y = clockSamplingInterp(x, inFs, outFs, jitter) after np.random.seed(seed)
    quant_*    x, nBits, maxV, minV -> y = quantizer(x, nBits, maxV, minV)
    conv_*     sigIn, the parameters (cfg), seed -> out = adc / dac / resample / dac -> adc after np.random.seed(seed); qdist = the
               smallest distance of a value the reference handed to its quantizer from a decision threshold and xmax = the largest
               such |value| (recorded by wrapping the reference's quantizer, the reference is not edited).  Kept only if
               qdist >= 100 * 1e-9 * xmax; seeds are searched until one qualifies.
    gardner_*  x (the dac -> adc pair of the reference's notebook at the case's clock offset, 16-QAM, raised cosine, roll-off 0.05,
               adc at 8 bits, then pnorm), the parameters -> out, tv = gardnerClockRecovery(x, param); dist_sig (in units of the
               single-precision spacing at the largest |out|) and dist_t (absolute) between the reference's result and
               tests/clock_restatement.py's, margin = the smallest | |t_nco| - 1 | of the restatement's run, gaps = the indices
               where |diff(tv)| > 0.5.  Asserted here and again by tests/clock_cases.py: equal shapes, equal gap pattern,
               margin >= 10 dist_t.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_clock.py [family or case ...]
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True

_nb = types.ModuleType("numba")


def _identity_decorator(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f


_nb.njit = _nb.jit = _identity_decorator
_nb.prange = range
_nb_typed = types.ModuleType("numba.typed")
_nb_typed.List = list
_nb.typed = _nb_typed
sys.modules["numba"] = _nb
sys.modules["numba.typed"] = _nb_typed
if importlib.util.find_spec("tqdm") is None:
    _tq = types.ModuleType("tqdm")
    _tq.tqdm = lambda it, **k: it
    _tqn = types.ModuleType("tqdm.notebook")
    _tqn.tqdm = _tq.tqdm
    _tq.notebook = _tqn
    sys.modules["tqdm"] = _tq
    sys.modules["tqdm.notebook"] = _tqn
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(HERE, "..", "..", "reference")))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import numpy as np  # noqa: E402

import optic.dsp.core as ref_core  # noqa: E402
import optic.models.devices as ref_dev  # noqa: E402
import optic.dsp.clockRecovery as ref_clk  # noqa: E402
from optic.comm.modulation import modulateGray as ref_modulate  # noqa: E402
from optic.comm.metrics import fastBERcalc as ref_ber  # noqa: E402
from optic.utils import parameters as ref_parameters  # noqa: E402

import clock_restatement as rs  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "clock")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py
B = 1e-9                    # the bound firFilter is held to against reference fixtures (tests/clock_cases.py: FIR_REL)
RATIO_ADC = 0.5 * (1 + 105e-6)


def save(name, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    return size


def params(d):
    p = ref_parameters()
    for k, v in d.items():
        setattr(p, k, v)
    return p


# ---- interpolation
INTERP = {
    "adc_ratio_c128": dict(N=3001, cols=2, ratio=RATIO_ADC, dtype="complex128", jitter=0),
    "unity_f64": dict(N=2000, cols=3, ratio=1.0, dtype="float64", jitter=0),
    "double_c64": dict(N=1500, cols=2, ratio=2.0, dtype="complex64", jitter=0),
    "third_f32": dict(N=3000, cols=1, ratio=1 / 3, dtype="float32", jitter=0),
    "jitter_c128": dict(N=1000, cols=2, ratio=RATIO_ADC, dtype="complex128", jitter=2.5),
    "jitter_c64": dict(N=1000, cols=1, ratio=2.0, dtype="complex64", jitter=2.5),
    "jitter_f64": dict(N=1000, cols=2, ratio=1.0, dtype="float64", jitter=2.5),
    "jitter_f32": dict(N=1000, cols=3, ratio=1 / 3, dtype="float32", jitter=2.5),
}


def gen_interp(name):
    c = INTERP[name]
    inFs = 64e9
    outFs = inFs * c["ratio"]
    jitter = c["jitter"] / inFs                       # in input sampling periods
    tin_end = (c["N"] - 1) / inFs
    first = 7000 + 100 * sorted(INTERP).index(name)
    for seed in range(first, first + 100):            # (with jitter: until times fall before the start, beyond the end, out of order)
        np.random.seed(seed)
        tout = rs.jittered(c["N"], inFs, outFs, jitter)
        found = dict(negative=int(np.sum(tout < 0)), beyond=int(np.sum(tout > tin_end)), unordered=int(np.sum(np.diff(tout) < 0)))
        if not c["jitter"] or min(found.values()) > 0:
            break
    else:
        raise SystemExit(f"{name}: no seed gives times on all three sides")
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(c["N"], c["cols"]))
    if c["dtype"].startswith("complex"):
        x = x + 1j * rng.normal(size=x.shape)
    x = x.astype(c["dtype"])
    np.random.seed(seed)
    y = ref_core.clockSamplingInterp(x, inFs, outFs, jitter)
    assert y.dtype == x.dtype and np.array_equal(y, rs.clock_interp(x, inFs, outFs, tout), equal_nan=True)
    cfg = dict(c, name=name, seed=seed, inFs=inFs, outFs=outFs, jitter_s=jitter, numpy=np.__version__, **found)
    size = save(f"interp_{name}", x=x, y=y, cfg=json.dumps(cfg))
    print(f"interp_{name}: {size >> 10} KiB  out {y.shape}  negative {cfg['negative']} beyond {cfg['beyond']} unordered {cfg['unordered']}", flush=True)


# ---- quantizer
QUANT = {"b1": dict(nBits=1, maxV=1.1, minV=-1.3, n=400), "b2": dict(nBits=2, maxV=0.9, minV=-0.7, n=400),
         "b8": dict(nBits=8, maxV=1, minV=-1, n=1500), "b16": dict(nBits=16, maxV=0.777, minV=-0.123, n=600)}


def gen_quant(name):
    c = QUANT[name]
    seed = 7100 + sorted(QUANT).index(name)
    rng = np.random.default_rng(seed)
    d = rs.quant_levels(c["nBits"], c["maxV"], c["minV"])
    span = c["maxV"] - c["minV"]
    pick = rng.integers(0, len(d) - 1, size=c["n"] // 4)
    mids = (d[pick] + d[pick + 1]) / 2                                   # the decision thresholds themselves, and their neighbours
    x = np.concatenate([rng.uniform(c["minV"] - 0.2 * span, c["maxV"] + 0.2 * span, size=c["n"] // 2), mids, np.nextafter(mids, np.inf),
                        np.nextafter(mids, -np.inf), d[pick], [c["minV"], c["maxV"], d[-1], c["minV"] - span, c["maxV"] + span, 0.0]])
    x = x[:2 * (len(x) // 2)].reshape(-1, 2)
    y = ref_core.quantizer(x, c["nBits"], c["maxV"], c["minV"])
    assert np.array_equal(y, rs.quantizer(x, c["nBits"], c["maxV"], c["minV"]))
    cfg = dict(c, name=name, seed=seed, levels=len(d), numpy=np.__version__)
    size = save(f"quant_{name}", x=x, y=y, cfg=json.dumps(cfg))
    print(f"quant_{name}: {size >> 10} KiB  levels {len(d)}  x {x.shape}", flush=True)


# ---- signals: 16-QAM, raised cosine, roll-off 0.05
def shaped_signal(nsymb, cols, seed, SpS=4):
    """(sigTx at SpS samples per symbol, symbTx): the transmitter of the reference's notebook."""
    np.random.seed(seed)
    bits = np.random.randint(2, size=4 * nsymb * cols)
    symb = ref_core.pnorm(ref_modulate(bits, 16, "qam")).reshape(-1, cols)
    pulse = ref_core.pulseShape(params(dict(SpS=SpS, nFilterTaps=1024, rollOff=0.05, pulseType="rc")))
    sig = ref_core.pnorm(ref_core.firFilter(pulse, ref_core.upsample(symb, SpS)))
    return sig, symb


class Recorder:
    """Wraps the quantizer the reference's converters call: the values handed to it, per call."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.saved = ref_dev.quantizer

        def recording(x, nBits=16, maxV=1, minV=-1):
            self.calls.append((np.array(x, dtype=np.float64), nBits, float(maxV), float(minV)))
            return self.saved(x, nBits, maxV, minV)

        ref_dev.quantizer = recording
        return self

    def __exit__(self, *a):
        ref_dev.quantizer = self.saved

    def distance(self):
        """(the smallest distance of a recorded value from a decision threshold, the largest |value|)."""
        q, top = np.inf, 0.0
        for x, nBits, maxV, minV in self.calls:
            d = rs.quant_levels(nBits, maxV, minV)
            thr = (d[:-1] + d[1:]) / 2
            v = x.reshape(-1)
            i = np.clip(np.searchsorted(thr, v), 1, len(thr) - 1)
            q = min(q, float(np.min(np.minimum(np.abs(v - thr[i - 1]), np.abs(v - thr[i])))))
            top = max(top, float(np.max(np.abs(v))))
        return q, top


FS = 4 * 32e9
CONV = {
    # name: function, input (complex / real, columns, 1-D), parameters
    "adc_complex_nofilter": dict(fn="adc", cplx=True, cols=2, single=True, p=dict(inFs=FS, outFs=FS * RATIO_ADC, nBits=8, ENOB=8, Vmax=0.9, Vmin=-0.8, AAF=False)),
    "adc_real_nofilter": dict(fn="adc", cplx=False, cols=1, one_d=True, single=True, p=dict(inFs=FS, outFs=FS * RATIO_ADC, nBits=6, ENOB=6, Vmax=1.0, Vmin=-1.0, AAF=False)),
    "dac_complex_nofilter": dict(fn="dac", cplx=True, cols=2, p=dict(inFs=FS, outFs=FS * (1 + 75e-6), nBits=8, ENOB=8, Vpp=2, AIF=False)),
    "dac_real_nofilter": dict(fn="dac", cplx=False, cols=2, p=dict(inFs=FS, outFs=FS * (1 + 75e-6), nBits=5, ENOB=5, Vpp=1.5, AIF=False)),
    "adc_complex_filters": dict(fn="adc", cplx=True, cols=2, p=dict(inFs=FS, outFs=FS * RATIO_ADC, nBits=8, ENOB=8, Vmax=1.5, Vmin=-1.5, AAF=True, N=201)),
    "adc_real_filters": dict(fn="adc", cplx=False, cols=1, p=dict(inFs=FS, outFs=FS * RATIO_ADC, nBits=8, ENOB=8, Vmax=1.5, Vmin=-1.5, AAF=True, N=101)),
    "dac_complex_filters": dict(fn="dac", cplx=True, cols=1, one_d=True, p=dict(inFs=FS, outFs=FS * (1 + 75e-6), nBits=8, ENOB=8, Vpp=2, AIF=True, N=201)),
    "dac_real_filters": dict(fn="dac", cplx=False, cols=2, p=dict(inFs=FS, outFs=FS * (1 + 75e-6), nBits=8, ENOB=8, Vpp=2, AIF=True, N=101)),
    "adc_jitter_enob": dict(fn="adc", cplx=True, cols=2, p=dict(inFs=FS, outFs=FS * RATIO_ADC, jitter=500e-15, nBits=8, ENOB=6.5, Vmax=1.5, Vmin=-1.5, AAF=False)),
    "adc_complex_nofilter_double": dict(fn="adc", cplx=True, cols=2, p=dict(inFs=FS, outFs=FS * RATIO_ADC, nBits=4, ENOB=4, Vmax=0.7, Vmin=-0.9, AAF=False)),
    "adc_defaults": dict(fn="adc", cplx=True, cols=1, p=dict()),
    "resample_down": dict(fn="resample", cplx=True, cols=2, p=dict(inFs=FS, outFs=FS / 2, N=201)),
    "resample_up_1d": dict(fn="resample", cplx=True, cols=1, one_d=True, p=dict(inFs=FS / 2, outFs=FS, N=101)),
    "notebook_pair": dict(fn="pair", cplx=True, cols=2, p=dict(
        dac=dict(inFs=FS, outFs=FS * (1 + 75e-6), jitter=500e-15, nBits=8, ENOB=5.5, Vpp=2, AIF=True),
        adc=dict(inFs=FS * (1 + 75e-6), outFs=2 * 32e9 * (1 + 105e-6), jitter=500e-15, nBits=8, ENOB=6.5, AAF=True, N=1001))),
}
CONV_SYMBOLS = 500          # 2000 samples at 4 samples per symbol


def run_conv(c, sig, seed):
    np.random.seed(seed)
    if c["fn"] == "pair":
        pd, pa = params(c["p"]["dac"]), params(c["p"]["adc"])
        mid = ref_dev.dac(sig, pd)
        pa.Vmax, pa.Vmin = np.max(mid.real), np.min(mid.real)
        return ref_dev.adc(mid, pa), dict(Vmax=float(pa.Vmax), Vmin=float(pa.Vmin))
    p = params(c["p"])
    fn = dict(adc=ref_dev.adc, dac=ref_dev.dac, resample=ref_core.resample)[c["fn"]]
    out = fn(sig, p)
    return out, {k: (v if isinstance(v, (bool, int, float, str)) else float(v)) for k, v in vars(p).items()}


def gen_conv(name):
    c = CONV[name]
    first = 7200 + 50 * sorted(CONV).index(name)
    for seed in range(first, first + 50):
        sig, _ = shaped_signal(CONV_SYMBOLS, c["cols"], seed)
        if not c["cplx"]:
            sig = np.ascontiguousarray(sig.real)
        if not c.get("single"):                       # (the reference's transmitter works in single precision)
            sig = sig.astype(np.complex128 if c["cplx"] else np.float64)
        if c.get("one_d"):
            sig = sig[:, 0].copy()
        keep = sig.copy()
        with Recorder() as rec:
            out, written = run_conv(c, sig, seed)
        assert np.array_equal(sig, keep)
        qdist, xmax = rec.distance() if rec.calls else (np.inf, 0.0)
        if qdist >= 100 * B * xmax:
            break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 50}) keeps every sample 100 B max|x| off the thresholds")
    cfg = dict(name=name, fn=c["fn"], p=c["p"], written=written, seed=seed, one_d=bool(c.get("one_d")), numpy=np.__version__)
    size = save(f"conv_{name}", sigIn=sig, out=out, qdist=qdist, xmax=xmax, cfg=json.dumps(cfg))
    print(f"conv_{name}: {size >> 10} KiB  seed {seed}  in {sig.dtype}{sig.shape} out {out.dtype}{out.shape}  qdist {qdist:.3e}  xmax {xmax:.3f}", flush=True)


# ---- clock recovery
GARDNER = {
    "p300_nyq_c128": dict(ppm=300, nsymb=3500, cols=1, dtype="complex128", p=dict(isNyquist=True, lpad=1, maxPPM=500)),
    "m300_nyq_c64_1d": dict(ppm=-300, nsymb=3500, cols=1, one_d=True, dtype="complex64", p=dict(isNyquist=True, lpad=7, maxPPM=500)),
    "zero_nyq_c128": dict(ppm=0, nsymb=1500, cols=2, dtype="complex128", p=dict(isNyquist=True, lpad=0, maxPPM=0)),
    "p300_ted_c64": dict(ppm=300, nsymb=3500, cols=1, dtype="complex64", p=dict(isNyquist=False, lpad=0, maxPPM=500, kp=2e-3)),
    "m300_ted_c128_1d": dict(ppm=-300, nsymb=3500, cols=1, one_d=True, dtype="complex128", p=dict(isNyquist=False, lpad=7, maxPPM=0)),
    "two_modes_c64": dict(ppm=300, nsymb=2000, cols=2, dtype="complex64", p=dict(isNyquist=True, lpad=1, maxPPM=500, ki=2e-6)),
}


def clocked_signal(ppm, nsymb, cols, seed):
    """The notebook's dac -> adc pair with the adc's clock `ppm` off (roll-off 0.05, adc at 8 bits with its filters on), then pnorm;
    also the transmitted symbols."""
    sig, symb = shaped_signal(nsymb, cols, seed)
    np.random.seed(seed + 1)
    mid = ref_dev.dac(sig, params(dict(inFs=FS, outFs=FS, nBits=8, ENOB=8, Vpp=2, AIF=True)))
    mid = mid.reshape(len(mid), -1)
    rx = ref_dev.adc(mid, params(dict(inFs=FS, outFs=2 * 32e9 * (1 + ppm / 1e6), nBits=8, ENOB=8, Vmax=float(np.max(mid.real)),
                                      Vmin=float(np.min(mid.real)), AAF=True, N=1001)))
    return ref_core.pnorm(rx.reshape(len(rx), -1)), symb


def gap_indices(tv):
    return [np.nonzero(np.abs(np.diff(tv[:, k])) > 0.5)[0].tolist() for k in range(tv.shape[1])]


def gen_gardner(name):
    c = GARDNER[name]
    seed = 7900 + 10 * sorted(GARDNER).index(name)
    x, symb = clocked_signal(c["ppm"], c["nsymb"], c["cols"], seed)
    x = x.astype(c["dtype"])
    if c.get("one_d"):
        x = x[:, 0].copy()
    p = dict(kp=1e-3, ki=1e-6, returnTiming=True)
    p.update(c["p"])
    keep = x.copy()
    out, tv = ref_clk.gardnerClockRecovery(x, params(p))
    assert np.array_equal(x, keep)
    want, tvw, info = rs.gardner(x, p["kp"], p["ki"], p["isNyquist"], p["lpad"], p["maxPPM"])
    assert out.shape == want.shape and tv.shape == tvw.shape and out.dtype == np.complex64 and tv.dtype == np.float64, (out.shape, want.shape)
    gaps = gap_indices(tv)
    assert gaps == gap_indices(tvw), (gaps, gap_indices(tvw))
    spacing = float(np.spacing(np.float32(np.max(np.abs(want)))))
    dist_sig = float(np.max(np.abs(out.astype(np.complex128) - want.astype(np.complex128))) / spacing)
    dist_t = float(np.max(np.abs(tv - tvw)))
    assert info["margin"] >= 10 * dist_t, (info["margin"], dist_t)
    ppm_ref = ref_clk.calcClockDrift(tv)
    cfg = dict(name=name, ppm=c["ppm"], p=p, seed=seed, one_d=bool(c.get("one_d")), gaps=gaps, last_n=info["last_n"], numpy=np.__version__,
               drift=[None if np.isnan(v) else float(v) for v in ppm_ref])
    size = save(f"gardner_{name}", x=x, out=out, tv=tv, dist_sig=dist_sig, dist_t=dist_t, margin=info["margin"], cfg=json.dumps(cfg))
    print(f"gardner_{name}: {size >> 10} KiB  x {x.dtype}{x.shape} out {out.shape}  gaps {[len(g) for g in gaps]}  dist_sig {dist_sig:.1f} spacings  "
          f"dist_t {dist_t:.2e}  margin {info['margin']:.2e}  drift {cfg['drift']}", flush=True)


def chain_ber():
    """What the reference alone gives on the signal of tests/test_gpu_clock.py's chain test (tests/clock_cases.py: chain_signal builds
    the same one from the same seed with this package): BER of the recovered and of the unrecovered adc output."""
    import clock_cases as cc
    x, symb = clocked_signal(300, cc.CHAIN_SYMBOLS, 2, cc.CHAIN_SEED)
    out = ref_clk.gardnerClockRecovery(x, params(dict(cc.CHAIN_GARDNER)))
    for label, y in (("recovered", out[0::2]), ("unrecovered", x[0::2])):
        n = min(len(y), len(symb))
        ber = ref_ber(y[:n], symb[:n], 16, "qam")[0]
        d = 1500
        ber_d = ref_ber(y[d:n - d], symb[d:n - d], 16, "qam")[0]
        print(f"chain {label}: BER {ber} (all)  {ber_d} (1500 discarded each side)", flush=True)


FAMILIES = {"interp": (INTERP, gen_interp), "quant": (QUANT, gen_quant), "conv": (CONV, gen_conv), "gardner": (GARDNER, gen_gardner)}

if __name__ == "__main__":
    want = sys.argv[1:] or list(FAMILIES)
    for w in want:
        if w == "chain_ber":
            chain_ber()
        elif w in FAMILIES:
            for case in FAMILIES[w][0]:
                FAMILIES[w][1](case)
        else:
            fam, case = w.split(":", 1)
            FAMILIES[fam][1](case)
