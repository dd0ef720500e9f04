"""Shared by the sampling-clock tests: the fixtures tests/golden/clock/*.npz (tools/gen_golden_clock.py), the conditions every
fixture must meet so that no test passes emptily, the parameter objects, the bounds, and the files the emulator
(tests/emu/emu_clock.cpp) reads and writes.

The bounds:
    interpolation, clip, quantizer and every converter with its filters off    np.array_equal with the reference's recorded result
    converters with filters on       max |out - ref| <= k FIR_REL max |ref|, k the number of firFilter calls in the path and
                                     FIR_REL = 1e-9 the bound the receiver tests hold firFilter to against reference fixtures.  The
                                     quantizer is discontinuous, so the generator kept a fixture only if no value handed to the
                                     quantizer lies within 100 FIR_REL max|x| of a decision threshold (qdist, xmax: re-checked here)
    clock recovery against tests/clock_restatement.py      signal, timing values and shapes bit-equal
    clock recovery against the reference's recorded run    the same shapes and gap pattern; the distances at most 2 x those the
                                     generator recorded between the reference and the restatement (the device equals the
                                     restatement, so the recorded distance is the expected value; the factor covers a fixture
                                     regenerated under another numpy).  Recorded: at most 9.9 single-precision spacings and 1.04e-6,
                                     margins | |t_nco| - 1 | of 1.1e-4 and more (>= 10 x the timing distance, asserted).
"""
import glob
import json
import os
import subprocess

import numpy as np

import clock_restatement as rs
from opticommpy_amd import _lib, clock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clock")
FIR_REL = 1e-9


def names(family):
    return sorted(os.path.basename(p)[len(family) + 1:-4] for p in glob.glob(os.path.join(GOLDEN, f"{family}_*.npz")))


INTERP, QUANT, CONV, GARDNER = names("interp"), names("quant"), names("conv"), names("gardner")
FILTERS = {"adc_complex_filters": 2, "adc_real_filters": 2, "adc_defaults": 2, "dac_complex_filters": 1, "dac_real_filters": 1,
           "resample_down": 1, "resample_up_1d": 1, "notebook_pair": 3}          # firFilter calls in the path; absent: none

# the chain test (tests/test_gpu_clock.py) and tools/gen_golden_clock.py chain_ber
CHAIN_SYMBOLS, CHAIN_SEED = 8000, 4321
CHAIN_GARDNER = dict(kp=1e-3, ki=1e-6, isNyquist=True, lpad=1, maxPPM=500)
# what the reference alone gives on the signal its own functions build from CHAIN_SEED (1500 symbols discarded each side), per mode
CHAIN_REFERENCE_BER = dict(recovered=[0.00430086, 0.00385077], unrecovered=[0.49475, 0.49905])
FS = 4 * 32e9


class Param:
    """Stand-in for the reference's parameters object: attributes only."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


_LOADED = {}


def load(family, name):
    """A fixture, read once and shared (nobody writes to it)."""
    key = f"{family}_{name}"
    if key not in _LOADED:
        z = np.load(os.path.join(GOLDEN, f"{key}.npz"))
        g = {k: z[k] for k in z.files}
        g["cfg"] = json.loads(str(g["cfg"]))
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _LOADED[key] = g
    return _LOADED[key]


def check_conditions(family, g):
    """What the generator promised, re-asserted on the stored arrays."""
    c = g["cfg"]
    if family == "interp":
        assert g["x"].dtype.name == c["dtype"] and g["y"].dtype == g["x"].dtype and g["y"].shape[1] == g["x"].shape[1]
        assert len(g["y"]) == clock.output_length(len(g["x"]), 1 / c["inFs"], 1 / c["outFs"])
        if c["jitter"]:
            assert c["negative"] > 0 and c["beyond"] > 0 and c["unordered"] > 0
    elif family == "quant":
        d = rs.quant_levels(c["nBits"], c["maxV"], c["minV"])
        x = g["x"].reshape(-1)
        thr = (d[:-1] + d[1:]) / 2
        assert np.any(x == c["minV"]) and np.any(x == c["maxV"]) and np.any(x < c["minV"]) and np.any(x > d[-1])
        assert np.sum(np.isin(x, thr)) >= 1 and set(np.unique(g["y"])) <= set(d)
    elif family == "conv":
        assert float(g["qdist"]) >= 100 * FIR_REL * float(g["xmax"])
        assert g["sigIn"].dtype.kind in "fc" and g["out"].size > 0 and (g["sigIn"].ndim == 1) == c["one_d"]
    elif family == "gardner":
        assert g["out"].dtype == np.complex64 and g["tv"].dtype == np.float64 and g["x"].dtype.name in ("complex128", "complex64")
        assert float(g["margin"]) >= 10 * float(g["dist_t"]) and float(g["dist_t"]) > 0 and float(g["dist_sig"]) > 0
        assert gap_indices(g["tv"]) == c["gaps"]
        if c["ppm"]:
            assert c["p"]["isNyquist"] is False or sum(len(q) for q in c["gaps"]) >= 1


def gap_indices(tv):
    tv = np.asarray(tv)
    return [np.nonzero(np.abs(np.diff(tv[:, k])) > 0.5)[0].tolist() for k in range(tv.shape[1])]


# ---- the calls the fixtures record, on any implementation `m` of the public interface (the package, or Emu below)
def run_interp(m, g, x=None):
    c = g["cfg"]
    np.random.seed(c["seed"])
    return m.clockSamplingInterp(g["x"] if x is None else x, c["inFs"], c["outFs"], c["jitter_s"])


def run_quant(m, g, x=None):
    c = g["cfg"]
    return m.quantizer(g["x"] if x is None else x, c["nBits"], c["maxV"], c["minV"])


def run_conv(m, g, sig=None):
    c = g["cfg"]
    sig = g["sigIn"] if sig is None else sig
    np.random.seed(c["seed"])
    if c["fn"] == "pair":
        mid = m.dac(sig, Param(**c["p"]["dac"]))
        return m.adc(mid, Param(Vmax=c["written"]["Vmax"], Vmin=c["written"]["Vmin"], **c["p"]["adc"]))
    return getattr(m, c["fn"])(sig, Param(**c["p"]))


def run_gardner(m, g, x=None):
    return m.gardnerClockRecovery(g["x"] if x is None else x, Param(**g["cfg"]["p"]))


def check_conv(name, g, out):
    """A converter's output against the reference's: bit-equal with the filters off, within k FIR_REL max |ref| with them on."""
    out, ref = np.asarray(out), g["out"]
    assert out.shape == ref.shape and out.dtype == ref.dtype, (out.shape, out.dtype, ref.shape, ref.dtype)
    k = FILTERS.get(name, 0)
    if not k:
        assert np.array_equal(out, ref)
        return 0.0
    d = float(np.max(np.abs(out - ref)) / np.max(np.abs(ref)))
    assert d <= k * FIR_REL, (name, d)
    return d


def check_gardner(g, out, tv):
    """A clock recovery result for the fixture's signal: bit-equal to the restatement, near the reference's recorded run."""
    c = g["cfg"]["p"]
    want, tvw, info = restated(g)
    out, tv = np.asarray(out), np.asarray(tv)
    assert out.dtype == np.complex64 and tv.dtype == np.float64
    assert out.shape == want.shape == g["out"].shape and tv.shape == tvw.shape == g["tv"].shape
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and np.array_equal(tv.view(np.uint64), tvw.view(np.uint64))
    assert gap_indices(tv) == g["cfg"]["gaps"]
    spacing = float(np.spacing(np.float32(np.max(np.abs(want)))))
    dist_sig = float(np.max(np.abs(out.astype(np.complex128) - g["out"].astype(np.complex128))) / spacing)
    dist_t = float(np.max(np.abs(tv - g["tv"])))
    assert dist_sig <= 2 * float(g["dist_sig"]) and dist_t <= 2 * float(g["dist_t"]), (dist_sig, dist_t, c)
    return dict(dist_sig=dist_sig, dist_t=dist_t)


_RESTATED = {}


def restated(g):
    """The restatement's run of a clock recovery fixture, computed once."""
    key = g["cfg"]["name"]
    if key not in _RESTATED:
        p = g["cfg"]["p"]
        _RESTATED[key] = rs.gardner(g["x"], p["kp"], p["ki"], p["isNyquist"], p["lpad"], p["maxPPM"])
    return _RESTATED[key]


def chain_signal(oa):
    """The chain test's signal with this package's own functions: 16-QAM symbols (CHAIN_SEED), raised cosine of roll-off 0.05 at 4
    samples per symbol, dac at the nominal clock, the symbols; the adc that follows runs 300 ppm fast (chain_adc_param)."""
    np.random.seed(CHAIN_SEED)
    bits = np.random.randint(2, size=4 * CHAIN_SYMBOLS * 2)
    symb = np.asarray(oa.pnorm(oa.modulateGray(bits, 16, "qam"))).reshape(-1, 2)
    up = np.zeros((4 * len(symb), 2), dtype=np.complex128)
    up[::4] = symb
    pulse = oa.pulseShape(Param(SpS=4, nFilterTaps=1024, rollOff=0.05, pulseType="rc"))
    sig = oa.pnorm(oa.firFilter(pulse, up))
    np.random.seed(CHAIN_SEED + 1)
    mid = oa.dac(sig, Param(inFs=FS, outFs=FS, nBits=8, ENOB=8, Vpp=2, AIF=True))
    return mid, symb


def chain_adc_param(mid):
    return Param(inFs=FS, outFs=2 * 32e9 * (1 + 300 / 1e6), nBits=8, ENOB=8, Vmax=float(np.max(mid.real)), Vmin=float(np.min(mid.real)),
                 AAF=True, N=1001)


# ---- the emulator (tests/emu/emu_clock.cpp)
def build_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_clock") / "emu_clock"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_clock.cpp"), "-o", str(exe)])
    return str(exe)


def emu_constants(exe):
    v = [int(s) for s in subprocess.check_output([exe, "const"]).split()]
    return dict(zip(("chunk", "win", "ring", "flush", "lag", "block", "max_blocks"), v))


class Emu:
    """The public interface with the kernels walked on the CPU: the host side is the package's own (clock.py's checks, tables, times
    and draws); ``firFilter`` has no emulator, so a converter with its filters on is not offered."""

    def __init__(self, exe, tmp):
        self.exe, self.tmp = exe, tmp

    def _run(self, op, ints, floats, arrays, out_specs):
        I = np.zeros(16, dtype=np.int64)
        D = np.zeros(8, dtype=np.float64)
        I[:len(ints)], D[:len(floats)] = ints, floats
        with open(self.tmp / "in.bin", "wb") as f:
            f.write(I.tobytes())
            f.write(D.tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([self.exe, op, str(self.tmp / "in.bin"), str(self.tmp / "out.bin")])
        raw = open(self.tmp / "out.bin", "rb").read()
        outs, off = [], 0
        for dtype, shape in out_specs:
            nb = int(np.prod(shape)) * np.dtype(dtype).itemsize
            outs.append(np.frombuffer(raw[off:off + nb], dtype=dtype).reshape(shape).copy())
            off += nb
        assert off == len(raw), (off, len(raw))
        return outs

    def _interp(self, x, inFs, outFs, form, **kw):
        q = clock._plan_interp(x, inFs, outFs, form, **kw)
        p = q["params"]
        if not p.n_out:
            return np.empty(q["shape"], dtype=q["dtype"])
        times = [t for t in (q["t_re"], q["t_im"]) if t is not None]
        return self._run("chain", [p.n_in, p.n_out, p.ncols, p.dtype, p.form, p.clip, p.quantize, p.qlevels, q["t_re"] is not None,
                                   q["t_im"] is not None], [p.inTs, p.outTs, p.lo, p.hi, p.qmin, p.qdelta], [x] + times,
                         [(q["dtype"], q["shape"])])[0]

    def clockSamplingInterp(self, x, inFs, outFs, jitter=0):
        x = clock._two_d(clock._array(x, "x"), "x")
        t = clock.output_times(x.shape[0], 1 / inFs, 1 / outFs, jitter)
        return self._interp(x, inFs, outFs, _lib.CLOCK_COMPLEX if x.dtype.kind == "c" else _lib.CLOCK_REAL, t_re=t)

    def _quantize_flat(self, x, code, count, table, shape):
        return self._run("quantize", [count, code, table[2]], [table[0], table[1]], [x], [(np.float64, shape)])[0]

    def quantizer(self, x, nBits=16, maxV=1, minV=-1):
        x = clock._two_d(clock._array(x, "x"), "x")
        return self._quantize_flat(x, _lib.METRICS_DTYPES[x.dtype.name], x.size, clock.quant_table(nBits, maxV, minV), x.shape)

    def clip(self, x, lo, hi):
        lo, hi = clock._bounds(x, lo, hi)
        return self._run("clip", [x.size, _lib.METRICS_DTYPES[x.dtype.name]], [lo, hi], [x], [(x.dtype, x.shape)])[0]

    def minmax(self, x):
        r = self._run("minmax", [x.size, _lib.METRICS_DTYPES[x.dtype.name]], [], [x], [(np.float64, (2,))])[0]
        return float(r[0]), float(r[1])

    def adc(self, sigIn, prm):
        assert prm.AAF is False
        x, _ = clock._composite_input(sigIn, "sigIn")
        cplx = x.dtype.kind == "c"
        inTs, outTs = 1 / prm.inFs, 1 / prm.outFs
        jitter, nBits, ENOB = getattr(prm, "jitter", 0), prm.nBits, prm.ENOB
        t_re = clock.output_times(x.shape[0], inTs, outTs, jitter)
        t_im = clock.output_times(x.shape[0], inTs, outTs, jitter) if cplx else None
        out = self._interp(x, prm.inFs, prm.outFs, _lib.CLOCK_COMPONENTS if cplx else _lib.CLOCK_REAL, t_re=t_re, t_im=t_im,
                           clip=(prm.Vmin, prm.Vmax), quant=clock.quant_table(nBits, prm.Vmax, prm.Vmin))
        if nBits > ENOB:
            out = out + clock._extra_noise(out.shape, cplx, prm.Vmax - prm.Vmin, nBits, ENOB)
        return out.flatten() if out.shape[1] == 1 else out

    def dac(self, sigIn, prm):
        assert prm.AIF is False and prm.nBits <= prm.ENOB
        x, _ = clock._composite_input(sigIn, "sigIn", ("complex128", "float64"))
        cplx = x.dtype.kind == "c"
        Vmin, Vmax = self.minmax(x)
        table = clock.quant_table(prm.nBits, Vmax, Vmin)
        flat = x.view(np.float64) if cplx else x
        out = self._quantize_flat(flat, _lib.METRICS_DTYPES["float64"], flat.size, table, flat.shape)
        out = out.view(np.complex128) if cplx else out
        jitter = getattr(prm, "jitter", 0)
        t_re = clock.output_times(x.shape[0], 1 / prm.inFs, 1 / prm.outFs, jitter)
        t_im = clock.output_times(x.shape[0], 1 / prm.inFs, 1 / prm.outFs, jitter) if cplx else None
        out = self._interp(out, prm.inFs, prm.outFs, _lib.CLOCK_COMPONENTS if cplx else _lib.CLOCK_REAL, t_re=t_re, t_im=t_im)
        out = (out.view(np.float64) * (prm.Vpp / (Vmax - Vmin))).view(out.dtype)
        return out.flatten() if out.shape[1] == 1 else out

    def gardner_raw(self, sigIn, prm=None):
        """(full signal, timing values, last_n per mode, status per mode) as the kernel leaves them."""
        q = clock._prepare_gardner(sigIn, prm)
        p, x = q["params"], q["x"]
        return self._run("gardner", [p.n, p.lpad, p.Ln, p.nModes, p.dtype, p.nyquist], [p.kp, p.ki], [x],
                         [(np.complex64, (p.Ln, p.nModes)), (np.float64, (p.Ln, p.nModes)), (np.int64, (p.nModes,)), (np.int32, (p.nModes,))]) + [q]

    def gardnerClockRecovery(self, sigIn, prm=None):
        full, tv, last, status, q = self.gardner_raw(sigIn, prm)
        assert not np.any(status)
        out = full[0:min(max(0, int(np.max(last))), q["Ln"]), :]
        if q["input1D"]:
            out = out.flatten()
        return (out, tv) if q["returnTiming"] else out

    def calcClockDrift(self, t, per_column=0):
        t = np.asarray(t, dtype=np.float64)
        t = t.reshape(len(t), 1) if t.ndim == 1 else t
        return self._run("drift", [t.shape[0], t.shape[1], per_column], [], [t], [(np.float64, (t.shape[1],))])[0]
