"""The sampling clock on the device: the converters that put a clock offset on a signal and the stage that takes it off again.

Drop-ins for ``clockSamplingInterp``, ``quantizer`` and ``resample`` (optic/dsp/core.py:272-349, 494-549), ``adc`` and ``dac``
(optic/models/devices.py:793-1022) and ``gardnerClockRecovery`` / ``calcClockDrift`` with the scalar helpers ``gardnerTED``,
``gardnerTEDnyquist`` and ``interpolator`` (optic/dsp/clockRecovery.py).  Arguments are numpy arrays or ``DeviceArray``s; a
``DeviceArray`` in gives ``DeviceArray``s out and the field never leaves device memory: what crosses the bus are the few numbers a
call needs on the host (``dac``'s minimum and maximum, the output length of the clock recovery) and the random draws the reference
makes on the host (jitter, the ``ENOB`` noise), uploaded once.  There is no CPU fallback: numpy arguments take the same kernels.

Types.  ``clockSamplingInterp`` and ``quantizer`` take complex128, complex64, float64 and float32; ``resample``, ``adc`` and
``dac`` compose the device ``firFilter`` and take a complex128 ``DeviceArray`` (numpy input of any of the four types follows the
reference's branches for it, real in, real out; ``dac`` takes double precision only); ``gardnerClockRecovery`` takes complex128 or
complex64 and returns a complex64 signal and float64 timing values.  Anything else raises ``TypeError`` / ``ValueError`` before
anything is allocated.

The converters reproduce numpy bit for bit (opticommpy_amd/csrc/clock_kernels.h states every expression), including these habits
of the reference:

* ``adc`` clips complex samples with ``np.clip(z, Vmin + 1j Vmin, Vmax + 1j Vmax)``, numpy's *lexicographic* order of complex
  numbers: a sample whose real part is below ``Vmin`` becomes ``Vmin + 1j Vmin`` entirely, one whose real part is strictly inside
  is not clipped in its imaginary part at all (the quantizer's rails then bound it);
* with complex input and jitter the real and the imaginary parts get *different* jitter draws (two draws, the real parts' first);
* the quantizer's table is ``np.arange(minV, maxV + D, D)``: its step is ``(minV + D) - minV``, which need not equal ``D`` in the
  last bit, and it may hold ``2 ** nBits + 1`` levels;
* ``resample`` returns 1-D for 1-D input, ``adc`` and ``dac`` for every one-column input.

Random draws come from numpy's global state in the reference's order, so a caller who seeds ``np.random`` gets the reference's run.

Deviations, on purpose: ``quantizer`` on complex input quantises the real part (the reference takes the complex distance to the
real levels, which decides the same level except where rounding makes a tie); ``gardnerClockRecovery`` keeps its state in double
and evaluates the detector in double on the stored (single-precision) outputs, as tests/clock_restatement.py states; where a
negative clock gap takes the output index to the end of the output the reference writes a timing value out of bounds, here that
write is dropped; where the loop falls back to output 0 the reference raises, here the column ends.
"""
import ctypes as C
import logging as logg
import math

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["clockSamplingInterp", "quantizer", "resample", "adc", "dac", "gardnerClockRecovery", "calcClockDrift", "gardnerTED",
           "gardnerTEDnyquist", "interpolator"]

_DTYPES = tuple(_lib.METRICS_DTYPES)
_COMPLEX = ("complex128", "complex64")
MAX_BITS = 32


# ------------------------------------------------------------------------------------ host-side quantities
def _array(x, name, dtypes=_DTYPES):
    """The argument as the kernels take it: a DeviceArray of one of ``dtypes`` as it is, anything else as a numpy array of one."""
    if _dev.is_device(x):
        if x.dtype.name not in dtypes:
            raise TypeError(f"device array {name} has dtype {x.dtype.name}: {', '.join(dtypes)} expected")
        return x
    x = np.asarray(x)
    if x.dtype.name not in dtypes:
        if x.dtype.kind not in "biufc":
            raise TypeError(f"{name} has dtype {x.dtype.name}: a numeric array is expected")
        wide = "complex128" if x.dtype.kind == "c" else "float64"
        if wide not in dtypes:
            wide = dtypes[0]
        x = x.astype(wide)
    return x


def _two_d(x, name):
    if x.ndim != 2:
        raise ValueError(f"{name} must have two dimensions (samples, modes), as in the reference; it has {x.ndim}")
    if x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{name} has shape {tuple(x.shape)}: at least one sample and one mode are needed")
    return x


def _columns(x, name):
    """(2-D array, was 1-D): the reference's ``sigIn.reshape(len(sigIn), 1)``."""
    if x.ndim == 1:
        return x.reshape(x.shape[0], 1), True
    return _two_d(x, name), False


def _rates(inFs, outFs):
    for name, v in (("inFs", inFs), ("outFs", outFs)):
        if not np.isfinite(v) or not v > 0:
            raise ValueError(f"{name} = {v}: a sampling frequency must be positive")
    return 1 / inFs, 1 / outFs


def output_length(N, inTs, outTs):
    """len(np.arange(0, N * inTs, outTs)): numpy's own rule, in double."""
    return max(int(math.ceil((N * inTs - 0) / outTs)), 0)


def _check_jitter(jitter):
    if not np.isfinite(jitter) or jitter < 0:
        raise ValueError(f"jitter = {jitter}: a standard deviation cannot be negative")


def output_times(N, inTs, outTs, jitter):
    """The output times with one jitter draw from numpy's global state (None without jitter: the kernel computes i * outTs)."""
    _check_jitter(jitter)
    if not jitter > 0:
        return None
    tout = np.arange(0, N * inTs, outTs)
    tout += np.random.normal(0, jitter, tout.shape)
    return tout


def quant_table(nBits, maxV, minV):
    """(qmin, qdelta, levels) of ``d = np.arange(minV, maxV + D, D)``, D = (maxV - minV) / (2 ** nBits - 1): d[i] = qmin + i qdelta."""
    if int(nBits) != nBits or nBits < 1 or nBits > MAX_BITS:
        raise ValueError(f"nBits = {nBits}: an integer between 1 and {MAX_BITS} is expected")
    maxV, minV = float(maxV), float(minV)
    if not (np.isfinite(maxV) and np.isfinite(minV)) or not maxV > minV:
        raise ValueError(f"maxV = {maxV}, minV = {minV}: finite values with maxV > minV are expected")
    D = (maxV - minV) / (2 ** int(nBits) - 1)
    levels = int(math.ceil(((maxV + D) - minV) / D))
    return minV, (minV + D) - minV, levels


def _bounds(x, lo, hi):
    """Clip bounds as numpy takes Python scalars: in the array's own precision."""
    kind = np.float32 if x.dtype.name in ("complex64", "float32") else np.float64
    return float(kind(lo)), float(kind(hi))


# ------------------------------------------------------------------------------------ the library calls
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _plan_interp(x, inFs, outFs, form, t_re=None, t_im=None, clip=None, quant=None):
    """Every host-side quantity of one interpolation pass (nothing is launched): ``params`` (``_lib.ClockParams``), the times, the
    output's shape and dtype."""
    inTs, outTs = _rates(inFs, outFs)
    N, ncols = int(x.shape[0]), int(x.shape[1])
    n_out = output_length(N, inTs, outTs)
    for t in (t_re, t_im):
        assert t is None or (t.dtype == np.float64 and t.shape == (n_out,))
    p = _lib.ClockParams(n_in=N, n_out=n_out, ncols=ncols, dtype=_lib.METRICS_DTYPES[x.dtype.name], form=form, inTs=inTs, outTs=outTs,
                         qlevels=1, qdelta=1.0)
    out_dtype = x.dtype
    if clip is not None:
        p.clip, (p.lo, p.hi) = 1, _bounds(x, *clip)
        if not p.lo <= p.hi:
            raise ValueError(f"Vmin = {clip[0]}, Vmax = {clip[1]}: Vmin <= Vmax is expected")
    if quant is not None:
        p.quantize, (p.qmin, p.qdelta, p.qlevels) = 1, quant
        out_dtype = np.dtype(np.complex128 if x.dtype.kind == "c" else np.float64)
    return dict(params=p, t_re=t_re, t_im=t_im, shape=(n_out, ncols), dtype=np.dtype(out_dtype))


def _interp(x, inFs, outFs, form, **kw):
    from .models import _state
    q = _plan_interp(x, inFs, outFs, form, **kw)
    lib = _lib.load()
    out = _dev.empty(_dev.is_device(x), q["shape"], q["dtype"])
    if q["shape"][0]:
        xp, keep = _dev.arg(x, x.dtype)
        rc = lib.ssf_clock_interp(_state["device"], C.byref(q["params"]), xp, _ptr(q["t_re"]), _ptr(q["t_im"]), _dev.out_ptr(out))
        _lib.raise_for(lib, None, rc)
        del keep
    return out


def _quantize(x, table):
    """Every real value of x (the components of complex data) to its nearest level: float64 / complex128 of x's shape."""
    from .models import _state
    lib = _lib.load()
    cplx = x.dtype.kind == "c"
    single = x.dtype.name in ("complex64", "float32")
    out = _dev.empty(_dev.is_device(x), x.shape, np.complex128 if cplx else np.float64)
    xp, keep = _dev.arg(x, x.dtype)
    rc = lib.ssf_quantize(_state["device"], x.size * (2 if cplx else 1), _lib.METRICS_DTYPES["float32" if single else "float64"],
                          table[0], table[1], table[2], xp, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


def _minmax(x):
    from .models import _state
    lib = _lib.load()
    res = (C.c_double * 2)()
    xp, keep = _dev.arg(x, x.dtype)
    _lib.raise_for(lib, None, lib.ssf_minmax(_state["device"], x.size, _lib.METRICS_DTYPES[x.dtype.name], xp, res))
    del keep
    return res[0], res[1]


def _scale_add(x, noise=None, scale=None):
    """(x + noise) * scale on float64 / complex128 data, either part optional; noise is a host array."""
    from .models import _state
    lib = _lib.load()
    out = _dev.empty(_dev.is_device(x), x.shape, x.dtype)
    xp, keep = _dev.arg(x, x.dtype)
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=x.dtype)
        assert noise.shape == tuple(x.shape)
    rc = lib.ssf_clock_scale_add(_state["device"], x.size * (2 if x.dtype.kind == "c" else 1), 1.0 if scale is None else float(scale),
                                 scale is not None, xp, _ptr(noise), _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


def _flat(x):
    return x.reshape(-1) if _dev.is_device(x) else x.flatten()


# ------------------------------------------------------------------------------------ element-wise functions
def clockSamplingInterp(x, inFs, outFs, jitter=0):
    """Interpolate the columns of ``x`` (2-D) to the sampling rate ``outFs`` (optic/dsp/core.py:272-314): ``np.interp`` at the
    times ``arange(0, N / inFs, 1 / outFs)``, to which ``jitter > 0`` adds one ``np.random.normal(0, jitter)`` draw from numpy's
    global state.  The result has ``x``'s dtype."""
    x = _two_d(_array(x, "x"), "x")
    inTs, outTs = _rates(inFs, outFs)
    t = output_times(x.shape[0], inTs, outTs, jitter)
    return _interp(x, inFs, outFs, _lib.CLOCK_COMPLEX if x.dtype.kind == "c" else _lib.CLOCK_REAL, t_re=t)


def quantizer(x, nBits=16, maxV=1, minV=-1):
    """Uniform quantizer (optic/dsp/core.py:317-349): every value of ``x`` (2-D) to the nearest of the levels
    ``np.arange(minV, maxV + D, D)``, ``D = (maxV - minV) / (2 ** nBits - 1)``, the lower one on a tie.  float64 whatever the input;
    of complex input the real part is quantised."""
    x = _two_d(_array(x, "x"), "x")
    table = quant_table(nBits, maxV, minV)
    from .models import _state
    lib = _lib.load()
    out = _dev.empty(_dev.is_device(x), x.shape, np.float64)
    xp, keep = _dev.arg(x, x.dtype)
    rc = lib.ssf_quantize(_state["device"], x.size, _lib.METRICS_DTYPES[x.dtype.name], table[0], table[1], table[2], xp, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


# ------------------------------------------------------------------------------------ composites
def _composite_input(sigIn, name, dtypes=_DTYPES):
    if _dev.is_device(sigIn) and sigIn.dtype.name != "complex128":
        raise TypeError(f"device array {name} has dtype {sigIn.dtype.name}: the filters of this call take complex128")
    x = _array(sigIn, name, dtypes)
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must have one or two dimensions")
    return _columns(x, name)


def _form(x):
    return _lib.CLOCK_COMPLEX if x.dtype.kind == "c" else _lib.CLOCK_REAL


def resample(sigIn, param):
    """Resample to ``param.outFs`` (optic/dsp/core.py:494-549): anti-aliasing ``firFilter`` ahead of the interpolation when the
    rate falls, behind it when it rises.  Parameters: N (501), inFs (2), outFs (2)."""
    from .rx import firFilter, lowPassFIR
    N = getattr(param, "N", 501)
    inFs = getattr(param, "inFs", 2)
    outFs = getattr(param, "outFs", 2)
    x, input1D = _composite_input(sigIn, "sigIn")
    _rates(inFs, outFs)
    if int(N) != N or N < 1:
        raise ValueError(f"N = {N}: the filters need at least one tap")
    if outFs < inFs:
        x = firFilter(lowPassFIR(outFs / 2, inFs, min(x.shape[0], int(N)), typeF="rect"), x)
    out = _interp(x, inFs, outFs, _form(x))
    if outFs > inFs and out.shape[0]:
        out = firFilter(lowPassFIR(inFs / 2, outFs, min(out.shape[0], int(N)), typeF="rect"), out)
    return _flat(out) if input1D else out


def _extra_noise(shape, cplx, scale, nBits, ENOB):
    """The noise that models ENOB < nBits, drawn as the reference draws it (devices.py:894-903)."""
    Pnq_ideal = scale ** 2 / (12 * (2 ** (2 * nBits)))
    Pnq_actual = scale ** 2 / (12 * (2 ** (2 * ENOB)))
    Pn_extra = Pnq_actual - Pnq_ideal
    if cplx:
        from .models import gaussianComplexNoise
        return gaussianComplexNoise(shape, 2 * Pn_extra)
    return np.random.normal(0, np.sqrt(Pn_extra), shape)


def adc(sigIn, param):
    """Analog-to-digital converter (optic/models/devices.py:793-909): anti-aliasing filter, interpolation to ``outFs`` with
    jitter, clip to [Vmin, Vmax], ``nBits`` quantizer, anti-aliasing filter, the noise of ``ENOB < nBits``.  Interpolation, clip
    and quantizer are one pass over the data.  Defaults are written back to ``param`` as the reference does: inFs (1), outFs (1),
    jitter (0), nBits (8), ENOB (8), Vmax (1), Vmin (-1), AAF (True), N (201)."""
    from .rx import firFilter, lowPassFIR
    for name, default in (("inFs", 1), ("outFs", 1), ("jitter", 0), ("nBits", 8), ("ENOB", 8), ("Vmax", 1), ("Vmin", -1), ("AAF", True),
                          ("N", 201)):
        setattr(param, name, getattr(param, name, default))
    inFs, outFs, jitter, nBits, Vmax, Vmin, AAF, N, ENOB = (param.inFs, param.outFs, param.jitter, param.nBits, param.Vmax, param.Vmin,
                                                            param.AAF, param.N, param.ENOB)
    if ENOB > nBits:
        logg.warning("ADC ENOB is greater than ADC nBits. The effective number of bits (ENOB) should be less than or equal to the "
                     "number of bits (nBits) for a consistent ADC model.")
    x, _ = _composite_input(sigIn, "sigIn")
    inTs, outTs = _rates(inFs, outFs)
    _check_jitter(jitter)
    table = quant_table(nBits, Vmax, Vmin)
    if AAF and (int(N) != N or N < 1):
        raise ValueError(f"N = {N}: the filters need at least one tap")
    if AAF:
        Ntaps = min(x.shape[0], int(N))
        hi = lowPassFIR(outFs / 2, inFs, Ntaps, typeF="rect")
        ho = lowPassFIR(outFs / 2, outFs, Ntaps, typeF="rect")
        x = firFilter(hi, x)
    cplx = x.dtype.kind == "c"
    t_re = output_times(x.shape[0], inTs, outTs, jitter)
    t_im = output_times(x.shape[0], inTs, outTs, jitter) if cplx else None        # a second draw for the imaginary parts
    out = _interp(x, inFs, outFs, _lib.CLOCK_COMPONENTS if cplx else _lib.CLOCK_REAL, t_re=t_re, t_im=t_im, clip=(Vmin, Vmax), quant=table)
    if AAF and out.shape[0]:
        out = firFilter(ho, out)
    if nBits > ENOB and out.shape[0]:
        out = _scale_add(out, noise=_extra_noise(tuple(out.shape), cplx, Vmax - Vmin, nBits, ENOB))
    return _flat(out) if out.shape[1] == 1 else out


def dac(sigIn, param):
    """Digital-to-analog converter (optic/models/devices.py:912-1022): ``nBits`` quantizer between the signal's own minimum and
    maximum (over real and imaginary parts), interpolation to ``outFs`` with jitter, anti-imaging filter, the noise of
    ``ENOB < nBits``, scaling to ``Vpp``.  Defaults written back: inFs (1), outFs (1), nBits (8), ENOB (8), jitter (0), Vpp (2),
    AIF (True), N (201)."""
    from .rx import firFilter, lowPassFIR
    for name, default in (("inFs", 1), ("outFs", 1), ("nBits", 8), ("ENOB", 8), ("jitter", 0), ("Vpp", 2), ("AIF", True), ("N", 201)):
        setattr(param, name, getattr(param, name, default))
    inFs, outFs, nBits, ENOB, jitter, Vpp, AIF, N = (param.inFs, param.outFs, param.nBits, param.ENOB, param.jitter, param.Vpp, param.AIF,
                                                     param.N)
    if ENOB > nBits:
        logg.warning("DAC ENOB is greater than DAC nBits. The effective number of bits (ENOB) should be less than or equal to the "
                     "number of bits (nBits) for a consistent ADC model.")
    if not _dev.is_device(sigIn) and np.asarray(sigIn).dtype.name in ("complex64", "float32"):
        raise TypeError("dac takes double precision (complex128 or float64): the reference builds a single-precision signal's "
                        "quantizer table in single precision, which is not reproduced")
    x, _ = _composite_input(sigIn, "sigIn", ("complex128", "float64"))
    inTs, outTs = _rates(inFs, outFs)
    _check_jitter(jitter)
    quant_table(nBits, 1, 0)
    if AIF and (int(N) != N or N < 1):
        raise ValueError(f"N = {N}: the filters need at least one tap")
    Vmin, Vmax = _minmax(x)
    out = _quantize(x, quant_table(nBits, Vmax, Vmin))
    cplx = x.dtype.kind == "c"
    t_re = output_times(x.shape[0], inTs, outTs, jitter)
    t_im = output_times(x.shape[0], inTs, outTs, jitter) if cplx else None
    out = _interp(out, inFs, outFs, _lib.CLOCK_COMPONENTS if cplx else _lib.CLOCK_REAL, t_re=t_re, t_im=t_im)
    if not out.shape[0]:
        return _flat(out) if out.shape[1] == 1 else out
    if AIF:
        out = firFilter(lowPassFIR(outFs / 2, outFs, min(out.shape[0], int(N)), typeF="rect"), out)
    noise = _extra_noise(tuple(out.shape), cplx, Vmax - Vmin, nBits, ENOB) if nBits > ENOB else None
    out = _scale_add(out, noise=noise, scale=Vpp / (Vmax - Vmin))
    return _flat(out) if out.shape[1] == 1 else out


# ------------------------------------------------------------------------------------ clock recovery
def gardnerTED(x):
    """Gardner timing error detector on three samples (optic/dsp/clockRecovery.py:24-39).  A plain host function."""
    return np.real(np.conj(x[1]) * (x[2] - x[0]))


def gardnerTEDnyquist(x):
    """Modified Gardner timing error detector for Nyquist pulses (optic/dsp/clockRecovery.py:42-57).  A plain host function."""
    return np.abs(x[1]) ** 2 * (np.abs(x[0]) ** 2 - np.abs(x[2]) ** 2)


def interpolator(x, t):
    """Cubic interpolation of four samples with the Farrow structure (optic/dsp/clockRecovery.py:60-82).  A plain host function."""
    return (x[0] * (-1 / 6 * t ** 3 + 1 / 6 * t) + x[1] * (1 / 2 * t ** 3 + 1 / 2 * t ** 2 - 1 * t)
            + x[2] * (-1 / 2 * t ** 3 - 1 * t ** 2 + 1 / 2 * t + 1) + x[3] * (1 / 6 * t ** 3 + 1 / 2 * t ** 2 + 1 / 3 * t))


def _prepare_gardner(sigIn, param=None):
    """Every check and every host-side quantity of a call, without touching the library."""
    kp = getattr(param, "kp", 1e-3)
    ki = getattr(param, "ki", 1e-6)
    isNyquist = getattr(param, "isNyquist", True)
    returnTiming = getattr(param, "returnTiming", False)
    lpad = getattr(param, "lpad", 1)
    maxPPM = getattr(param, "maxPPM", 500)
    x = _array(sigIn, "sigIn", _COMPLEX)
    if x.ndim not in (1, 2):
        raise ValueError("sigIn must have one or two dimensions")
    x, input1D = _columns(x, "sigIn")
    if int(lpad) != lpad or lpad < 0:
        raise ValueError(f"lpad = {lpad}: the number of padded zeros must be a non-negative integer")
    for name, v in (("kp", kp), ("ki", ki), ("maxPPM", maxPPM)):
        if not np.isfinite(v):
            raise ValueError(f"{name} = {v} must be finite")
    n, nModes = int(x.shape[0]), int(x.shape[1])
    if nModes > 65535:
        raise ValueError(f"sigIn has {nModes} modes: at most 65535 are recovered in one call")
    nSamples = n + int(lpad)
    Ln = int((1 - maxPPM / 1e6) * nSamples)
    if Ln < 1:
        raise ValueError(f"maxPPM = {maxPPM} leaves no output for {nSamples} samples")
    p = _lib.GardnerParams(n=n, lpad=int(lpad), Ln=Ln, nModes=nModes, dtype=_lib.METRICS_DTYPES[x.dtype.name], nyquist=bool(isNyquist),
                           kp=float(kp), ki=float(ki))
    return dict(x=x, params=p, input1D=input1D, returnTiming=bool(returnTiming), Ln=Ln, nModes=nModes)


def _drift(t, per_column):
    from .models import _state
    lib = _lib.load()
    ppm = np.empty(t.shape[1], dtype=np.float64)
    tp, keep = _dev.arg(t, np.float64)
    rc = lib.ssf_clock_drift(_state["device"], t.shape[0], t.shape[1], per_column, tp, ppm.ctypes.data_as(C.POINTER(C.c_double)))
    _lib.raise_for(lib, None, rc)
    del keep
    return ppm


def gardnerClockRecovery(sigIn, param=None):
    """Clock recovery with Gardner's algorithm and a PI loop filter (optic/dsp/clockRecovery.py:85-191), one wavefront per mode.

    Parameters read from ``param`` with the reference's defaults: kp (1e-3), ki (1e-6), isNyquist (True), returnTiming (False),
    lpad (1), maxPPM (500).  Returns the recovered signal (complex64, cut to the furthest output any mode reached; 1-D for 1-D
    input), with ``returnTiming`` also the timing values (float64, ``(Ln, nModes)``, not cut)."""
    from .models import _state
    q = _prepare_gardner(sigIn, param)
    lib = _lib.load()
    x, Ln, nModes = q["x"], q["Ln"], q["nModes"]
    on_dev = _dev.is_device(x)
    xp, keep = _dev.arg(x, x.dtype)
    full = _dev.empty(on_dev, (Ln, nModes), np.complex64)
    t_nco = _dev.empty(on_dev, (Ln, nModes), np.float64)
    last = (C.c_int64 * nModes)()
    rc = lib.ssf_gardner(_state["device"], C.byref(q["params"]), xp, _dev.out_ptr(full), _dev.out_ptr(t_nco), last)
    _lib.raise_for(lib, None, rc)
    del keep
    rows = min(max(0, max(last)), Ln)
    if on_dev:
        out = _dev.DeviceArray((rows, nModes), np.complex64)
        if rows:
            _lib.raise_for(lib, None, lib.ssf_device_memcpy(_state["device"], out.ptr, full.ptr, out.nbytes))
    else:
        out = full[0:rows, :]
    if logg.getLogger().isEnabledFor(logg.INFO):
        logg.info("Running clock recovery...")
        for k, ppm in enumerate(_drift(t_nco, 1)):
            logg.info(f"Estimated clock drift mode {k}: {ppm:.2f} ppm")
    if q["input1D"]:
        out = _flat(out)
    return (out, t_nco) if q["returnTiming"] else out


def calcClockDrift(t_nco_values):
    """Clock drift in ppm from the timing values (optic/dsp/clockRecovery.py:194-232): per column, the mean distance of the clock
    gaps (the peaks of ``|diff(t - mean(t))|`` of height >= 0.5, by ``scipy.signal.find_peaks``' rule) and the sign of the mean
    over all columns; ``nan`` with fewer than two gaps.  A numpy array of one value per column."""
    t = _array(t_nco_values, "t_nco_values", ("float64",))
    if t.ndim not in (1, 2):
        raise ValueError("t_nco_values must have one or two dimensions")
    t, _ = _columns(t, "t_nco_values")
    return _drift(t, 0)
