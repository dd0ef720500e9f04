"""Adaptive equalizers of the direct-detection chain on the device: ffe, dfe, volterra.

Drop-in for ``ffe``, ``dfe`` and ``volterra`` (optic/dsp/equalization.py:1176-2143 with their numba cores), the stage between
``pnorm`` and ``fastBERcalc`` in the reference's IM/DD chain ``photodiode -> resample -> pnorm -> ffe | dfe | volterra ->
fastBERcalc``.  One library call (``ssf_siso_eq``, include/ssf.h) runs a whole equalizer on the GPU: a ``DeviceArray`` in gives a
``DeviceArray`` out and nothing the size of the signal crosses the bus; the coefficients always come back as host numpy arrays.

All three are one recursion, LMS over a regressor ``phi(k)``: ``y = w . phi``, ``e = r - y``, ``w += mu_s e conj(phi)``, with ``r``
the training symbol while ``k < nTrain`` and otherwise the nearest point of the table (the first minimum in table order).  One
wavefront walks every symbol that adapts or feeds a later decision with the coefficients in registers; for ``ffe`` and ``volterra``
in 'data-aided' mode the symbols behind ``nTrain`` of the last pass run one per thread with the coefficients fixed
(opticommpy_amd/csrc/engine_siso.hip).  ``last_call`` says which kernel took how many symbols.

Arguments are 1-D numpy arrays or ``DeviceArray``s, float64 / float32 for real data and complex128 / complex64 for complex data;
``sigIn`` and ``symbRef`` are both real or both complex.  Inputs are never written.

Scope and limits (anything else raises ``ValueError`` / ``TypeError`` before anything is launched or allocated; there is no CPU
fallback):

* at most 1536 coefficients per call (24 per lane of the wavefront): ``nTaps`` | ``nTapsFF + nTapsFB`` | ``n1Taps + n2Taps ** 2
  (+ n3Taps ** 3 at order 3)``; ``nTaps``, ``nTapsFF``, ``n1Taps`` and ``nTapsFB`` at most 256 each;
* 1 <= ``SpS`` <= 8 and ``SpS`` <= ``nTaps`` (the reference indexes out of range beyond), ``n >= SpS``;
* ``n1Taps >= n2Taps``, ``n1Taps >= n3Taps`` (the reference only logs and then fails), ``order`` 2 or 3;
* ``constType`` 'pam' or 'ook' for real data, 'qam' or 'psk' for complex data, ``M`` a power of two up to 1024 (the table the
  kernels stage); ``volterra`` takes real data only;
* ``prec`` one of float32, float64, complex64, complex128, real for real data and complex for complex data;
* ``preconvIters >= 1``, ``nTrain >= 0``, ``len(symbRef) >= min(nTrain, N)`` with ``N = len(sigIn) // SpS`` output symbols;
* ``trainingMode`` 'data-aided' or 'fulltime'.

Deviations from the reference, on purpose:

* arithmetic is double whatever ``prec`` says, and ``sigOut``, ``mse`` and the coefficients are float64 (complex128 for complex
  data).  ``prec`` decides the precision the constellation is built and power-normalised in, and the power-normalised ``sigIn`` and
  ``symbRef`` (for ``volterra`` also the ``anorm``-ed input) are rounded to ``prec`` before they are widened;
* the caller's ``param.f`` / ``param.b`` / ``param.h`` are never written (the reference updates them in place): the final
  coefficients are new arrays;
* ``mse`` of complex data is float64 (the reference stores it in a complex array);
* 'ook' with real data runs the real recursion (the reference sends every ``constType`` but 'pam' to its complex core);
* the nearest table point of complex data is the first minimum of ``|y - c| ** 2`` (the reference compares ``|y - c|``).
"""
import ctypes as C

import numpy as np

from . import _lib
from . import device as _dev
from .wdm_tx import grayMapping

__all__ = ["ffe", "dfe", "volterra", "last_call"]

MAX_COEFFS, MAX_TAPS, MAX_FB, MAX_SPS, MAX_M = _lib.SISO_MAX_COEFFS, _lib.SISO_MAX_TAPS, _lib.SISO_MAX_FB, _lib.SISO_MAX_SPS, _lib.SISO_MAX_M
_REAL, _COMPLEX = ("float64", "float32"), ("complex128", "complex64")

# what the last call ran: kind, serial_symbols (all passes), parallel_symbols (the frozen kernel), R (coefficient slots per lane
# of the serial kernel, 0 if it did not run), N
last_call = {}

_FROZEN = True             # measurement aid of tools/bench_siso.py: False keeps every symbol with the serial kernel


def _table(M, constType, prec):
    """The decision table with the reference's expressions in ``prec``: grayMapping(M, constType).astype(prec), then pnorm."""
    c = (np.arange(0, 2).astype(np.float32) if constType == "ook" else grayMapping(M, constType)).astype(prec)
    return c / np.sqrt(np.mean(c * np.conj(c)).real)


def _signal(x, name):
    if _dev.is_device(x):
        if x.dtype.name not in _REAL + _COMPLEX:
            raise TypeError(f"device array {name} has dtype {x.dtype.name}: float64, float32, complex128 or complex64 expected")
    else:
        x = np.asarray(x)
        if x.dtype.name not in _REAL + _COMPLEX:
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if x.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    return x


def _integer(name, v, lo, hi=None):
    if isinstance(v, (bool, np.bool_)) or int(v) != v or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} = {v}: it must be an integer " + (f"between {lo} and {hi}" if hi is not None else f"of at least {lo}"))
    return int(v)


def _coefficients(given, shape, dtype, name, spike=None):
    """A fresh array of the call's own: the caller's initial coefficients or the reference's default (a central spike or zeros)."""
    if given is None:
        a = np.zeros(shape, dtype=dtype)
        if spike is not None:
            a[spike] = 1.0
        return a
    a = np.asarray(given.get() if _dev.is_device(given) else given)
    if a.shape != tuple(shape):
        raise ValueError(f"{name} has shape {a.shape}: {tuple(shape)} expected")
    if np.iscomplexobj(a) and np.dtype(dtype).kind != "c":
        raise TypeError(f"{name} is complex but the data is real")
    return np.array(a, dtype=dtype, order="C")


def _prepare(kind, sigIn, symbRef, param):
    """Every check and every host-side quantity of a call, without touching the library."""
    g = lambda k, d: getattr(param, k, d)                                                    # noqa: E731
    if kind == "ffe":
        nTaps, nFB, mu = g("nTaps", 5), 0, g("mu", 0.0001)
    elif kind == "dfe":
        nTaps, nFB, mu = g("nTapsFF", 5), g("nTapsFB", 5), g("mu", 0.0001)
    else:
        nTaps, nFB, mu = g("n1Taps", 5), 0, g("mu", 0.001)
    n2, n3, order = (g("n2Taps", 3), g("n3Taps", 2), g("order", 2)) if kind == "volterra" else (1, 1, 2)
    SpS, nTrain, M, constType = g("SpS", 1), g("nTrain", 1000), g("M", 4), g("constType", "pam")
    mode, preconv = g("trainingMode", "data-aided"), g("preconvIters", 1)
    prec = g("prec", np.float32 if kind == "volterra" else None)

    x, ref = _signal(sigIn, "sigIn"), _signal(symbRef, "symbRef")
    cx = x.dtype.kind == "c"
    if (ref.dtype.kind == "c") != cx:
        raise TypeError(f"sigIn is {x.dtype.name} and symbRef {ref.dtype.name}: both must be real or both complex")
    prec = np.dtype(x.dtype if prec is None else prec)
    if prec.name not in _REAL + _COMPLEX:
        raise ValueError(f"prec must be float32, float64, complex64 or complex128, not {prec.name}")
    if kind == "volterra" and (cx or prec.kind == "c"):
        raise TypeError("volterra takes real data and a real prec")
    if (prec.kind == "c") != cx:
        raise TypeError(f"prec = {prec.name} with {'complex' if cx else 'real'} data")
    if constType not in ("pam", "ook", "qam", "psk"):
        raise ValueError(f"constType must be 'pam', 'ook', 'qam' or 'psk', not {constType!r}")
    if cx and constType in ("pam", "ook"):
        raise ValueError(f"constType = {constType!r} is real-valued: complex data needs 'qam' or 'psk'")
    if not cx and constType in ("qam", "psk"):
        raise ValueError(f"constType = {constType!r} is complex-valued: real data needs 'pam' or 'ook'")
    if constType == "ook":
        M = 2
    if isinstance(M, (bool, np.bool_)) or int(M) != M or M < 2 or int(M) & (int(M) - 1):
        raise ValueError("M must be a power of two, at least 2")
    if M > MAX_M:
        raise ValueError(f"M = {M}: the kernels stage a decision table of at most {MAX_M} points")
    M = int(M)
    if mode not in _lib.SISO_MODES:
        raise ValueError(f"trainingMode must be 'data-aided' or 'fulltime', not {mode!r}")
    names = {"ffe": ("nTaps", "nTapsFB"), "dfe": ("nTapsFF", "nTapsFB"), "volterra": ("n1Taps", "nTapsFB")}[kind]
    nTaps = _integer(names[0], nTaps, 1, MAX_TAPS)
    nFB = _integer(names[1], nFB, 0, MAX_FB)
    SpS = _integer("SpS", SpS, 1, MAX_SPS)
    if SpS > nTaps:
        raise ValueError(f"SpS = {SpS} exceeds {names[0]} = {nTaps}")
    preconv = _integer("preconvIters", preconv, 1, 2 ** 31 - 1)
    nTrain = _integer("nTrain", nTrain, 0)
    ncoef = nTaps + nFB
    if kind == "volterra":
        n2, n3 = _integer("n2Taps", n2, 1), _integer("n3Taps", n3, 1)
        if n2 > nTaps or n3 > nTaps:
            raise ValueError(f"n1Taps = {nTaps} must be at least n2Taps = {n2} and n3Taps = {n3}")
        if order not in (2, 3):
            raise ValueError(f"order = {order}: 2 or 3")
        ncoef = nTaps + n2 ** 2 + (n3 ** 3 if order == 3 else 0)
    if ncoef > MAX_COEFFS:
        raise ValueError(f"{ncoef} coefficients: one call adapts at most {MAX_COEFFS} (24 per lane of the wavefront)")
    mu = float(mu)
    if not np.isfinite(mu):
        raise ValueError("mu must be finite")
    n = int(x.shape[0])
    if n < 1:
        raise ValueError("sigIn is empty")
    N = n // SpS
    if N < 1:
        raise ValueError(f"sigIn has {n} samples: fewer than one symbol at SpS = {SpS}")
    if ref.shape[0] < min(nTrain, N):
        raise ValueError(f"symbRef has {ref.shape[0]} symbols: at least min(nTrain, N) = {min(nTrain, N)} are needed")

    work = np.complex128 if cx else np.float64
    if kind == "ffe":
        parts = [_coefficients(g("f", None), (nTaps,), work, "param.f", nTaps // 2)]
    elif kind == "dfe":
        parts = [_coefficients(g("f", None), (nTaps,), work, "param.f", nTaps // 2), _coefficients(g("b", None), (nFB,), work, "param.b")]
    else:
        h = g("h", None)
        if h is not None and len(h) != 3:
            raise ValueError("param.h must be [h1, h2, h3]")
        h = [None] * 3 if h is None else h
        parts = [_coefficients(h[0], (nTaps,), work, "param.h[0]", nTaps // 2), _coefficients(h[1], (n2, n2), work, "param.h[1]"),
                 _coefficients(h[2], (n3, n3, n3), work, "param.h[2]")]
    table = _table(M, constType, prec)
    p = _lib.SisoParams(n=n, nref=int(ref.shape[0]), nTrain=nTrain, kind=_lib.SISO_KINDS[kind], mode=_lib.SISO_MODES[mode],
                        dtype=_lib.METRICS_DTYPES[x.dtype.name], ref_dtype=_lib.METRICS_DTYPES[ref.dtype.name],
                        prec32=int(prec.name in ("float32", "complex64")), order=int(order), nTaps=nTaps, nFB=nFB, n2=n2, n3=n3, SpS=SpS, M=M,
                        preconvIters=preconv, ncoef=ncoef, no_frozen=int(not _FROZEN), mu=mu)
    return dict(x=x, ref=ref, params=p, parts=parts, table=np.ascontiguousarray(table.astype(np.complex128)).view(np.float64), N=N, cx=cx,
                kind=kind, order=int(order), ncoef=ncoef)


def expected_split(q, frozen=True):
    """(serial symbols over all passes, symbols of the frozen kernel) of a prepared call: siso_kernels.h: split_of."""
    p = q["params"]
    N, nTrain, nTaps, SpS = q["N"], p.nTrain, p.nTaps, p.SpS
    passes = p.preconvIters if nTrain < N else 1
    serial_last = N
    if frozen and p.mode == 0 and q["kind"] != "dfe":
        start = max(nTrain, (nTaps + SpS - 1) // SpS if passes > 1 else 0)
        if start < N:
            serial_last = start
    return (passes - 1) * (nTrain + 1) + serial_last, N - serial_last


def _run(kind, sigIn, symbRef, param):
    from .models import _state
    q = _prepare(kind, sigIn, symbRef, param)
    lib = _lib.load()
    x, ref, N, p = q["x"], q["ref"], q["N"], q["params"]
    on_dev = _dev.is_device(x)
    xp, keep_x = _dev.arg(x, x.dtype)
    rp, keep_r = (None, None) if ref.shape[0] == 0 else _dev.arg(ref, ref.dtype)
    used = q["parts"] if not (kind == "volterra" and q["order"] == 2) else q["parts"][:2]
    coef = np.concatenate([a.reshape(-1) for a in used])
    out = _dev.empty(on_dev, (N,), np.complex128 if q["cx"] else np.float64)
    mse = _dev.empty(on_dev, (N,), np.float64)
    rc = lib.ssf_siso_eq(_state["device"], C.byref(p), q["table"].ctypes.data_as(C.POINTER(C.c_double)), coef.ctypes.data_as(C.c_void_p),
                         xp, rp, _dev.out_ptr(out), _dev.out_ptr(mse))
    _lib.raise_for(lib, None, rc)
    del keep_x, keep_r
    last_call.clear()
    last_call.update(kind=kind, serial_symbols=int(p.serial_symbols), parallel_symbols=int(p.parallel_symbols), R=int(p.R), N=N)
    res, at = [], 0
    for a in q["parts"]:
        if at < coef.size:
            res.append(coef[at:at + a.size].reshape(a.shape).copy())
            at += a.size
        else:
            res.append(a)                     # order 2: h3 comes back as given
    return out, res, mse


def ffe(sigIn, symbRef, param):
    """Feed-forward equalizer (optic/dsp/equalization.py:1545-1865).  Parameters read from ``param`` with the reference's defaults:
    nTaps (5), mu (1e-4), SpS (1), nTrain (1000), prec (the input's dtype), M (4), constType ('pam'), f, trainingMode
    ('data-aided'), preconvIters (1).  Returns ``(sigOut, f, mse)``."""
    out, c, mse = _run("ffe", sigIn, symbRef, param)
    return out, c[0], mse


def dfe(sigIn, symbRef, param):
    """Decision-feedback equalizer (optic/dsp/equalization.py:1176-1542).  Parameters: nTapsFF (5), nTapsFB (5), SpS (1), mu (1e-4),
    nTrain (1000), prec (the input's dtype), M (4), constType ('pam'), f, b, trainingMode ('data-aided'), preconvIters (1).
    Returns ``(sigOut, f, b, mse)``."""
    out, c, mse = _run("dfe", sigIn, symbRef, param)
    return out, c[0], c[1], mse


def volterra(sigIn, symbRef, param):
    """Volterra equalizer up to the third order (optic/dsp/equalization.py:1868-2143).  Parameters: n1Taps (5), n2Taps (3), n3Taps
    (2), h, SpS (1), mu (1e-3), nTrain (1000), order (2), prec (float32), M (4), constType ('pam'), trainingMode ('data-aided'),
    preconvIters (1).  Returns ``(sigOut, [h1, h2, h3], mse)``; ``sigOut`` is power-normalised."""
    out, c, mse = _run("volterra", sigIn, symbRef, param)
    return out, c, mse
