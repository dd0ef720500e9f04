"""Sequence and symbol detection of the direct-detection chain on the device: mlse, detector, and the whitening filter behind them.

Drop-in for ``mlse`` and ``detector`` (optic/comm/modulation.py:582-680, 412-481) and for ``autocorr``, ``levinson`` and
``estimateWhiteningFilter`` (optic/dsp/core.py:1143-1254): the stage between ``ffe`` and ``fastBERcalc`` in ``... -> ffe -> mlse ->
fastBERcalc``.  A ``DeviceArray`` in gives a ``DeviceArray`` out and nothing the size of the signal crosses the bus.

``mlse`` is the Viterbi algorithm over a known impulse response ``h`` (opticommpy_amd/csrc/engine_seqdet.hip): one workgroup per
column runs the forward pass with one lane per trellis state and keeps one survivor byte per state and step; the traceback is
three launches that no longer depend on each other symbol by symbol.  All path metrics start at zero, the branch metric is
``|y[n] - yExpected| ** 2`` with the expected outputs summed in the reference's order, equal candidates go to the lowest
predecessor state, the final state is the lowest-index minimum.  ``last_call`` says what ran and holds the final minimum path
metric of every column.

Arguments are numpy arrays or ``DeviceArray``s; inputs are never written and a second call returns the same bits.

Scope and limits (anything else raises ``ValueError`` / ``TypeError`` before anything is launched or allocated; there is no CPU
fallback):

* ``mlse``: ``y`` 1-D or ``(N, nModes)`` with at most 64 columns, each an independent sequence over the same ``h``; 1 to 64
  constellation points, at most 11 taps, at most 1024 states ``M ** (taps - 1)``, survivor memory at most 2 ** 31 bytes.  A numpy
  ``y`` has any real or complex float dtype (the arithmetic is double, the result has ``y``'s dtype); a ``DeviceArray`` is float64 or
  complex128.  Real ``y`` needs real-valued ``h`` and ``constSymb`` (complex arrays with zero imaginary parts are narrowed);
* ``detector``: 1 to 64 points, ``r`` 1-D or ``(n, nModes)``, ``rule`` 'MAP' or 'ML', ``len(px) == M``, ``σ2 > 0`` under 'MAP';
* ``autocorr`` / ``estimateWhiteningFilter``: real ``x``, ``1 <= nTaps <= 256``, ``nTaps <= len(x)``.

Deviations from the reference, on purpose:

* the reference computes in ``y``'s precision; here single- and half-precision input is widened first;
* ``|.| ** 2`` of a complex value is ``re ** 2 + im ** 2`` (the reference squares ``np.abs``);
* ``detector`` raises where the reference prints a message and returns zeros.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["mlse", "detector", "autocorr", "levinson", "estimateWhiteningFilter", "last_call"]

MAX_M, MAX_STATES, MAX_TAPS, MAX_COLS = _lib.SEQDET_MAX_M, _lib.SEQDET_MAX_STATES, _lib.SEQDET_MAX_TAPS, _lib.SEQDET_MAX_COLS
T, CHUNK = _lib.SEQDET_SURV_CHUNK, _lib.SEQDET_STAGE_CHUNK       # survivor chunk, staging chunk of y
MAX_SURVIVOR_BYTES = _lib.SEQDET_MAX_SURVIVOR_BYTES
AC_MAX_TAPS = _lib.SEQDET_AC_MAX_TAPS

# what the last mlse call ran: states, kernel ('forward_wave64' | 'forward_multiwave'), chunk (steps per survivor chunk),
# survivor_bytes, final_metric (float64 per column: the smallest path metric after the last step), N, cols
last_call = {}

_TIMING = False            # measurement aid of tools/bench_seqdet.py: True adds fwd_ms / tb_ms (device events) to last_call


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _host_vector(a, name):
    a = np.asarray(a.get() if _dev.is_device(a) else a)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    if a.dtype.kind not in "fciub":
        raise TypeError(f"{name} has dtype {a.dtype.name}: numbers expected")
    return a


def _signal(x, name):
    """The array as the library takes it, its result dtype, and whether it is complex."""
    if _dev.is_device(x):
        if x.dtype.name not in ("float64", "complex128"):
            raise TypeError(f"device array has dtype {x.dtype.name}, this call needs float64 or complex128")
        out_dtype = x.dtype
    else:
        x = np.asarray(x)
        if x.dtype.kind not in "fc":
            raise TypeError(f"{name} has dtype {x.dtype.name}: a real or complex float dtype expected")
        out_dtype = x.dtype
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must be 1-D or (n, nModes)")
    return x, np.dtype(out_dtype), np.dtype(out_dtype).kind == "c"


def survivor_bytes(N, cols, states):
    """Survivor memory of a call: a row of max(4, states rounded up to 4) bytes per step, each column rounded up to 16."""
    return cols * ((N * ((states + 3) & ~3) + 15) // 16 * 16)


def _prepare_mlse(y, h, constSymb):
    """Every check and every host-side quantity of a call, without touching the library."""
    y, out_dtype, cx = _signal(y, "y")
    h, c = _host_vector(h, "h"), _host_vector(constSymb, "constSymb")
    M, taps = int(c.shape[0]), int(h.shape[0])
    if M < 1 or M > MAX_M:
        raise ValueError(f"constSymb has {M} points: mlse takes 1 to {MAX_M}")
    if taps < 1:
        raise ValueError("h is empty")
    if taps > MAX_TAPS:
        raise ValueError(f"h has {taps} taps: at most {MAX_TAPS}")
    states = M ** (taps - 1)
    if states > MAX_STATES:
        raise ValueError(f"{M} ** {taps - 1} = {states} states: the trellis holds at most {MAX_STATES}")
    cols = 1 if y.ndim == 1 else int(y.shape[1])
    if cols < 1 or cols > MAX_COLS:
        raise ValueError(f"y has {cols} columns: 1 to {MAX_COLS}")
    N = int(y.shape[0])
    if N < 1:
        raise ValueError("y is empty")
    sb = survivor_bytes(N, cols, states)
    if sb > MAX_SURVIVOR_BYTES:
        raise ValueError(f"survivor memory of {sb} bytes is above 2 ** 31 bytes")
    if not cx:
        for a, name in ((h, "h"), (c, "constSymb")):
            if np.iscomplexobj(a) and np.any(a.imag != 0):
                raise ValueError(f"y is real but {name} has imaginary parts")
    h2 = np.ascontiguousarray(h.astype(np.complex128)).view(np.float64)
    c2 = np.ascontiguousarray(c.astype(np.complex128)).view(np.float64)
    return dict(y=y, h=h2, c=c2, M=M, taps=taps, states=states, cols=cols, N=N, cx=cx, out_dtype=out_dtype, survivor_bytes=sb)


def mlse(y, h, constSymb):
    """Maximum-likelihood sequence estimation by the Viterbi algorithm (optic/comm/modulation.py:582-680): the sequence of points
    of ``constSymb`` whose convolution with ``h`` is nearest to ``y``.  Returns an array like ``y``."""
    from .models import _state
    q = _prepare_mlse(y, h, constSymb)
    lib = _lib.load()
    y, on_dev = q["y"], _dev.is_device(q["y"])
    work = np.complex128 if q["cx"] else np.float64
    yp, keep = _dev.arg(y, work)
    out = _dev.empty(on_dev, y.shape, work)
    p = _lib.MlseParams(n=q["N"], cols=q["cols"], dtype=_lib.METRICS_DTYPES[np.dtype(work).name], M=q["M"], taps=q["taps"], timing=int(_TIMING))
    fin = np.empty(q["cols"], dtype=np.float64)
    rc = lib.ssf_mlse(_state["device"], C.byref(p), _dp(q["h"]), _dp(q["c"]), yp, _dev.out_ptr(out), _dp(fin))
    _lib.raise_for(lib, None, rc)
    del keep
    last_call.clear()
    last_call.update(states=int(p.states), kernel=_lib.SEQDET_KERNELS[p.kernel], chunk=int(p.chunk), survivor_bytes=int(p.survivor_bytes),
                     final_metric=fin, N=q["N"], cols=q["cols"])
    if _TIMING:
        last_call.update(fwd_ms=float(p.fwd_ms), tb_ms=float(p.tb_ms))
    return out if on_dev else out.astype(q["out_dtype"], copy=False)


def _prepare_detector(r, σ2, constSymb, px, rule):
    if rule not in _lib.SEQDET_RULES:
        raise ValueError(f"rule must be 'MAP' or 'ML', not {rule!r}")
    r, out_dtype, cx = _signal(r, "r")
    c = _host_vector(constSymb, "constSymb")
    M = int(c.shape[0])
    if M < 1 or M > MAX_M:
        raise ValueError(f"constSymb has {M} points: detector takes 1 to {MAX_M}")
    if r.size < 1:
        raise ValueError("r is empty")
    logpx = np.zeros(M)
    if rule == "MAP":
        if not float(σ2) > 0:
            raise ValueError(f"σ2 = {σ2}: the noise variance must be positive under the MAP rule")
        if px is not None:
            px = np.asarray(px.get() if _dev.is_device(px) else px, dtype=np.float64).reshape(-1)
            if px.shape[0] != M:
                raise ValueError(f"px has {px.shape[0]} entries for {M} constellation points")
            with np.errstate(divide="ignore"):
                logpx = np.log(px)
        else:
            logpx = np.log(1 / M * np.ones(M))
    widen = not cx and np.iscomplexobj(c) and bool(np.any(c.imag != 0))      # real r against a complex table: distances are complex
    if widen and _dev.is_device(r):
        raise TypeError("a real device array against a complex constSymb: hand r over as complex128")
    c2 = np.ascontiguousarray(c.astype(np.complex128)).view(np.float64)
    return dict(r=r, c=c2, logpx=np.ascontiguousarray(logpx, dtype=np.float64), M=M, cx=cx or widen, widen=widen, out_dtype=out_dtype,
                rule=_lib.SEQDET_RULES[rule], sigma2=float(σ2) if rule == "MAP" else 1.0)


def detector(r, σ2, constSymb, px=None, rule="MAP"):
    """Symbol-by-symbol detection by the MAP or the ML rule (optic/comm/modulation.py:412-481).  Returns ``(decided, indDec)``:
    the decided points in ``r``'s dtype and their indices in ``constSymb`` as int64, both of ``r``'s shape and kind."""
    from .models import _state
    q = _prepare_detector(r, σ2, constSymb, px, rule)
    lib = _lib.load()
    r, on_dev = q["r"], _dev.is_device(q["r"])
    work = np.complex128 if q["cx"] else np.float64
    rp, keep = _dev.arg(r, work)
    decided, ind = _dev.empty(on_dev, r.shape, work), _dev.empty(on_dev, r.shape, np.int64)
    rc = lib.ssf_detector(_state["device"], r.size, _lib.METRICS_DTYPES[np.dtype(work).name], q["M"], q["rule"], q["sigma2"], _dp(q["c"]),
                          _dp(q["logpx"]), rp, _dev.out_ptr(decided), _dev.out_ptr(ind))
    _lib.raise_for(lib, None, rc)
    del keep
    if on_dev:
        return decided, ind
    if q["widen"]:
        decided = decided.real
    return decided.astype(q["out_dtype"], copy=False), ind


def _real_vector(x, nTaps):
    if _dev.is_device(x):
        if x.dtype.kind == "c":
            raise ValueError("autocorr takes real data")
        if x.dtype.name != "float64":
            raise TypeError(f"device array has dtype {x.dtype.name}, this call needs float64")
    else:
        x = np.asarray(x)
        if x.dtype.kind == "c":
            raise ValueError("autocorr takes real data")
        if x.dtype.kind not in "fiub":
            raise TypeError(f"x has dtype {x.dtype.name}: real numbers expected")
    if x.ndim != 1:
        raise ValueError("x must be one-dimensional")
    if isinstance(nTaps, (bool, np.bool_)) or int(nTaps) != nTaps or nTaps < 1 or nTaps > AC_MAX_TAPS:
        raise ValueError(f"nTaps = {nTaps}: it must be an integer between 1 and {AC_MAX_TAPS}")
    if nTaps > x.shape[0]:
        raise ValueError(f"nTaps = {nTaps} exceeds the {x.shape[0]} samples of x")
    return x, int(nTaps)


def autocorr(x, nTaps):
    """Unbiased autocorrelation estimate at the lags 0 .. nTaps - 1 (optic/dsp/core.py:1194-1227): one launch for all lags.
    Returns a numpy float64 array for either kind of argument: only ``nTaps`` values leave the GPU."""
    from .models import _state
    x, nTaps = _real_vector(x, nTaps)
    lib = _lib.load()
    xp, keep = _dev.arg(x, np.float64)
    r = np.empty(nTaps, dtype=np.float64)
    _lib.raise_for(lib, None, lib.ssf_autocorr(_state["device"], int(x.shape[0]), nTaps, xp, _dp(r)))
    del keep
    return r


def levinson(r, nTaps):
    """Levinson-Durbin recursion on the host (optic/dsp/core.py:1143-1190), with the reference's loop bounds as written: both inner
    loops run over ``range(1, i)``."""
    r = np.asarray(r.get() if _dev.is_device(r) else r)
    if isinstance(nTaps, (bool, np.bool_)) or int(nTaps) != nTaps or nTaps < 1 or nTaps > r.shape[0]:
        raise ValueError(f"nTaps = {nTaps}: it must be an integer between 1 and len(r) = {r.shape[0]}")
    a = np.zeros(int(nTaps), dtype=r.dtype)
    a[0] = 1.0
    e = r[0]
    for i in range(1, int(nTaps)):
        acc = 0
        for j in range(1, i):
            acc += a[j] * r[i - j]
        k = -(r[i] + acc) / e
        nxt = a.copy()
        for j in range(1, i):
            nxt[j] += k * np.conj(a[i - j])
        nxt[i] = k
        a = nxt
        e *= 1 - np.abs(k) ** 2
    return a


def estimateWhiteningFilter(x, nTaps):
    """Whitening filter of ``nTaps`` coefficients from the signal's autocorrelation (optic/dsp/core.py:1231-1254).  Returns a numpy
    float64 array for either kind of argument."""
    return levinson(autocorr(x, nTaps), nTaps)
