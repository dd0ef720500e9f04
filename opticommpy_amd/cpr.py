"""Carrier phase recovery on the device: blind phase search with the 4th-power frequency offset estimation ahead of it.

Drop-in for ``cpr``, ``bps``, ``bpsGPU`` and ``fourthPowerFOE`` (optic/dsp/carrierRecovery.py:37-169, 172-223, 333-371;
optic/dsp/carrierRecoveryGPU.py:17-68), the stage between ``mimoAdaptEqualizer`` / ``decimate`` and the link metrics in the
reference's coherent chain.  One library call (``ssf_cpr``, include/ssf.h) runs frequency offset compensation, joint
normalisation, the search, ``np.unwrap(4 phi, axis=0) / 4`` and ``pnorm(x e^{j phi})`` on the GPU; a ``DeviceArray`` in gives a
``DeviceArray`` out without a host copy of the symbols (one small record per mode, the offset estimator's spectral peak, crosses
the bus).

Arguments are numpy arrays or ``DeviceArray``s, complex128 or complex64, of shape ``(n, nModes)`` or 1-D (1-D in, 1-D out).
Arithmetic is double whatever the input type; ``sigOut`` is complex128 and ``phaseEst`` float64.  Inputs are never written.

Scope and limits (anything else raises ``ValueError`` before anything is launched or allocated; there is no CPU fallback):

* ``alg`` 'bps' and 'bpsGPU' (the same device path).  'ddpll' and 'viterbi' are not implemented;
* ``constType`` 'qam' (square) or 'psk', ``M`` a power of two in [2, 1024];
* 1 <= ``B`` <= 1024 test phases; window parameter 0 <= ``N`` <= 2047 for ``cpr`` (half window ``N // 2`` <= 1023; ``bps`` takes
  the half window itself, <= 1023); ``n`` >= 2 symbols; at most 64 modes.

Deviations from the reference, on purpose:

* a complex64 signal is widened once and stays double: with ``runFOE`` the reference rounds the compensated signal back to
  single precision;
* the linewidth the reference only logs is not estimated; ``symbTx`` is accepted and ignored, as 'bps' ignores it there;
* 8-PSK and higher PSK are accepted although test phases pi/4 apart are equivalent for them, which leaves the reference's own
  result ill-conditioned.
"""
import ctypes as C
import sys
import types

import numpy as np

from . import _lib
from . import device as _dev
from .wdm_tx import grayMapping

__all__ = ["cpr", "bps", "bpsGPU", "fourthPowerFOE"]

MAX_M, MAX_B, MAX_HALF_WINDOW, MAX_MODES = 1024, 1024, 1023, 64
_DTYPES = ("complex128", "complex64")


def _table(M, constType, shapingFactor):
    """cpr's constellation with the reference's expressions and dtypes: grayMapping is complex64 and stays so through the
    normalisation (carrierRecovery.py:118-121)."""
    constSymb = grayMapping(M, constType)
    px = np.exp(-shapingFactor * np.abs(constSymb) ** 2)
    px = px / np.sum(px)
    constSymb /= np.sqrt(np.sum(np.abs(constSymb) ** 2 * px))
    return constSymb


def _check_constellation(M, constType):
    if constType not in ("qam", "psk"):
        raise ValueError(f"constType must be 'qam' or 'psk', not {constType!r}")
    if int(M) != M or M < 2 or M > MAX_M or int(M) & (int(M) - 1):
        raise ValueError(f"M must be a power of two between 2 and {MAX_M}")
    M = int(M)
    if constType == "qam" and int(round(np.sqrt(M))) ** 2 != M:
        raise ValueError(f"{M}-QAM is not square: 'qam' needs M = 4, 16, 64, 256 or 1024")
    return M


def _check_search(half, B):
    if int(B) != B or B < 1 or B > MAX_B:
        raise ValueError(f"B = {B}: the number of test phases must be between 1 and {MAX_B}")
    if int(half) != half or half < 0 or half > MAX_HALF_WINDOW:
        raise ValueError(f"half window {half}: it must be between 0 and {MAX_HALF_WINDOW} (N up to {2 * MAX_HALF_WINDOW + 1} for cpr)")
    return int(half), int(B)


def _signal(x, name="sigIn"):
    """(array, n, nModes): 1-D is one mode; no 'transposed' rule, as in the reference."""
    if _dev.is_device(x):
        if x.dtype.name not in _DTYPES:
            raise TypeError(f"device array has dtype {x.dtype.name}: complex128 or complex64 expected")
    else:
        x = np.asarray(x)
        if x.dtype.name not in _DTYPES:
            x = x.astype(np.complex128)
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must have one or two dimensions")
    n, modes = x.shape[0], (1 if x.ndim == 1 else x.shape[1])
    if n < 2:
        raise ValueError(f"{name} has {n} symbols: at least 2 are needed")
    if modes < 1:
        raise ValueError(f"{name} is empty")
    if modes > MAX_MODES:
        raise ValueError(f"{name} has {modes} modes: at most {MAX_MODES} are processed in one call")
    return x, int(n), int(modes)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _wide(table):
    return np.ascontiguousarray(np.asarray(table).astype(np.complex128)).view(np.float64)


def cpr(sigIn, param=None, symbTx=None):
    """Carrier phase recovery (optic/dsp/carrierRecovery.py:37-169) with blind phase search.

    Parameters read from ``param`` with the reference's defaults: alg ('bps'), M (4), constType ('qam'), shapingFactor (0),
    B (64), N (35), Ts (1/32e9), runFOE (True), returnPhases (False).  Returns ``sigOut``, or ``(sigOut, phaseEst)`` with
    ``param.returnPhases``."""
    from .models import _state
    alg = getattr(param, "alg", "bps")
    M = getattr(param, "M", 4)
    constType = getattr(param, "constType", "qam")
    shapingFactor = getattr(param, "shapingFactor", 0)
    B = getattr(param, "B", 64)
    N = getattr(param, "N", 35)
    Ts = getattr(param, "Ts", 1 / 32e9)
    runFOE = getattr(param, "runFOE", True)
    returnPhases = getattr(param, "returnPhases", False)

    if alg in ("ddpll", "viterbi"):
        raise ValueError(f"alg = {alg!r} is not implemented on the device ('ddpll' is a serial loop, 'viterbi' another estimator): "
                         "use 'bps' or 'bpsGPU'")
    if alg not in ("bps", "bpsGPU"):
        raise ValueError(f"alg must be 'bps' or 'bpsGPU', not {alg!r}")
    M = _check_constellation(M, constType)
    if int(N) != N or N < 0:
        raise ValueError(f"N = {N}: the window parameter must be a non-negative integer")
    half, B = _check_search(int(N) // 2, B)
    x, n, modes = _signal(sigIn)
    if runFOE and not (Ts > 0 and np.isfinite(Ts)):
        raise ValueError(f"Ts = {Ts}: the symbol period must be positive")
    table = _table(M, constType, shapingFactor)

    p = _lib.CprParams(n=n, nModes=modes, M=M, dtype=_lib.METRICS_DTYPES[x.dtype.name], B=B, Nh=half, runFOE=int(bool(runFOE)),
                       P=M if constType == "psk" else 4, Fs=1 / Ts)
    lib = _lib.load()
    on_dev = _dev.is_device(x)
    ptr, keep = _dev.arg(x, x.dtype)
    out = _dev.empty(on_dev, x.shape, np.complex128)
    phase = _dev.empty(on_dev, x.shape, np.float64) if returnPhases else None
    fo = np.zeros(modes)
    rc = lib.ssf_cpr(_state["device"], C.byref(p), _dp(_wide(table)), ptr, _dev.out_ptr(out),
                     None if phase is None else _dev.out_ptr(phase), _dp(fo))
    _lib.raise_for(lib, None, rc)
    del keep
    return (out, phase) if returnPhases else out


def bps(sigIn, N, constSymb, B):
    """Blind phase search (carrierRecovery.py:172-223): the raw test phase of every symbol, ``(n, nModes)`` float64 (1-D for a
    1-D input).  ``N`` is half of the 2 N + 1 symbol window, ``constSymb`` the constellation the distances are taken to."""
    from .models import _state
    table = np.asarray(constSymb).reshape(-1)
    if table.size < 2 or table.size > MAX_M:
        raise ValueError(f"constSymb holds {table.size} points: between 2 and {MAX_M} are searched")
    half, B = _check_search(N, B)
    x, n, modes = _signal(sigIn)
    lib = _lib.load()
    on_dev = _dev.is_device(x)
    ptr, keep = _dev.arg(x, x.dtype)
    phase = _dev.empty(on_dev, x.shape, np.float64)
    rc = lib.ssf_bps(_state["device"], n, modes, _lib.METRICS_DTYPES[x.dtype.name], half, B, table.size, _dp(_wide(table)), ptr,
                     _dev.out_ptr(phase))
    _lib.raise_for(lib, None, rc)
    del keep
    return phase


bpsGPU = bps


def fourthPowerFOE(sigIn, Fs, M=4):
    """Frequency offset estimation and compensation with the M-th power method (carrierRecovery.py:333-371).  Returns
    ``(sigOut, fo)``; ``fo`` is a numpy array of length nModes."""
    from .models import _state
    if int(M) != M or M < 1 or M > MAX_M:
        raise ValueError(f"M = {M}: the power must be an integer between 1 and {MAX_M}")
    if not (Fs > 0 and np.isfinite(Fs)):
        raise ValueError(f"Fs = {Fs}: the sampling frequency must be positive")
    x, n, modes = _signal(sigIn)
    lib = _lib.load()
    ptr, keep = _dev.arg(x, x.dtype)
    out = _dev.empty(_dev.is_device(x), x.shape, np.complex128)
    fo = np.zeros(modes)
    rc = lib.ssf_foe(_state["device"], n, modes, _lib.METRICS_DTYPES[x.dtype.name], int(M), float(Fs), ptr, _dev.out_ptr(out), _dp(fo))
    _lib.raise_for(lib, None, rc)
    del keep
    return out, fo


class _CallableModule(types.ModuleType):
    """``opticommpy_amd.cpr`` names this module and the function ``cpr`` alike: calling the module calls the function, so
    ``oa.cpr(sigIn, param)`` and ``from opticommpy_amd.cpr import bps`` both work."""

    def __call__(self, *args, **kwargs):
        return cpr(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
