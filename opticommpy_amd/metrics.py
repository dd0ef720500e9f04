"""Link metrics on the device: BER, SER, SNR, GMI, NGMI, MI and EVM of received against transmitted symbols.

Drop-in for ``fastBERcalc``, ``monteCarloGMI``, ``monteCarloMI``, ``calcEVM`` (optic/comm/metrics.py:111-195, 329-493, 572-637),
``demodulateGray`` (optic/comm/modulation.py:369-408), ``pnorm``, ``anorm`` and ``signalPower`` (optic/dsp/core.py:69-85, 701-736), plus
``metrics``, which returns all seven numbers of one library call (``ssf_metrics``, include/ssf.h): the symbols are normalised once
and read once per pass, and only ``nModes`` result records come back from the GPU.  The four reference-named functions are that
same call with a selection of what is wanted, so their values equal those of ``metrics`` bit for bit.

Arguments are numpy arrays or ``DeviceArray``s, complex128 / complex64 (float64 / float32 for real data); arithmetic is double
whatever the input type.  Results are numpy arrays of length ``nModes``.

Deviations from the reference, on purpose:

* inputs are never modified (the reference's ``monteCarloGMI`` / ``monteCarloMI`` rotate and normalise the caller's arrays in place);
* ``discard=k`` evaluates symbols ``[k : n - k]`` -- what the notebooks do with ``ind = np.arange(discard, n - discard)`` on numpy
  arrays; a DeviceArray has no slicing;
* constellations are those of ``grayMapping``: 'qam' (square), 'psk', 'pam' with M a power of two up to 1024; anything else raises
  ``ValueError`` before anything is launched.

There is no CPU fallback: without the library or without a GPU every call raises.
"""
import ctypes as C
import functools
import sys
import types

import numpy as np

from . import _lib
from . import device as _dev
from .synchronization import Qfunc, bert, theoryBER  # noqa: F401  (optic/comm/metrics.py names them; they live with syncDataSequences)
from .theory import (  # noqa: F401  (optic/comm/metrics.py names them; they live in theory.py)
    ASE_NyquistWDM, GN_Model_NyquistWDM, GNmodel_OSNR, calcLinOSNR, calcMI, condEntropy, constellationMI, theoryMI,
)
from .wdm_tx import grayMapping

__all__ = ["fastBERcalc", "monteCarloGMI", "monteCarloMI", "calcEVM", "demodulateGray", "pnorm", "anorm", "signalPower", "metrics",
           "bert", "theoryBER", "Qfunc", "theoryMI", "constellationMI", "calcMI", "condEntropy", "GN_Model_NyquistWDM", "ASE_NyquistWDM",
           "GNmodel_OSNR", "calcLinOSNR"]

_NAMES = ("BER", "SER", "SNR", "GMI", "NGMI", "MI", "EVM")


class LinkMetrics(dict):
    """Result of ``metrics``: a dict whose entries (arrays of length nModes) are also attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def _check_constellation(M, constType):
    if constType not in ("qam", "psk", "pam"):
        raise ValueError(f"constType must be 'qam', 'psk' or 'pam', not {constType!r}")
    if int(M) != M or M < 2 or M > 1024 or int(M) & (int(M) - 1):
        raise ValueError("M must be a power of two between 2 and 1024")
    return int(M)


def _tables(M, constType, px=None):
    """The reference's derived tables, built with its expressions and explicit dtypes: (raw table widened to double, table
    normalised to unit energy in double, px, Es, H)."""
    if px is None or len(px) == 0:
        return _uniform_tables(M, constType)
    return _build_tables(M, constType, px)


@functools.lru_cache(maxsize=32)
def _uniform_tables(M, constType):
    return _build_tables(M, constType, None)                                # (read-only: handed to the library as they are)


def _build_tables(M, constType, px):
    M = _check_constellation(M, constType)
    const = grayMapping(M, constType)                                       # complex64 / float32 (ValueError for a non-square QAM)
    if px is None or len(px) == 0:
        px = 1 / M * np.ones(M)
    px = np.asarray(px, dtype=np.float64).reshape(-1)
    if px.shape != (M,):
        raise ValueError(f"px must hold M = {M} probabilities")
    Es = np.sum(np.abs(const) ** 2 * px)                                    # float32 squares, float64 sum
    H = np.sum(-px * np.log2(px))
    wide = np.complex128 if np.iscomplexobj(const) else np.float64
    norm = const.astype(wide) / np.sqrt(Es)
    return const.astype(np.complex128), norm.astype(np.complex128), px, float(Es), float(H)


@functools.lru_cache(maxsize=32)
def _evm_tables(M, constType):
    """calcEVM's table is pnorm(grayMapping(...)), which stays in single precision; |c|^2 in float32 for its float32 mean."""
    M = _check_constellation(M, constType)
    const = grayMapping(M, constType)
    const = const / np.sqrt(np.mean(const * np.conj(const)).real)
    assert const.dtype in (np.complex64, np.float32)
    return const.astype(np.complex128), (np.abs(const) ** 2).astype(np.float32)


def _columns(x, name):
    """(array, n, nModes, transposed) under the reference's shape rules: 1-D is one mode, shape[1] > shape[0] is transposed."""
    if not _dev.is_device(x):
        x = np.asarray(x)
        if x.dtype.name not in _lib.METRICS_DTYPES:
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if x.ndim == 1:
        n, modes, transposed = x.shape[0], 1, 0
    elif x.ndim == 2:
        transposed = int(x.shape[1] > x.shape[0])
        n, modes = (x.shape[1], x.shape[0]) if transposed else x.shape
    else:
        raise ValueError(f"{name} must have one or two dimensions")
    if n < 1 or modes < 1:
        raise ValueError(f"{name} is empty")
    if modes > 64:
        raise ValueError(f"{name} has {modes} modes: at most 64 are evaluated in one call")
    return x, int(n), int(modes), transposed


def _pointer(x):
    if _dev.is_device(x):
        if x.dtype.name not in _lib.METRICS_DTYPES:
            raise TypeError(f"device array has dtype {x.dtype.name}: complex128, complex64, float64 or float32 expected")
        return _dev.arg(x, x.dtype)
    return _dev.arg(x, x.dtype)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _run(want, rx, tx, M, constType, px, discard):
    from .models import _state
    blind = want == _lib.METRICS_EVM_BLIND
    if blind:
        norm, w32 = _evm_tables(M, constType)
        raw, pxa, Es, H = None, None, 1.0, 1.0
    else:
        raw, norm, pxa, Es, H = _tables(M, constType, px)
        w32 = None
    rx, n, modes, transposed = _columns(rx, "rx")
    if not blind:
        tx, nt, mt, tt = _columns(tx, "tx")
        if (nt, mt, tt) != (n, modes, transposed) or tx.ndim != rx.ndim:
            raise ValueError(f"rx and tx differ in shape: {rx.shape} and {tx.shape}")
        if rx.dtype != tx.dtype:
            if _dev.is_device(rx) or _dev.is_device(tx):
                raise TypeError(f"rx is {rx.dtype.name}, tx is {tx.dtype.name}: device arrays are not converted")
            both = np.complex128 if (np.iscomplexobj(rx) or np.iscomplexobj(tx)) else np.float64
            rx, tx = rx.astype(both), tx.astype(both)
    discard = int(discard)
    if discard < 0 or 2 * discard >= n:
        raise ValueError(f"discard = {discard} leaves none of the {n} symbols")
    p = _lib.MetricsParams(n=n, discard=discard, nModes=modes, M=int(M), dtype=_lib.METRICS_DTYPES[rx.dtype.name],
                           transposed=transposed, rotate=int(constType in ("qam", "psk")), want=want, Es=Es, H=H)
    lib = _lib.load()
    prx, keep_rx = _pointer(rx)
    ptx, keep_tx = (None, None) if blind else _pointer(tx)
    norm_f = np.ascontiguousarray(norm).view(np.float64)
    raw_f = None if raw is None else np.ascontiguousarray(raw).view(np.float64)
    out = (_lib.MetricsResult * modes)()
    rc = lib.ssf_metrics(_state["device"], C.byref(p), prx, ptx, None if raw_f is None else _dp(raw_f), _dp(norm_f),
                         None if pxa is None else _dp(pxa), None if w32 is None else w32.ctypes.data_as(C.POINTER(C.c_float)), out)
    _lib.raise_for(lib, None, rc)
    del keep_rx, keep_tx
    return {name: np.array([getattr(o, name) for o in out]) for name in _NAMES}


def metrics(rx, tx, M, constType, px=None, discard=0):
    """BER, SER, SNR [dB], GMI, NGMI, MI and (data-aided) EVM per mode from one pass sequence over the symbols.

    Returns a ``LinkMetrics`` (a dict with attribute access); every entry equals what the function of that name returns."""
    w = _lib.METRICS_BER | _lib.METRICS_GMI | _lib.METRICS_MI | _lib.METRICS_EVM
    return LinkMetrics(_run(w, rx, tx, M, constType, px, discard))


def fastBERcalc(rx, tx, M, constType, px=None, discard=0):
    """Monte Carlo BER, SER and SNR [dB] per mode (optic/comm/metrics.py:111-195).  Returns (BER, SER, SNR)."""
    r = _run(_lib.METRICS_BER, rx, tx, M, constType, px, discard)
    return r["BER"], r["SER"], r["SNR"]


def monteCarloGMI(rx, tx, M, constType, px=None, discard=0):
    """Monte Carlo generalised mutual information (optic/comm/metrics.py:329-426), with the reference's direct-form LLRs and
    their clip to +-500.  Returns (GMI, NGMI).  Unlike the reference, rx and tx are left as they are."""
    r = _run(_lib.METRICS_GMI, rx, tx, M, constType, px, discard)
    return r["GMI"], r["NGMI"]


def monteCarloMI(rx, tx, M, constType, px=None, discard=0):
    """Monte Carlo mutual information (optic/comm/metrics.py:429-547).  Unlike the reference, rx and tx are left as they are."""
    return _run(_lib.METRICS_MI, rx, tx, M, constType, px, discard)["MI"]


def calcEVM(symb, M, constType, symbTx=None, discard=0):
    """Error vector magnitude per mode (optic/comm/metrics.py:572-637): data-aided with ``symbTx``, otherwise against the
    nearest point of the unit-power constellation.  As in the reference both arrays are normalised jointly over all modes."""
    if symbTx is None or len(symbTx) == 0:
        return _run(_lib.METRICS_EVM_BLIND, symb, None, M, constType, None, discard)["EVM"]
    return _run(_lib.METRICS_EVM, symb, symbTx, M, constType, None, discard)["EVM"]


def demodulateGray(symb, M, constType):
    """Hard decisions to bits, log2(M) per symbol (optic/comm/modulation.py:369-408).  numpy in: numpy int64 out; a DeviceArray
    in: an int32 DeviceArray out."""
    from .models import _state
    raw = _tables(M, constType)[0]
    on_dev = _dev.is_device(symb)
    if not on_dev:
        symb = np.asarray(symb)
        if symb.dtype.name not in _lib.METRICS_DTYPES:
            symb = symb.astype(np.complex128 if np.iscomplexobj(symb) else np.float64)
    if symb.ndim != 1 or symb.shape[0] < 1:
        raise ValueError("symb must be a non-empty one-dimensional sequence of symbols")
    bits = int(M).bit_length() - 1
    lib = _lib.load()
    ptr, keep = _pointer(symb)
    out = _dev.empty(on_dev, (symb.shape[0] * bits,), np.int32)
    rc = lib.ssf_demodulate(_state["device"], symb.shape[0], _lib.METRICS_DTYPES[symb.dtype.name], int(M),
                            _dp(np.ascontiguousarray(raw).view(np.float64)), ptr, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out if on_dev else out.astype(np.int64)


def _flat(x):
    if not _dev.is_device(x):
        x = np.asarray(x)
        if x.dtype.name not in _lib.METRICS_DTYPES:
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if x.size < 1:
        raise ValueError("empty array")
    return x


def pnorm(x):
    """x / sqrt(mean |x|^2) over the whole array (optic/dsp/core.py:701-717), in double precision.  A DeviceArray gives a
    DeviceArray."""
    from .models import _state
    x = _flat(x)
    lib = _lib.load()
    ptr, keep = _pointer(x)
    out = _dev.empty(_dev.is_device(x), x.shape, np.complex128 if x.dtype.kind == "c" else np.float64)
    _lib.raise_for(lib, None, lib.ssf_pnorm(_state["device"], x.size, _lib.METRICS_DTYPES[x.dtype.name], ptr, _dev.out_ptr(out)))
    del keep
    return out


def anorm(x):
    """x / max |x| over the whole array (optic/dsp/core.py:720-736), in double precision; the maximum is taken in a fixed order.
    A DeviceArray gives a DeviceArray."""
    from .models import _state
    x = _flat(x)
    lib = _lib.load()
    ptr, keep = _pointer(x)
    out = _dev.empty(_dev.is_device(x), x.shape, np.complex128 if x.dtype.kind == "c" else np.float64)
    p = _lib.SisoParams(n=x.size, kind=_lib.SISO_KINDS["anorm"], dtype=_lib.METRICS_DTYPES[x.dtype.name])
    _lib.raise_for(lib, None, lib.ssf_siso_eq(_state["device"], C.byref(p), None, None, ptr, None, _dev.out_ptr(out), None))
    del keep
    return out


def signalPower(x):
    """Sum over the columns of their mean power (optic/dsp/core.py:69-85)."""
    from .models import _state
    x = _flat(x)
    lib = _lib.load()
    ptr, keep = _pointer(x)
    p = C.c_double()
    rows = x.shape[0] if x.ndim else 1
    _lib.raise_for(lib, None, lib.ssf_signal_power(_state["device"], x.size, rows, _lib.METRICS_DTYPES[x.dtype.name], ptr, C.byref(p)))
    del keep
    return p.value


class _CallableModule(types.ModuleType):
    """``opticommpy_amd.metrics`` names this module and the function ``metrics`` alike: calling the module calls the function, so
    ``oa.metrics(rx, tx, M, constType)`` and ``from opticommpy_amd.metrics import fastBERcalc`` both work."""

    def __call__(self, *args, **kwargs):
        return metrics(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
