"""Sequence synchronisation on the device: the transmitted symbols aligned to the received signal.

Drop-in for ``symbolSync`` and ``finddelay`` (optic/dsp/core.py:552-675, 678-698), the stage between ``edc`` and
``mimoAdaptEqualizer`` in the reference's coherent chain.  One library call (``ssf_symbol_sync``, include/ssf.h) decimates the
received signal to one sample per symbol, correlates every transmitted with every received mode through batched transforms, finds
the peaks, decides mode permutation, quarter-turn rotation, conjugation and delay, and gathers the aligned symbols; a
``DeviceArray`` in gives a ``DeviceArray`` out, and only the record of the decisions (a few numbers per mode) crosses the bus.

``rx`` and ``tx`` are numpy arrays or ``DeviceArray``s, complex128 or complex64, of shape ``(n, nModes)`` or 1-D.  The result
has ``tx``'s shape and dtype: the arithmetic on ``tx`` is a permutation, a product with 1, -1, 1j or -1j, a conjugation and a
roll, so it equals the reference's bit for bit (up to the sign of zeros) wherever the decisions are the same.  Inputs are never
written.

Scope and limits (anything else raises ``ValueError`` before anything is launched or allocated; there is no CPU fallback):
``mode`` 'amp' or 'real'; at most 8 modes, the same number on both sides; at least 2 symbols on either side; a complex ``tx``;
``len(rx)`` a multiple of ``SpS``.
"""
import ctypes as C
import types

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["symbolSync", "finddelay"]

MAX_MODES = _lib.SYNC_MAX_MODES
_COMPLEX = ("complex128", "complex64")


def _sequence(x, name, need_complex):
    """(array, n, nModes): 1-D is one mode."""
    if _dev.is_device(x):
        if x.dtype.name not in _COMPLEX:
            if need_complex and x.dtype.kind != "c":
                raise ValueError(f"{name} must be complex: a real (PAM) sequence is not synchronised on the device")
            raise TypeError(f"device array has dtype {x.dtype.name}: complex128 or complex64 expected")
    else:
        x = np.asarray(x)
        if need_complex and x.dtype.kind != "c":
            raise ValueError(f"{name} must be complex: a real (PAM) sequence is not synchronised on the device")
        if x.dtype.name not in _COMPLEX:
            x = x.astype(np.complex128)
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must have one or two dimensions")
    n, modes = x.shape[0], (1 if x.ndim == 1 else x.shape[1])
    if modes < 1 or modes > MAX_MODES:
        raise ValueError(f"{name} has {modes} modes: between 1 and {MAX_MODES} are synchronised in one call")
    return x, int(n), int(modes)


def _check(rx, tx, SpS, mode):
    if mode not in _lib.SYNC_MODES:
        raise ValueError(f"mode must be 'amp' or 'real', not {mode!r}")
    if int(SpS) != SpS or SpS < 1:
        raise ValueError(f"SpS = {SpS}: the samples per symbol must be a positive integer")
    SpS = int(SpS)
    rx, n_rx, modes = _sequence(rx, "rx", False)
    tx, n_tx, modes_tx = _sequence(tx, "tx", True)
    if modes != modes_tx:
        raise ValueError(f"rx has {modes} modes and tx {modes_tx}")
    if n_rx % SpS:
        raise ValueError(f"cannot reshape array of size {n_rx} into shape (-1, {SpS}): len(rx) is not a multiple of SpS")
    if n_tx < 2 or n_rx // SpS < 2:
        raise ValueError(f"{n_tx} transmitted and {n_rx // SpS} received symbols: at least 2 are needed on either side")
    if SpS * modes > 256:
        raise ValueError(f"SpS * nModes = {SpS * modes}: at most 256 sampling classes are searched")
    params = _lib.SyncParams(n_rx=n_rx, n_tx=n_tx, nModes=modes, SpS=SpS, mode=_lib.SYNC_MODES[mode],
                             rx_dtype=_lib.METRICS_DTYPES[rx.dtype.name], tx_dtype=_lib.METRICS_DTYPES[tx.dtype.name])
    return rx, tx, params


def symbolSync(rx, tx, SpS, mode="amp", return_info=False):
    """Symbol synchronizer (optic/dsp/core.py:552-675): ``tx`` aligned to ``rx``, which holds ``SpS`` samples per symbol.

    ``mode`` 'amp' correlates the amplitudes, 'real' the real parts (it also undoes rotations by multiples of pi/2 and a
    conjugation).  With ``return_info`` the call returns ``(tx, info)``; ``info`` holds, per mode, ``delay``, ``swap``, ``rot``
    (1, -1, 1j or -1j, as applied) and ``conj``, and the ``(nModes, nModes)`` ``corrMatrix``."""
    from .models import _state
    rx, tx, p = _check(rx, tx, SpS, mode)
    lib = _lib.load()
    on_dev = _dev.is_device(rx) or _dev.is_device(tx)
    rx_ptr, keep_rx = _dev.arg(rx, rx.dtype)
    tx_ptr, keep_tx = _dev.arg(tx, tx.dtype)
    out = _dev.empty(on_dev, tx.shape, tx.dtype)
    res = _lib.SyncResult()
    rc = lib.ssf_symbol_sync(_state["device"], C.byref(p), rx_ptr, tx_ptr, _dev.out_ptr(out), C.byref(res))
    _lib.raise_for(lib, None, rc)
    del keep_rx, keep_tx
    if not return_info:
        return out
    m = p.nModes
    info = types.SimpleNamespace(delay=np.array(res.delay[:m], dtype=np.int64), swap=np.array(res.swap[:m], dtype=np.int64),
                                 rot=np.array([_lib.SYNC_ROT[r] for r in res.rot[:m]], dtype=np.complex64),
                                 conj=np.array(res.conj[:m], dtype=bool),
                                 corrMatrix=np.array(res.corrMatrix[:m * m], dtype=np.float64).reshape(m, m))
    return out, info


def _vector(x, name):
    if _dev.is_device(x):
        if x.dtype.name not in _lib.METRICS_DTYPES:
            raise TypeError(f"device array has dtype {x.dtype.name}: complex128, complex64, float64 or float32 expected")
    else:
        x = np.asarray(x)
        if x.dtype.name not in _lib.METRICS_DTYPES:
            x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    if x.ndim != 1 or x.shape[0] < 1:
        raise ValueError(f"{name} must be a 1-D array with at least one element")
    return x


def finddelay(x, y):
    """Delay between x and y in samples (optic/dsp/core.py:678-698): ``argmax |correlate(x, y)| - len(x) + 1`` with scipy's
    full correlation (``y`` conjugated), the first maximum.  Real or complex 1-D arrays, host or device; a Python int."""
    from .models import _state
    x, y = _vector(x, "x"), _vector(y, "y")
    lib = _lib.load()
    x_ptr, keep_x = _dev.arg(x, x.dtype)
    y_ptr, keep_y = _dev.arg(y, y.dtype)
    delay = C.c_int64(0)
    rc = lib.ssf_finddelay(_state["device"], x.shape[0], y.shape[0], _lib.METRICS_DTYPES[x.dtype.name], _lib.METRICS_DTYPES[y.dtype.name],
                           x_ptr, y_ptr, C.byref(delay))
    _lib.raise_for(lib, None, rc)
    del keep_x, keep_y
    return int(delay.value)
