"""Data-sequence synchronisation on the device: syncDataSequences, with movingAverage, bert, theoryBER and Qfunc.

Drop-in for ``syncDataSequences`` (optic/dsp/synchronization.py:30-170), ``movingAverage`` (optic/dsp/core.py:829-880) and ``bert``,
``theoryBER``, ``Qfunc`` (optic/comm/metrics.py:37-105, 550-569, 640-686).  ``syncDataSequences`` is the step that produces the
training and reference symbols of ``ffe`` / ``dfe`` / ``volterra`` / ``mlse`` and of ``fastBERcalc`` when the received signal is a
delayed, repeated copy of the transmitted one.

``syncDataSequences`` is composed in Python over ``DeviceArray``s: the tiled (and, for reference = 'symbols', zero-stuffed)
transmitted sequence and the zero-padded received one are written by one kernel (``ssf_sync_tile``) and are never built on the host;
``symbolSync`` aligns them; for 'symbols' the non-zero samples of every column are gathered in their order and divided by their root
mean square (``ssf_sync_extract``: flags, an exclusive scan per workgroup plus workgroup offsets, scatter) and the waveform comes from
``firFilter`` and ``pnorm``; for 'signal' the symbols come from ``resample``, ``decimate``, ``pnorm`` and ``detector``.  A
``DeviceArray`` in gives ``DeviceArray``s out and nothing of the signal's length crosses the bus -- only ``symbolSync``'s record of
decisions and scalars; numpy arguments are uploaded once each and the two results downloaded once each.  Inputs are never written and
a second call returns the same bits.

Kept from the reference: a transmitted symbol that is exactly 0 is dropped from ``symb`` under reference = 'symbols' (the samples
after it move up); ``symb`` has ``len(rx) // SpS + 1`` rows there, the last ones zero; ``movingAverage`` does not take N = 1.

Deviations, on purpose: results are double precision whatever the input (float64 for real ``rx`` and ``tx``, complex128 otherwise);
a real ``tx`` is widened on the device, synchronised and its real part returned, which is exact for real ``rx`` -- with a complex
``rx`` in syncMode 'real' the reference would cast a rotation by +-1j into a real array, so that case raises ``ValueError``;
``bert`` raises ``ValueError`` for an empty class where the reference returns NaN; ``movingAverage`` takes N up to 2048.

Scope and limits (anything else raises ``ValueError`` / ``TypeError`` before the library is loaded; there is no CPU fallback):
``reference`` 'signal' or 'symbols'; ``syncMode`` 'amp' or 'real'; ``SpS`` an integer >= 1; at most 8 modes, the same number on
both sides (``decimate`` searches at most 256 sampling classes, six modes at 41 samples per symbol: under 'signal' seven or eight
modes are decimated in two groups of columns, which changes nothing, every column having its own sampling phase); at least 2 rows on
either side; arrays complex128, complex64 or float64, 1-D or ``(n, nModes)``; ``pulseType`` 'rect',
'nrz', 'rrc' or 'rc' and ``nFilterTaps`` an integer >= 1 under 'symbols'.  ``bert``'s bits are 0 or 1: a bit counts as 1 where it
equals 1, on the host and on the device alike.
"""
import ctypes as C
import math
import types

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["syncDataSequences", "movingAverage", "bert", "theoryBER", "Qfunc"]

MAX_MODES = _lib.SYNC_MAX_MODES
DECIMATE_MODES = 256 // 41                     # decimate searches at most 256 sampling classes, 41 per mode under reference = 'signal'
MAX_N = _lib.SYNCDATA_MA_MAX_N
_DTYPES = ("complex128", "complex64", "float64")
_BIT_DTYPES = ("int8", "uint8", "int32", "int64", "bool")

# what the last syncDataSequences call decided: symbolSync's info (delay, swap, rot, conj, corrMatrix), repeats, padL and, under
# reference = 'symbols', the kept samples per column
last_call = {}


def _array(x, name):
    """A numpy array or DeviceArray of a dtype the kernels load, its rows and columns."""
    if _dev.is_device(x):
        if x.dtype.name not in _DTYPES:
            raise TypeError(f"device array {name} has dtype {x.dtype.name}: complex128, complex64 or float64 expected")
    else:
        x = np.asarray(x)
        if x.dtype.kind not in "fciub":
            raise TypeError(f"{name} has dtype {x.dtype.name}: numbers expected")
        if x.dtype.name not in _DTYPES:
            x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must have one or two dimensions")
    return x, int(x.shape[0]), (1 if x.ndim == 1 else int(x.shape[1]))


def _head(d, rows):
    """The first ``rows`` rows of a 2-D DeviceArray: the same memory (a view that keeps its owner alive)."""
    v = d.reshape(d.shape)
    v.shape = (int(rows), d.shape[1])
    return v


def _real_part(lib, device, d):
    out = _dev.DeviceArray(d.shape, np.float64)
    _lib.raise_for(lib, None, lib.ssf_real_part(device, d.size, d.ptr, out.ptr))
    return out


def _tile(rx, tx, n_pad, stuff):
    """(rx zero-padded, tx zero-stuffed and tiled): two (n_pad, nModes) complex128 DeviceArrays written by one launch."""
    from .models import _state
    lib = _lib.load()
    modes = 1 if rx.ndim == 1 else rx.shape[1]
    rx_ptr, keep_rx = _dev.arg(rx, rx.dtype)
    tx_ptr, keep_tx = _dev.arg(tx, tx.dtype)
    p = _lib.SyncTileParams(n_rx=rx.shape[0], n_tx=tx.shape[0], n_pad=n_pad, nModes=modes, SpS=stuff,
                            rx_dtype=_lib.METRICS_DTYPES[rx.dtype.name], tx_dtype=_lib.METRICS_DTYPES[tx.dtype.name])
    rx_pad, tx_rep = _dev.DeviceArray((n_pad, modes), np.complex128), _dev.DeviceArray((n_pad, modes), np.complex128)
    _lib.raise_for(lib, None, lib.ssf_sync_tile(_state["device"], C.byref(p), rx_ptr, tx_ptr, rx_pad.ptr, tx_rep.ptr))
    del keep_rx, keep_tx
    return rx_pad, tx_rep


def _extract(x, n_out, real_out, normalize=True):
    """(symb, kept): per column of the (n, nModes) complex128 DeviceArray the non-zero samples in their order from row 0 of ``n_out``
    rows, divided by their root mean square unless ``normalize`` is off; ``kept`` their number per column (numpy int64)."""
    from .models import _state
    lib = _lib.load()
    n, modes = x.shape
    symb = _dev.DeviceArray((n_out, modes), np.float64 if real_out else np.complex128)
    kept = (C.c_int64 * modes)()
    xp, keep = _dev.arg(x, np.complex128)
    rc = lib.ssf_sync_extract(_state["device"], n, modes, n_out, _lib.METRICS_DTYPES[symb.dtype.name], int(bool(normalize)), xp, symb.ptr, kept)
    _lib.raise_for(lib, None, rc)
    del keep
    return symb, np.array(kept[:], dtype=np.int64)


def _copy_columns(lib, device, src, first, width, dst, at):
    """dst[:, at : at + width] = src[:, first : first + width] on the device (complex128, the same number of rows)."""
    rc = lib.ssf_copy_columns(device, src.shape[0], width, src.shape[1], first, dst.shape[1], at, src.ptr, dst.ptr)
    _lib.raise_for(lib, None, rc)


def _decimate41(lib, device, x):
    """decimate from 41 samples per symbol to 1.  It takes DECIMATE_MODES columns at a time and every column has its own sampling
    phase, so more columns go through in groups and the results are put side by side."""
    from .rx import decimate
    p = types.SimpleNamespace(SpSin=41, SpSout=1)
    n, modes = x.shape
    if modes <= DECIMATE_MODES:
        return decimate(x, p)
    out = _dev.DeviceArray((n // 41, modes), np.complex128)
    for first in range(0, modes, (modes + 1) // 2):
        width = min((modes + 1) // 2, modes - first)
        part = _dev.DeviceArray((n, width), np.complex128)
        _copy_columns(lib, device, x, first, width, part, 0)
        _copy_columns(lib, device, decimate(part, p), 0, width, out, first)
    return out


def _prepare_sync(rx, tx, param):
    """Every check of a syncDataSequences call, without touching the library."""
    q = types.SimpleNamespace()
    q.SpS = getattr(param, "SpS", 1)
    q.reference = getattr(param, "reference", "signal")
    q.syncMode = getattr(param, "syncMode", "amp")
    q.pulseType = getattr(param, "pulseType", "rrc")
    q.rollOff = getattr(param, "rollOff", 0.01)
    q.nFilterTaps = getattr(param, "nFilterTaps", 1024)
    q.constType = getattr(param, "constType", "pam")
    q.M = getattr(param, "M", 4)
    if q.reference not in ("signal", "symbols"):
        raise ValueError(f"reference must be 'signal' or 'symbols', not {q.reference!r}")
    if q.syncMode not in _lib.SYNC_MODES:
        raise ValueError(f"syncMode must be 'amp' or 'real', not {q.syncMode!r}")
    if isinstance(q.SpS, (bool, np.bool_)) or int(q.SpS) != q.SpS or q.SpS < 1:
        raise ValueError(f"SpS = {q.SpS}: the samples per symbol must be a positive integer")
    q.SpS = int(q.SpS)
    q.rx, q.n_rx, modes = _array(rx, "rx")
    q.tx, q.n_tx, modes_tx = _array(tx, "tx")
    if modes != modes_tx:
        raise ValueError(f"rx has {modes} modes and tx {modes_tx}")
    if modes < 1 or modes > MAX_MODES:
        raise ValueError(f"{modes} modes: between 1 and {MAX_MODES} are synchronised in one call")
    if q.n_rx < 2 or q.n_tx < 2:
        raise ValueError(f"{q.n_tx} transmitted and {q.n_rx} received rows: at least 2 are needed on either side")
    q.modes = modes
    q.real_tx, q.real_rx = q.tx.dtype.kind != "c", q.rx.dtype.kind != "c"
    if q.real_tx and not q.real_rx and q.syncMode == "real":
        raise ValueError("a real tx against a complex rx in syncMode 'real': the rotation found may be +-1j, which a real sequence cannot "
                         "take; hand tx over as complex")
    q.real_out = q.real_tx and q.real_rx
    q.input1D = q.rx.ndim == 1
    q.stuff = q.SpS if q.reference == "symbols" else 1
    q.period = q.n_tx * q.stuff
    q.repeats = -(-q.n_rx // q.period)
    q.n_pad = q.repeats * q.period
    if q.n_pad > 1 << 31:
        raise ValueError(f"the tiled sequence has {q.n_pad} rows: at most 2 ** 31")
    if q.reference == "signal":
        from .metrics import _check_constellation
        _check_constellation(q.M, q.constType)
        if (q.n_rx * 41) // q.SpS < 41:
            raise ValueError("rx holds less than one symbol")
    else:
        from .wdm_tx import pulseShape
        if isinstance(q.nFilterTaps, (bool, np.bool_)) or int(q.nFilterTaps) != q.nFilterTaps or q.nFilterTaps < 1:
            raise ValueError(f"nFilterTaps = {q.nFilterTaps}: the pulse-shaping filter needs a positive integer number of taps")
        q.pulse = pulseShape(types.SimpleNamespace(pulseType=q.pulseType, SpS=q.SpS, rollOff=q.rollOff, nFilterTaps=int(q.nFilterTaps)))
        if not np.all(np.isfinite(q.pulse)):
            raise ValueError(f"pulseType = {q.pulseType!r} with rollOff = {q.rollOff} and SpS = {q.SpS} gives taps that are not finite")
    return q


def syncDataSequences(rx, tx, param):
    """Synchronize data sequences with a given reference sequence (optic/dsp/synchronization.py:30-170).  Parameters read from
    ``param`` with the reference's defaults: SpS (1), reference ('signal'), syncMode ('amp'), pulseType ('rrc'), rollOff (0.01),
    nFilterTaps (1024), constType ('pam'), M (4).  Returns ``(tx_, symb)``: the transmitted waveform aligned to ``rx`` (1-D for a
    1-D ``rx``) and the transmitted symbols, ``(n, nModes)``."""
    from .models import _state
    from .sync import symbolSync
    q = _prepare_sync(rx, tx, param)
    lib = _lib.load()
    device = _state["device"]
    on_dev = _dev.is_device(q.rx) or _dev.is_device(q.tx)
    rxd = q.rx if _dev.is_device(q.rx) else _dev.to_device(q.rx)
    txd = q.tx if _dev.is_device(q.tx) else _dev.to_device(q.tx)
    rx_pad, tx_rep = _tile(rxd, txd, q.n_pad, q.stuff)

    aligned, info = symbolSync(rx_pad, tx_rep, 1, q.syncMode, return_info=True)
    aligned = _head(aligned, q.n_rx)
    last_call.clear()
    last_call.update(info=info, repeats=q.repeats, padL=q.n_pad - q.n_rx, reference=q.reference)

    if q.reference == "symbols":
        from .metrics import pnorm
        from .rx import firFilter
        symb, last_call["kept"] = _extract(aligned, q.n_rx // q.SpS + 1, q.real_out)
        tx_ = pnorm(firFilter(q.pulse, aligned))
        if q.real_out:
            tx_ = _real_part(lib, device, tx_)
    else:
        from .clock import resample
        from .metrics import pnorm
        from .seqdet import detector
        from .wdm_tx import grayMapping
        x = resample(aligned, types.SimpleNamespace(inFs=q.SpS, outFs=41))
        n_symb = x.shape[0] // 41
        s = _decimate41(lib, device, _head(x, n_symb * 41))
        const = grayMapping(q.M, q.constType)
        const = const / np.sqrt(np.mean(const * np.conj(const)).real)          # the reference's pnorm of the single-precision table
        shape = s.shape
        s = detector(pnorm(s.reshape(-1)), 0.0001, const, rule="ML")[0]
        symb = pnorm(s.reshape(shape))
        if q.real_out:
            symb = _real_part(lib, device, symb)
        tx_ = _real_part(lib, device, aligned) if q.real_out else aligned.copy()

    if q.input1D:
        tx_ = tx_.reshape(-1)
    if on_dev:
        return tx_, symb
    return tx_.get(), symb.get()


def movingAverage(x, N):
    """Sliding-window mean along every column (optic/dsp/core.py:829-880): ``y[i]`` is the mean of the ``N`` samples from
    ``i - N // 2`` to ``i + (N - 1) // 2``, zeros outside the signal.  The result has ``x``'s shape and kind, in double precision."""
    from .models import _state
    if isinstance(N, (bool, np.bool_)) or int(N) != N or N < 2:
        raise ValueError(f"N = {N}: the window must be an integer of at least 2 (the reference's slice is empty for N = 1)")
    if N > MAX_N:
        raise ValueError(f"N = {N}: windows of at most {MAX_N} samples are averaged on the device")
    x, n, cols = _array(x, "x")
    if n < 1 or cols < 1 or cols > 65535:
        raise ValueError(f"x has shape {x.shape}: at least one row and 1 to 65535 columns")
    lib = _lib.load()
    on_dev = _dev.is_device(x)
    ptr, keep = _dev.arg(x, x.dtype)
    out = _dev.empty(on_dev, x.shape, np.float64 if x.dtype.kind == "f" else np.complex128)
    rc = lib.ssf_moving_average(_state["device"], n, cols, int(N), _lib.METRICS_DTYPES[x.dtype.name], ptr, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


def _prepare_bert(Irx, bitsTx, seed):
    if _dev.is_device(Irx):
        if Irx.dtype.name != "float64":
            raise TypeError(f"device array Irx has dtype {Irx.dtype.name}: float64 expected" if Irx.dtype.kind != "c" else "Irx must be real")
    else:
        Irx = np.asarray(Irx)
        if Irx.dtype.kind == "c":
            raise TypeError("Irx must be real")
        if Irx.dtype.kind not in "fiub":
            raise TypeError(f"Irx has dtype {Irx.dtype.name}: real numbers expected")
        Irx = np.ascontiguousarray(Irx, dtype=np.float64)
    n = int(Irx.size)
    if n < 1:
        raise ValueError("Irx is empty")
    if bitsTx is None:
        np.random.seed(seed=seed)
        bitsTx = np.random.randint(2, size=n)
    if _dev.is_device(bitsTx):
        if bitsTx.dtype.name not in ("int8", "uint8", "bool"):
            raise TypeError(f"device array bitsTx has dtype {bitsTx.dtype.name}: one byte per bit (int8, uint8 or bool) expected")
    else:
        bitsTx = np.asarray(bitsTx)
        if bitsTx.dtype.name not in _BIT_DTYPES:
            raise TypeError(f"bitsTx has dtype {bitsTx.dtype.name}: one of {', '.join(_BIT_DTYPES)} expected")
        bitsTx = np.ascontiguousarray(bitsTx == 1, dtype=np.uint8)       # converted once; the reference compares with 1 and with 0
        ones = int(np.count_nonzero(bitsTx))
        if ones == 0 or ones == n:
            raise ValueError("bitsTx holds only one of the two classes: the statistics of the other do not exist")
    if int(bitsTx.size) != n:
        raise ValueError(f"Irx has {n} samples and bitsTx {int(bitsTx.size)} bits")
    return Irx, bitsTx, n


def bert(Irx, bitsTx=None, seed=123):
    """Bit error rate and Q factor of an on-off-keyed intensity signal (optic/comm/metrics.py:37-105): the threshold
    ``Id = (std1 I0 + std0 I1) / (std1 + std0)`` from the class means and population standard deviations, the decisions
    ``Irx > Id`` against ``bitsTx``.  Returns ``(BER, Q)`` as Python floats; ``bert.last`` holds the other statistics."""
    from .models import _state
    Irx, bitsTx, n = _prepare_bert(Irx, bitsTx, seed)
    lib = _lib.load()
    xp, keep_x = _dev.arg(Irx, np.float64)
    bp, keep_b = _dev.arg(bitsTx, bitsTx.dtype)
    s = (C.c_double * 10)()
    _lib.raise_for(lib, None, lib.ssf_bert(_state["device"], n, xp, bp, s))
    del keep_x, keep_b
    if s[0] == 0 or s[1] == 0:
        raise ValueError("bitsTx holds only one of the two classes: the statistics of the other do not exist")
    bert.last = dict(n1=int(s[0]), n0=int(s[1]), I1=s[2], I0=s[3], std1=s[4], std0=s[5], Id=s[6], Q=s[7], errors=int(s[8]))
    return float(s[8] / n), float(s[7])


bert.last = {}


_erf = np.vectorize(math.erf, otypes=[np.float64])


def Qfunc(x):
    """Q(x) (optic/comm/metrics.py:550-569)."""
    return 0.5 - 0.5 * _erf(x / np.sqrt(2))[()]


def theoryBER(M, EbN0, constType):
    """Theoretical (approximate) bit error probability of Gray-mapped PAM / QAM / PSK over AWGN, EbN0 in dB
    (optic/comm/metrics.py:640-686), with the reference's expressions."""
    if constType not in ("qam", "psk", "pam"):
        raise ValueError(f"constType must be 'qam', 'psk' or 'pam', not {constType!r}")
    EbN0lin = 10 ** (EbN0 / 10)
    k = np.log2(M)
    if constType == "qam":
        L = np.sqrt(M)
        return 2 * (1 - 1 / L) / np.log2(L) * Qfunc(np.sqrt(3 * np.log2(L) / (L**2 - 1) * (2 * EbN0lin)))
    if constType == "psk":
        return 2 * Qfunc(np.sqrt(2 * k * EbN0lin) * np.sin(np.pi / M)) / k
    return (2 * (M - 1) / M) * Qfunc(np.sqrt(6 * np.log2(M) / (M**2 - 1) * EbN0lin)) / k
