"""IM/DD transmitter and AWGN channel on the device: ``pamTransmitter``, ``mzm``, ``pm``, ``iqm``, ``voa``, ``upsample``, ``awgn``,
and the host-side sources ``bitSource``, ``prbsGenerator`` and ``symbolSource``.

The front of the direct-detection notebooks (optic/models/tx.py:231-352, optic/models/devices.py:56-220, 263-286,
optic/dsp/core.py:395-432, optic/models/channels.py:522-565, optic/comm/sources.py) with the reference's names, parameter objects,
defaults and return values.  Everything that touches the samples runs in HIP kernels (opticommpy_amd/csrc/imddtx_kernels.h through
``ssf_pam_tx``, ``ssf_modulate_optical``, ``ssf_awgn`` and ``ssf_upsample``); a ``DeviceArray`` in gives a ``DeviceArray`` out and
nothing the size of the signal crosses the bus.  The random draws that define a seeded reference run (symbols, bits, and the noise
of a numpy-in ``awgn``) are numpy's, on the host.  The same functions are importable from ``opticommpy_amd.tx``, ``.devices``,
``.channels``, ``.core`` and ``.sources``, the modules of the reference's layout.

Every refusal (``ValueError``, ``TypeError`` or the reference's own ``AssertionError``) is raised before anything runs on the GPU.
There is no CPU fallback."""
import ctypes as C
import math

import numpy as np

from . import _lib
from . import device as _dev
from .utils import parameters
from .wdm_tx import _symbol_source, pulseShape

_PAM_DEFAULTS = (("M", 4), ("Rs", 32e9), ("SpS", 16), ("probDist", "uniform"), ("shapingFactor", 0), ("seed", None), ("nBits", 40000),
                 ("pulseType", "nrz"), ("nFilterTaps", 256), ("pulseRollOff", 0.01), ("mzmVpi", 3), ("mzmVb", 1.5), ("mzmER", 80),
                 ("mzmScale", 0.25), ("nPolModes", 1), ("power", -3), ("returnParam", False))      # tx.py:269-285, in that order
_PRBS_TAPS = {7: (6, 5), 9: (8, 4), 11: (10, 8), 13: (12, 11), 15: (14, 13), 23: (22, 17), 31: (30, 27)}
_F64, _C128 = np.dtype(np.float64), np.dtype(np.complex128)


def _device():
    from .models import _state
    return _state["device"]


class _HipBackend:
    """The four library calls; the arguments are checked, typed and contiguous by the time they get here."""

    def pam_tx(self, nSymbols, SpS, nPol, pulse, symbols, mzmScale, Vpi, Vb, ER, amp, sig):
        lib = _lib.load()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        _lib.raise_for(lib, None, lib.ssf_pam_tx(_device(), nSymbols, SpS, nPol, len(pulse), dp(symbols), dp(pulse), mzmScale, Vpi, Vb, ER,
                                                 amp, _dev.out_ptr(sig)))

    def modulate(self, kind, n, u, Ei, ei0, Vpi, VbI, VbQ, Vphi, ERI, ERQ, out):
        lib = _lib.load()
        u_ptr, _ku = _dev.arg(u, u.dtype)
        ei_ptr, _ke = _dev.arg(Ei, np.complex128) if Ei is not None else (None, None)
        _lib.raise_for(lib, None, lib.ssf_modulate_optical(_device(), _lib.MOD_KINDS[kind], n, _dtype_code(u.dtype), u_ptr, ei_ptr, ei0.real,
                                                           ei0.imag, Vpi, VbI, VbQ, Vphi, ERI, ERQ, _dev.out_ptr(out)))

    def awgn(self, n, ncols, sig, out, complexNoise, FsB, snr_lin, un, dev_seed):
        lib = _lib.load()
        in_ptr, _keep = _dev.arg(sig, sig.dtype)
        un_ptr = un.ctypes.data_as(C.c_void_p) if un is not None else None
        _lib.raise_for(lib, None, lib.ssf_awgn(_device(), n, ncols, _dtype_code(sig.dtype), _dtype_code(out.dtype), int(complexNoise), FsB,
                                               snr_lin, in_ptr, un_ptr, dev_seed, _dev.out_ptr(out)))

    def stuff(self, rows, w, factor, scale, x, out):
        lib = _lib.load()
        in_ptr, _keep = _dev.arg(x, x.dtype)
        _lib.raise_for(lib, None, lib.ssf_upsample(_device(), rows, w, factor, scale, in_ptr, _dev.out_ptr(out)))


_backend = _HipBackend()


def _dtype_code(dt):
    return _lib.METRICS_DTYPES[np.dtype(dt).name]


def _real_or_complex(x, what):
    """A numpy argument as float64 (real kinds) or complex128 (complex kinds), C-contiguous."""
    x = np.asarray(x)
    if x.dtype.kind == "c":
        return np.ascontiguousarray(x, dtype=np.complex128)
    if x.dtype.kind in "fiub":
        return np.ascontiguousarray(x, dtype=np.float64)
    raise TypeError(f"{what}: a numeric array is needed, not dtype {x.dtype}")


def _device_operand(x, what, allowed):
    if x.dtype not in allowed:
        raise TypeError(f"{what}: device array has dtype {x.dtype.name}, this call takes {' or '.join(d.name for d in allowed)}")
    if x.device != _device():
        raise ValueError(f"{what}: device array lives on GPU {x.device}, the selected device is {_device()} (set_device)")
    return x


# ------------------------------------------------------------------ sources (optic/comm/sources.py): host numpy only
def prbsGenerator(order=23, length=None, seed=1):
    """Pseudo-random binary sequence of ``order`` 7, 9, 11, 13, 15, 23 or 31 (optic/comm/sources.py:75-134): the reference's shift
    register, its feedback expression ``(lfsr >> a) ^ (lfsr >> b) & 1`` as Python parses it, bit for bit.  Host numpy."""
    if seed is None:
        seed = 1
    if seed <= 0:
        raise ValueError("Seed must be a positive integer.")
    if order not in _PRBS_TAPS:
        raise ValueError(f"PRBS order {order} is not supported. Supported orders are 7, 9, 11, 13, 15, 23, 31.")
    if length is None or length > 2**order - 1:
        length = 2**order - 1
    tap_a, tap_b = _PRBS_TAPS[order]
    bits = np.zeros(int(length), dtype=np.int64)
    max_val = (1 << order) - 1
    lfsr = int(seed)
    for i in range(int(length)):
        bits[i] = (lfsr >> (order - 1)) & 1
        fb = (lfsr >> tap_a) ^ (lfsr >> tap_b) & 1
        lfsr = ((lfsr << 1) | fb) & max_val
    return bits


def bitSource(param):
    """Bit sequence of length ``nBits`` [1000], ``mode`` 'random' (``np.random.randint`` under ``seed``) or 'prbs' (``order`` [23],
    ``seed`` the register's start) -- optic/comm/sources.py:23-72, bit for bit.  Host numpy."""
    nBits = getattr(param, "nBits", 1000)
    mode = getattr(param, "mode", "random")
    order = getattr(param, "order", None)
    seed = getattr(param, "seed", None)
    if mode == "random":
        if seed is not None:
            np.random.seed(seed)
        return np.random.randint(0, 2, nBits)
    if mode == "prbs":
        prbs = prbsGenerator(23 if order is None else order, nBits, seed)
        if len(prbs) < nBits:
            prbs = np.tile(prbs, nBits // len(prbs) + 1)
        return prbs[:nBits]
    raise ValueError("bitSource: mode must be 'random' or 'prbs'")


def symbolSource(param):
    """Random symbols of a unit-energy constellation (optic/comm/sources.py:137-212): ``nSymbols`` [1000], ``M`` [4], ``constType``
    ['qam'; 'pam' and 'psk' as well], ``dist`` ['uniform' or 'maxwell-boltzmann'], ``shapingFactor`` [0.0], ``px`` [None],
    ``seed`` [None].  ``np.random.choice`` under ``np.random.seed``: with a seed the reference's symbols exactly.  Host numpy."""
    nSymbols = int(getattr(param, "nSymbols", 1000))
    M = getattr(param, "M", 4)
    constType = getattr(param, "constType", "qam")
    dist = getattr(param, "dist", "uniform")
    shapingFactor = getattr(param, "shapingFactor", 0.0)
    px = getattr(param, "px", None)
    seed = getattr(param, "seed", None)
    if dist not in ("uniform", "maxwell-boltzmann") and px is None:
        raise ValueError("symbolSource: dist must be 'uniform' or 'maxwell-boltzmann'")
    if px is None:
        return _symbol_source(nSymbols, M, constType, dist, shapingFactor, seed)
    from .wdm_tx import _constellation
    if seed is not None:
        np.random.seed(seed)
    const = np.asarray(_constellation(M, constType)).flatten()
    px = np.asarray(px)
    const = const / np.sqrt(np.sum(px * np.abs(const) ** 2))
    return np.random.choice(const, nSymbols, p=px)


# ------------------------------------------------------------------ pamTransmitter
def pamTransmitter(param, *, device_output=False):
    """Optical PAM transmitter (optic/models/tx.py:231-352).  Parameters (defaults, as the reference's code sets them): M [4], Rs
    [32e9], SpS [16], probDist ['uniform'], shapingFactor [0], seed [None], nBits [40000], pulseType ['nrz'], nFilterTaps [256],
    pulseRollOff [0.01], mzmVpi [3], mzmVb [1.5], mzmER [80], mzmScale [0.25], nPolModes [1], power [-3 dBm], returnParam [False];
    every default is written back on ``param``.

    Returns ``(sigTxo, symbTx)`` -- ``(sigTxo, symbTx, param)`` with ``param.returnParam`` -- where sigTxo is complex128 of shape
    (N, nPolModes), N = (nBits // log2 M) * SpS, flattened for one mode, and symbTx float64 (nSymbols, nPolModes) on the host.
    ``device_output=True`` leaves sigTxo in HBM (DeviceArray).  The symbols are numpy's draws on the host (seed + mode index per
    mode), so a seeded call returns the reference's symbols and leaves ``np.random``'s global state where the reference leaves it;
    pulse shaping, peak normalisation, the modulator and the power normalisation run on the device (``ssf_pam_tx``: four launches
    per mode, one host wait)."""
    for k, d in _PAM_DEFAULTS:
        setattr(param, k, getattr(param, k, d))
    M = param.M
    if not isinstance(M, (int, np.integer)) or M < 2 or M & (M - 1):
        raise ValueError("pamTransmitter: M must be a power of two, at least 2")
    bits = int(np.log2(M))
    nSymbols = int(param.nBits) // bits
    if nSymbols < 1:
        raise ValueError("pamTransmitter: nBits gives fewer than one symbol")
    SpS, nPol = int(param.SpS), int(param.nPolModes)
    if SpS < 1 or nPol < 1:
        raise ValueError("pamTransmitter: SpS and nPolModes must be at least 1")
    if param.probDist not in ("uniform", "maxwell-boltzmann"):
        raise ValueError("pamTransmitter: probDist must be 'uniform' or 'maxwell-boltzmann'")
    if param.pulseType in ("rrc", "rc") and param.nFilterTaps > _lib.TX_MAX_TAPS:
        raise ValueError(f"pamTransmitter: at most {_lib.TX_MAX_TAPS} pulse-shaping taps")
    if not param.mzmVpi:
        raise ValueError("pamTransmitter: mzmVpi must be non-zero")
    pp = parameters()
    pp.pulseType, pp.nFilterTaps, pp.rollOff, pp.SpS = param.pulseType, param.nFilterTaps, param.pulseRollOff, SpS
    pulse = np.ascontiguousarray(pulseShape(pp), dtype=np.float64)            # (raises ValueError for an unknown pulseType)
    if len(pulse) > _lib.TX_MAX_TAPS:
        raise ValueError(f"pamTransmitter: at most {_lib.TX_MAX_TAPS} pulse-shaping taps")
    symbols = np.empty((nPol, nSymbols), dtype=np.float64)
    for indMode in range(nPol):
        seed = None if param.seed is None else param.seed + indMode
        symbols[indMode] = _symbol_source(nSymbols, M, "pam", param.probDist, param.shapingFactor, seed)
    N = nSymbols * SpS
    sig = _dev.empty(device_output, (N, nPol), np.complex128)
    amp = float(np.sqrt(1e-3 * 10 ** (param.power / 10)))                     # sqrt(dBm2W(power)), optic/utils.py:197
    _backend.pam_tx(nSymbols, SpS, nPol, pulse, symbols, float(param.mzmScale), float(param.mzmVpi), float(-param.mzmVb),
                    float(param.mzmER), amp, sig)
    if nPol == 1:
        sig = sig.reshape(N)
    symbTx = np.ascontiguousarray(symbols.T)
    return (sig, symbTx, param) if param.returnParam else (sig, symbTx)


# ------------------------------------------------------------------ pm, mzm, iqm
def _modulate(kind, Ei, u, Vpi, VbI=0.0, VbQ=0.0, Vphi=0.0, ERI=60.0, ERQ=60.0):
    name = kind
    if _dev.is_device(u):
        _device_operand(u, name + ": u", (_F64, _C128))
    else:
        try:
            u.shape
        except AttributeError:
            u = np.array([u])
        u = _real_or_complex(u, name + ": u")
    shape = tuple(u.shape)
    ei_arr, ei0 = None, 0j
    if _dev.is_device(Ei):
        assert tuple(Ei.shape) == shape, "Ei and u need to have the same dimensions"
        ei_arr = _device_operand(Ei, name + ": Ei", (_C128,))
    else:
        scalar = not hasattr(Ei, "shape") or (np.shape(Ei) == () and shape != ())
        if not scalar:
            assert tuple(Ei.shape) == shape, "Ei and u need to have the same dimensions"
            if np.asarray(Ei).dtype.kind not in "cfiub":
                raise TypeError(f"{name}: Ei must be numeric")
        if scalar or shape == ():
            ei0 = complex(Ei)
        else:
            ei_arr = np.ascontiguousarray(Ei, dtype=np.complex128)
    for v, what in ((Vpi, "Vpi"), (VbI, "Vb"), (VbQ, "Vb"), (Vphi, "Vphi"), (ERI, "ER"), (ERQ, "ER")):
        if not math.isfinite(v):
            raise ValueError(f"{name}: {what} must be finite")
    if Vpi == 0:
        raise ValueError(f"{name}: Vpi must be non-zero")
    on_dev = _dev.is_device(u) or _dev.is_device(Ei)
    out = _dev.empty(on_dev, shape, np.complex128)
    n = int(np.prod(shape, dtype=np.int64))
    if n == 0:
        return out
    _backend.modulate(kind, n, u, ei_arr, ei0, float(Vpi), float(VbI), float(VbQ), float(Vphi), float(ERI), float(ERQ), out)
    return out


def pm(Ei, u, Vπ):
    """Optical phase modulator (optic/models/devices.py:56-91): ``Ei * exp(1j * (u / Vπ) * π)``.  Ei a scalar, a numpy array or a
    complex128 DeviceArray of u's shape; u a scalar, a numpy array or a float64 / complex128 DeviceArray (a complex drive goes
    through the formula as written).  complex128 out, a DeviceArray if either argument is one."""
    return _modulate("pm", Ei, u, Vπ)


def mzm(Ei, u, param=None):
    """Mach-Zehnder modulator (optic/models/devices.py:94-144, ``calcMZM``): Vpi [2 V], Vb [-1 V], ER [60 dB].  Arguments and
    result as ``pm``'s; gamma is derived from ER in double precision on the host, the phases ``((u + Vb) / 2 / Vpi) * π`` are
    rounded as numpy rounds them and their sines and cosines are double precision."""
    if param is None:
        param = []
    return _modulate("mzm", Ei, u, getattr(param, "Vpi", 2), VbI=getattr(param, "Vb", -1), ERI=getattr(param, "ER", 60))


def iqm(Ei, u, param=None):
    """IQ modulator (optic/models/devices.py:147-220): Vpi [2 V], VbI [-2 V], VbQ [-2 V], Vphi [1 V], ERI [60 dB], ERQ [60 dB];
    the two arms are driven by ``u.real`` and ``u.imag``.  Arguments and result as ``pm``'s."""
    if param is None:
        param = []
    return _modulate("iqm", Ei, u, getattr(param, "Vpi", 2), getattr(param, "VbI", -2), getattr(param, "VbQ", -2),
                     getattr(param, "Vphi", 1), getattr(param, "ERI", 60), getattr(param, "ERQ", 60))


# ------------------------------------------------------------------ upsample, voa
def _stuff(x, factor, scale, what):
    on_dev = _dev.is_device(x)
    if on_dev:
        if x.device != _device():
            raise ValueError(f"{what}: device array lives on GPU {x.device}, the selected device is {_device()} (set_device)")
    else:
        x = np.ascontiguousarray(x)
    if x.ndim not in (1, 2):
        raise ValueError(f"{what}: a 1-D array or an (n, m) array of columns is needed")
    words = x.dtype.itemsize // 8
    shape = (int(x.shape[0]) * factor,) + tuple(int(s) for s in x.shape[1:])
    out = _dev.empty(on_dev, shape, x.dtype)
    rows, cols = int(x.shape[0]), int(x.shape[1]) if x.ndim == 2 else 1
    if rows * cols == 0:
        return out
    _backend.stuff(rows, cols * words, factor, float(scale), x, out)
    return out


def upsample(x, factor):
    """Insert ``factor - 1`` zeros after every sample (optic/dsp/core.py:395-432); a 2-D input is upsampled column-wise.  float64,
    complex64 or complex128 (any numpy dtype of 8 or 16 bytes per element), numpy or DeviceArray; the same kind and dtype come
    back and the samples are copied bit for bit."""
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)):
        raise TypeError("upsample: factor must be an integer")
    if factor < 1:
        raise ValueError("upsample: factor must be at least 1")
    dt = x.dtype if _dev.is_device(x) else np.asarray(x).dtype
    if dt.itemsize not in (8, 16) or (_dev.is_device(x) and dt not in (_F64, _C128, np.dtype(np.complex64))):
        raise TypeError(f"upsample: float64, complex64 or complex128 arrays, not {dt.name}")
    return _stuff(x, int(factor), 1.0, "upsample")


def voa(E, A=0):
    """Variable optical attenuator (optic/models/devices.py:263-286): ``E * 10 ** (-A / 20)``, A in dB.  complex128 or float64,
    numpy or DeviceArray; the same kind and dtype come back."""
    assert A >= 0, "Attenuation should be a positive scalar"
    if not math.isfinite(A):
        raise ValueError("voa: the attenuation must be finite")
    if _dev.is_device(E):
        _device_operand(E, "voa", (_F64, _C128))
    else:
        E = _real_or_complex(E, "voa")
    if E.ndim > 2:
        E2 = E.reshape(-1)
        return _stuff(E2, 1, 10 ** (-A / 20), "voa").reshape(E.shape)
    if E.ndim == 0:
        return _stuff(E.reshape(1), 1, 10 ** (-A / 20), "voa").reshape(())
    return _stuff(E, 1, 10 ** (-A / 20), "voa")


# ------------------------------------------------------------------ awgn
def awgn(sig, param):
    """AWGN channel (optic/models/channels.py:522-565): snr [20 dB], Fs [1], B [1], complexNoise [True], seed [None];
    ``σ² = (Fs / B) * mean(|sig|²) / 10^(snr / 10)`` with the mean over every element of every column, and
    ``sig + sqrt(σ² / 2) * (zr + 1j * zi)`` (zi = 0 without ``complexNoise``).  The power is reduced and the noise scaled and added
    on the device (``ssf_awgn``: two launches, no host wait in between; a result repeats bit for bit).

    numpy in, numpy out: zr and zi are the reference's own draws from numpy's global generator, seeded or not -- the real block,
    then the imaginary block; ``np.random.normal(0, s, shape)`` is ``s * np.random.standard_normal(shape)`` element for element, so
    the host draws unit normals and the device applies its own σ.  The reference's ``gaussianNoise`` / ``gaussianComplexNoise``
    are ``@njit``: what numba's generator would draw is another stream; the definition held to here is numpy's, the reference run
    with ``njit`` as the identity.  The dtype follows ``sig + noise``: float64 for a real signal with real noise, complex128
    otherwise (other real or complex dtypes are widened first).

    DeviceArray (complex128 or float64, 1-D or (n, nModes)) in, DeviceArray out: the noise is generated on the device (Philox4x32-10
    keyed by ``param.seed``, counter = sample, row = column, a stream tag of its own; fresh entropy without a seed): statistical
    parity, as ``edfa`` documents, repeatable bit for bit per seed."""
    snr = getattr(param, "snr", 20)
    Fs = getattr(param, "Fs", 1)
    B = getattr(param, "B", 1)
    complexNoise = bool(getattr(param, "complexNoise", True))
    seed = getattr(param, "seed", None)
    if not (B > 0) or not math.isfinite(B):
        raise ValueError("awgn: B must be positive and finite")
    if not (Fs > 0) or not math.isfinite(Fs):
        raise ValueError("awgn: Fs must be positive and finite")
    if not math.isfinite(snr):
        raise ValueError("awgn: snr must be finite")
    try:
        snr_lin = 10 ** (snr / 10)
    except OverflowError:
        snr_lin = math.inf
    if not (snr_lin > 0) or not math.isfinite(snr_lin):
        raise ValueError("awgn: 10^(snr / 10) is not a positive finite number")
    on_dev = _dev.is_device(sig)
    if on_dev:
        _device_operand(sig, "awgn", (_F64, _C128))
        if sig.ndim not in (1, 2):
            raise ValueError("awgn: a 1-D or (n, nModes) device array is needed")
    else:
        sig = _real_or_complex(sig, "awgn")
    shape = tuple(int(s) for s in sig.shape)
    total = int(np.prod(shape, dtype=np.int64))
    if total < 1:
        raise ValueError("awgn: the signal is empty")
    ncols = shape[1] if (on_dev and len(shape) == 2) else 1
    out_dtype = _C128 if (complexNoise or sig.dtype == _C128) else _F64
    if on_dev:
        from .models import _device_seed
        un, dev_seed = None, _device_seed(seed)
    else:
        if seed is not None:
            np.random.seed(seed)
        un = np.empty((2 if complexNoise else 1, total), dtype=np.float64)
        un[0] = np.random.standard_normal(shape).reshape(-1)
        if complexNoise:
            un[1] = np.random.standard_normal(shape).reshape(-1)
        dev_seed = 0
    out = _dev.empty(on_dev, shape, out_dtype)
    _backend.awgn(total // ncols, ncols, sig, out, complexNoise, float(Fs / B), float(snr_lin), un, dev_seed)
    return out
