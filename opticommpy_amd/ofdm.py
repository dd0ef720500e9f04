"""OFDM on the device: ``modulateOFDM`` and ``demodulateOFDM`` of the reference's ``optic/comm/ofdm.py`` as one launch each (three
with pilots) of ``engine_ofdm.hip``, on numpy arrays or on ``DeviceArray``s without a transfer, plus its host helpers ``hermit``,
``zeroPad`` and ``calcSymbolRate``.

Everything that depends only on the parameters -- which carrier is data, pilot or nothing, where the zero padding, the fftshift
and the Hermitian mirror put each of them at the transform's input, on which line between two pilots a carrier lies -- is a
*carrier plan*: small integer tables built once on the host and cached by the parameter values (``plan_cache_info``,
``release_plans``).  The kernels read their input and write their output through those tables, so no padded, shifted or mirrored
frame ever exists in memory."""
import ctypes as C
import itertools

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["modulateOFDM", "demodulateOFDM", "hermit", "zeroPad", "calcSymbolRate", "plan_cache_info", "release_plans"]

DEFAULT_PILOT = 0.25 + 0.25j       # what the reference's code uses (its docstring says 1 + 1j)
MIN_NFFT, MAX_NFFT, MAX_SPS = 4, 1 << 20, 64
_COMPLEX = (np.dtype(np.complex64), np.dtype(np.complex128))


# ------------------------------------------------------------------ host helpers
def hermit(V):
    """``[0, V, 0, conj(V) reversed]``: the spectrum of a real signal, ``2 len(V) + 2`` complex128 values."""
    V = np.asarray(V)
    n = len(V)
    Vh = np.zeros(2 * n + 2, dtype=complex)
    Vh[1:n + 1] = V
    Vh[n + 2:] = np.conjugate(V[::-1])
    return Vh


def zeroPad(x, L):
    """``x`` with ``L`` zeros in front and ``L`` behind."""
    return np.pad(x, (L, L), "constant", constant_values=0)


def calcSymbolRate(M, Rb, Nfft, Np, G, hermitSym):
    """OFDM symbol rate that carries the bit rate ``Rb`` with an ``M``-point constellation on the data carriers."""
    nData = (Nfft // 2 - 1 - Np) if hermitSym else (Nfft - Np)
    return Rb / (nData / (Nfft + G) * np.log2(M))


# ------------------------------------------------------------------ carrier plans
_PLANS = {}                # key -> plan, most recently used last
_PLAN_CAP = 16
_KEYS = itertools.count(1)  # a plan's number never comes back: the library may keep the tables of the plan it saw last


def plan_cache_info():
    """Keys ``(Nfft, SpS or None, hermitSymmetry, pilots, nulls)`` of the cached carrier plans, oldest first."""
    return list(_PLANS)


def release_plans():
    """Forget every cached carrier plan."""
    _PLANS.clear()


def _carriers(v, name):
    a = np.asarray(v if v is not None else [])
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D list of carrier indices, not of shape {a.shape}")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        if not (np.issubdtype(a.dtype, np.floating) and np.all(a == np.floor(a))):
            raise ValueError(f"{name} = {a.tolist()}: carrier indices must be integers")
    return a.astype(np.int64)


def _carrier_plan(Nfft, SpS, hermitSymmetry, pilots, nulls):
    """The tables of one parameter set (``SpS`` None: the demodulator's, without ``src_map``).  Raises ValueError for what the
    parameters cannot mean."""
    key = (Nfft, SpS, hermitSymmetry, tuple(pilots.tolist()), tuple(nulls.tolist()))
    plan = _PLANS.pop(key, None)
    if plan is not None:
        _PLANS[key] = plan
        return plan
    if Nfft < MIN_NFFT or Nfft > MAX_NFFT:
        raise ValueError(f"Nfft = {Nfft}: between {MIN_NFFT} and {MAX_NFFT} carriers are needed")
    if hermitSymmetry and Nfft % 2:
        raise ValueError(f"Nfft = {Nfft} is odd: Hermitian symmetry needs an even Nfft")
    Ns = Nfft // 2 - 1 if hermitSymmetry else Nfft
    Np, Nz = len(pilots), len(nulls)
    for name, a in (("pilotCarriers", pilots), ("nullCarriers", nulls)):
        if a.size and (a.min() < 0 or a.max() >= Ns):
            raise ValueError(f"{name} = {a.tolist()} leaves the carriers 0 .. {Ns - 1} (Ns = {Ns})")
    if len(np.unique(pilots)) != Np:
        raise ValueError(f"pilotCarriers = {pilots.tolist()} names a carrier twice")
    both = np.intersect1d(pilots, nulls)
    if both.size:
        raise ValueError(f"carriers {both.tolist()} are listed as pilot and as null")
    if Np == 1:
        raise ValueError(f"Np = 1 (pilotCarriers = {pilots.tolist()}): a line needs two pilots")
    data = np.setdiff1d(np.arange(Ns), np.union1d(pilots, nulls)).astype(np.int32)
    Ni = Ns - Np - len(np.unique(nulls))
    if Ns - Np - Nz < 1 or Ni < 1:
        raise ValueError(f"Ni = Ns - Np - Nz = {Ns} - {Np} - {Nz} = {Ns - Np - Nz}: no data carrier is left")
    if Ni != Ns - Np - Nz:
        raise ValueError(f"nullCarriers = {nulls.tolist()} names a carrier twice")
    plan = dict(key=next(_KEYS), Nfft=Nfft, SpS=SpS, Ns=Ns, Np=Np, Nz=Nz, Ni=Ni, data=data)
    ps = np.sort(pilots).astype(np.int32)
    plan["pilots"] = ps
    plan["hi"] = (np.clip(np.searchsorted(ps, np.arange(Ns), side="left"), 1, Np - 1) if Np else np.zeros(Ns)).astype(np.int32)
    # bin k of fft(frame) -> its carrier after fftshift (and the Hermitian slice 1 .. Ns), or -1
    at = np.fft.fftshift(np.arange(Nfft))                   # the bin that position i of the shifted spectrum shows
    carrier = np.arange(Nfft) - 1 if hermitSymmetry else np.arange(Nfft)
    carrier[(carrier < 0) | (carrier >= Ns)] = -1
    bins = np.empty(Nfft, dtype=np.int32)
    bins[at] = carrier
    plan["bin_carrier"] = bins
    if SpS is not None:
        if SpS < 1 or SpS > MAX_SPS:
            raise ValueError(f"SpS = {SpS}: between 1 and {MAX_SPS} samples per symbol are needed")
        if (Nfft * (SpS - 1)) % 2:
            raise ValueError(f"Nfft (SpS - 1) = {Nfft * (SpS - 1)} is odd: the zero padding cannot be split evenly")
        frame = np.zeros(Ns, dtype=np.int32)
        frame[data] = _lib.OFDM_SRC_DATA + 8 * np.arange(Ni, dtype=np.int32)
        frame[pilots] = _lib.OFDM_SRC_PILOT
        if hermitSymmetry:
            full = np.zeros(Nfft, dtype=np.int32)
            full[1:Ns + 1] = frame
            full[Ns + 2:] = np.where(frame[::-1] != 0, frame[::-1] | _lib.OFDM_SRC_CONJ, 0)
            frame = full
        pad = (Nfft * (SpS - 1)) // 2
        plan["src_map"] = np.ascontiguousarray(np.fft.fftshift(np.pad(frame, (pad, pad))), dtype=np.int32)
        assert plan["src_map"].shape == (SpS * Nfft,)
    for v in plan.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    while len(_PLANS) >= _PLAN_CAP:
        _PLANS.pop(next(iter(_PLANS)))
    _PLANS[key] = plan
    return plan


def _int_param(param, name, default):
    v = getattr(param, name, default)
    if isinstance(v, (bool, np.bool_)) or int(v) != v:
        raise ValueError(f"{name} = {v!r}: an integer is needed")
    return int(v)


def _signal(x, name):
    """The array argument: a DeviceArray as it is (its dtype is checked where the pointer is taken), numpy as complex64 / 128."""
    if _dev.is_device(x):
        if x.ndim != 1:
            raise ValueError(f"{name} has shape {x.shape}: a 1-D array is needed")
        return x
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"{name} has shape {a.shape}: a 1-D array is needed")
    if not np.issubdtype(a.dtype, np.complexfloating):
        raise ValueError(f"{name} has dtype {a.dtype.name}: a complex array is needed")
    return np.ascontiguousarray(a, dtype=np.complex64 if a.dtype == np.complex64 else np.complex128)


def _common(param, mod):
    Nfft = _int_param(param, "Nfft", 512)
    G = _int_param(param, "G", 4)
    hermitSymmetry = bool(getattr(param, "hermitSymmetry", False))
    pilot = complex(getattr(param, "pilot", DEFAULT_PILOT))
    SpS = _int_param(param, "SpS", 2) if mod else None
    pilots = _carriers(getattr(param, "pilotCarriers", None), "pilotCarriers")
    nulls = _carriers(getattr(param, "nullCarriers", None), "nullCarriers")
    plan = _carrier_plan(Nfft, SpS, hermitSymmetry, pilots, nulls)
    if G < 0 or G > Nfft:
        raise ValueError(f"G = {G}: a cyclic prefix of 0 .. Nfft = {Nfft} samples is needed")
    if plan["Np"] and pilot == 0:
        raise ValueError("pilot = 0: the channel estimate divides by the pilot symbol")
    return plan, G, pilot


def _prepare_mod(symb, param, dtype=np.complex64, route="auto"):
    """Every check and every table of a modulateOFDM call, without touching the library."""
    if np.dtype(dtype) not in _COMPLEX:
        raise ValueError(f"dtype = {np.dtype(dtype).name}: complex64 or complex128 is needed")
    x = _signal(symb, "symb")
    plan, G, pilot = _common(param, True)
    n = x.shape[0]
    if n % plan["Ni"] != 0 or n == 0:
        raise ValueError(f"Number of symbols ({n}) is not divisible by number of data carriers per OFDM frame ({plan['Ni']}).")
    F = n // plan["Ni"]
    if F * plan["SpS"] * plan["Nfft"] >= 1 << 31:
        raise ValueError(f"{F} frames of {plan['SpS'] * plan['Nfft']} samples: a call takes fewer than 2^31 samples")
    return dict(x=x, plan=plan, G=G, pilot=pilot, nframes=F, dtype=np.dtype(dtype), route=_lib.OFDM_ROUTES[route],
                nout=F * plan["SpS"] * (plan["Nfft"] + G))


def _prepare_demod(sig, param, route="auto"):
    """Every check and every table of a demodulateOFDM call, without touching the library."""
    x = _signal(sig, "sig")
    plan, G, pilot = _common(param, False)
    n = x.shape[0]
    if n % (plan["Nfft"] + G) != 0 or n == 0:
        raise ValueError(f"Number of received symbols ({n}) is not divisible by Nfft + G ({plan['Nfft'] + G}).")
    F = n // (plan["Nfft"] + G)
    if F * plan["Nfft"] >= 1 << 31:
        raise ValueError(f"{F} frames of {plan['Nfft']} samples: a call takes fewer than 2^31 samples")
    return dict(x=x, plan=plan, G=G, pilot=pilot, nframes=F, route=_lib.OFDM_ROUTES[route],
                returnChannel=bool(getattr(param, "returnChannel", False)))


def _params(q, in_dtype, out_dtype):
    plan = q["plan"]
    code = {np.dtype(np.complex64): _lib.SSF_C64, np.dtype(np.complex128): _lib.SSF_C128}
    return _lib.OfdmParams(nframes=q["nframes"], Nfft=plan["Nfft"], G=q["G"], SpS=plan["SpS"] or 1, Ns=plan["Ns"], Ni=plan["Ni"],
                           Np=plan["Np"], in_dtype=code[np.dtype(in_dtype)], out_dtype=code[np.dtype(out_dtype)], route=q["route"],
                           reserved=0, pilot_re=q["pilot"].real, pilot_im=q["pilot"].imag, plan_key=plan["key"])


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _in_ptr(x):
    if _dev.is_device(x) and x.dtype not in _COMPLEX:
        return _dev.arg(x, np.complex128)       # raises the TypeError of a DeviceArray of the wrong type
    return _dev.arg(x, x.dtype)


def modulateOFDM(symb, param=None, *, dtype=np.complex64, _route="auto"):
    """OFDM modulator (optic/comm/ofdm.py: modulateOFDM).

    ``symb``: 1-D complex64 or complex128, numpy or ``DeviceArray``, a whole number of frames of ``Ni`` symbols.  ``param.Nfft``
    (512), ``G`` (4), ``hermitSymmetry`` (False), ``pilot`` (0.25 + 0.25j), ``SpS`` (2), ``pilotCarriers``, ``nullCarriers`` as
    in the reference.  Returns ``numFrames SpS (Nfft + G)`` samples of the kind ``symb`` is: every frame's
    ``ifft(fftshift(zero-padded carriers)) sqrt(SpS Nfft)`` behind its cyclic prefix.

    As in the reference the frame's values are single precision (a complex128 symbol and the pilot are rounded) and the result is
    complex64; the transform itself runs in double and is rounded once.  ``dtype=np.complex128`` returns the same computation
    without that last rounding -- what ``firFilter`` and ``decimate`` take -- so ``modulateOFDM(x, p, dtype=np.complex128)
    .astype(np.complex64)`` equals the default output byte for byte."""
    from .models import _state
    q = _prepare_mod(symb, param, dtype, _route)
    x, plan = q["x"], q["plan"]
    xp, keep = _in_ptr(x)
    lib = _lib.load()
    p = _params(q, x.dtype, q["dtype"])
    out = _dev.empty(_dev.is_device(x), (q["nout"],), q["dtype"])
    rc = lib.ssf_ofdm_modulate(_state["device"], C.byref(p), _ip(plan["src_map"]), xp, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


def demodulateOFDM(sig, param=None, *, _route="auto"):
    """OFDM demodulator with pilot-based single-tap equalisation (optic/comm/ofdm.py: demodulateOFDM).

    ``sig``: 1-D complex64 or complex128 at one sample per symbol, numpy or ``DeviceArray``, a whole number of frames of
    ``Nfft + G`` samples.  ``param`` as for ``modulateOFDM`` (``SpS`` is not used), plus ``returnChannel`` (False).  Per frame:
    cut the prefix, ``fftshift(fft(frame)) / sqrt(Nfft)``, with Hermitian symmetry keep the carriers ``1 .. Ns``.  With pilots the
    channel is the mean over the frames of ``|Y[pilots] / pilot|`` and of its angle (not unwrapped, as in the reference), each
    joined by straight lines over the carriers with the end segments running on, and every frame is divided by it.  Returns the
    data carriers of all frames, flat, in the dtype and kind of ``sig``; with ``returnChannel`` also ``H``, ``Ns`` complex128
    values of the same kind, or ``0j`` without pilots.

    **``sig`` is never written.**  The reference transforms inside a view of its argument and so overwrites the caller's array;
    this function does not.  All arithmetic is double and a complex64 result is rounded once, where the reference rounds a
    complex64 signal after the transform and again after the division."""
    from .models import _state
    q = _prepare_demod(sig, param, _route)
    x, plan = q["x"], q["plan"]
    xp, keep = _in_ptr(x)
    lib = _lib.load()
    on_dev = _dev.is_device(x)
    p = _params(q, x.dtype, x.dtype)
    out = _dev.empty(on_dev, (q["nframes"] * plan["Ni"],), x.dtype)
    want_H = q["returnChannel"] and plan["Np"] > 0
    H = _dev.empty(on_dev, (plan["Ns"],), np.complex128) if want_H else None
    rc = lib.ssf_ofdm_demodulate(_state["device"], C.byref(p), _ip(plan["bin_carrier"]), _ip(plan["data"]),
                                 _ip(plan["pilots"]) if plan["Np"] else None, _ip(plan["hi"]) if plan["Np"] else None, xp,
                                 _dev.out_ptr(out), _dev.out_ptr(H) if want_H else None)
    _lib.raise_for(lib, None, rc)
    del keep
    if q["returnChannel"]:
        return out, (H if want_H else 0j)
    return out
