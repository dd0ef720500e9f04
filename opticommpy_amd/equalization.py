"""Adaptive MIMO equalizer on the device: NLMS, CMA, RDE, data-aided RDE, DD-LMS and static stages.

Drop-in for ``mimoAdaptEqualizer`` (optic/dsp/equalization.py:125-351 with ``coreAdaptEq`` and its update rules, 354-973), the
stage between ``decimate`` / ``edc`` and ``cpr`` in the reference's coherent chain.  One library call (``ssf_mimo_eq``,
include/ssf.h) runs every stage on the GPU; a ``DeviceArray`` in gives a ``DeviceArray`` out and nothing the size of the signal
crosses the bus (the coefficients ``H`` and, with ``returnResults``, ``errSq`` come back to the host).

In every update rule row ``k + N nModes`` of ``H`` is driven by the output of mode ``k`` alone, so an ``nModes x nModes`` equalizer
is ``nModes`` independent recursions: one wavefront per output mode walks the symbols with its ``nModes nTaps`` coefficients in
registers (opticommpy_amd/csrc/engine_eq.hip).

Arguments are numpy arrays or ``DeviceArray``s, complex128 or complex64, of shape ``(n, nModes)`` or 1-D (1-D in, 1-D out).
Inputs are never written.

Scope and limits (anything else raises ``ValueError`` before anything is launched or allocated; there is no CPU fallback):

* ``alg`` entries among 'nlms', 'cma', 'rde', 'da-rde', 'dd-lms', 'static'; 'rls' and 'dd-rls' are not implemented;
* ``runWL = False`` and ``storeCoeff = False`` only;
* 1 <= ``nModes`` <= 4, 1 <= ``nTaps`` <= 64, 1 <= ``SpS`` <= 8, ``n`` >= ``nTaps`` and ``n`` >= ``nModes`` (the reference's
  transposition of a wide array is not imitated, as in ``cpr``);
* ``constType`` / ``M`` as ``cpr`` accepts them;
* ``len(alg) == len(mu) == len(L)``, every ``L[i]`` >= 1, ``sum(L)`` <= ``totalNumSymb``, ``numIter`` >= 1;
* ``symbRef`` with at least ``sum(L)`` rows and ``nModes`` columns whenever a stage is 'nlms' or 'da-rde'.

Deviations from the reference, on purpose:

* arithmetic is double whatever ``prec`` says, and ``sigOut`` is complex128 (``prec`` still decides the precision the
  constellation, ``Rcma`` and the radii are computed in before they are widened);
* ``errSq`` is float64 (the reference stores it in a complex array);
* ``errSq`` of a 'static' stage is 0 (the reference leaves ``np.empty`` garbage there);
* a string ``alg`` is taken as a one-stage list (the reference's string branch raises ``TypeError``); a scalar ``mu`` or ``L``
  likewise;
* ``param.H`` may be an array of shape ``(nModes ** 2, nTaps)`` (the reference's ``if not H`` raises for one);
* a data-aided stage without ``symbRef`` raises (the reference silently trains against ``sigIn``);
* a complex128 input is not rounded to ``prec``.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import device as _dev
from .cpr import _check_constellation
from .sisoeq import dfe, ffe, volterra  # noqa: F401  (the reference keeps them in its equalization module)
from .wdm_tx import grayMapping

__all__ = ["mimoAdaptEqualizer", "ffe", "dfe", "volterra"]

MAX_MODES, MAX_TAPS, MAX_SPS = 4, 64, 8
ALGS = tuple(_lib.EQ_ALGS)
_AIDED = ("nlms", "da-rde")
_DTYPES = ("complex128", "complex64")


def _tables(M, constType, shapingFactor, prec):
    """(constSymb, Rcma, Rrde) with the reference's expressions in ``prec`` (equalization.py:234-241, 453-456)."""
    constSymb = grayMapping(M, constType).astype(prec)
    px = np.exp(-shapingFactor * np.abs(constSymb) ** 2)
    px = px / np.sum(px)
    constSymb /= np.sqrt(np.sum(np.abs(constSymb) ** 2 * px))
    Rcma = ((np.mean(np.abs(constSymb) ** 4) / np.mean(np.abs(constSymb) ** 2)) * np.ones((1, 1)).astype(prec))[0, 0]
    Rrde = np.unique(np.abs(constSymb)).astype(prec)
    return constSymb, float(Rcma.real), Rrde.real.astype(np.float64)


def total_symbols(n, nTaps, SpS):
    """totalNumSymb of the reference: the padded signal has n + 2 (nTaps // 2) samples."""
    return int(np.fix((n + 2 * (nTaps // 2) - nTaps) / SpS + 1))


def _array(x, name):
    """(array as 2-D, was 1-D): 1-D is one mode."""
    if _dev.is_device(x):
        if x.dtype.name not in _DTYPES:
            raise TypeError(f"device array {name} has dtype {x.dtype.name}: complex128 or complex64 expected")
    else:
        x = np.asarray(x)
        if x.dtype.name not in _DTYPES:
            x = x.astype(np.complex128)
    if x.ndim not in (1, 2):
        raise ValueError(f"{name} must have one or two dimensions")
    return (x.reshape(x.shape[0], 1), True) if x.ndim == 1 else (x, False)


def _as_list(v):
    if isinstance(v, (list, tuple)):
        return list(v)
    if isinstance(v, np.ndarray):
        return list(v.reshape(-1))
    return [v]


def _prepare(sigIn, param=None, symbRef=None):
    """Every check and every host-side quantity of a call, without touching the library: a dict with the 2-D signal ``x``, ``ref``
    (or None), ``params`` (``_lib.EqParams``), ``stages`` (``_lib.EqStage`` array), ``table``, ``radii``, ``H`` (the initial
    coefficients, a fresh complex128 array), ``total``, ``input1D``, ``returnResults``."""
    numIter = getattr(param, "numIter", 1)
    nTaps = getattr(param, "nTaps", 15)
    mu = getattr(param, "mu", [1e-3])
    getattr(param, "lambdaRLS", 0.99)
    SpS = getattr(param, "SpS", 2)
    H = getattr(param, "H", [])
    L = getattr(param, "L", [])
    storeCoeff = getattr(param, "storeCoeff", False)
    runWL = getattr(param, "runWL", False)
    alg = getattr(param, "alg", ["nlms"])
    constType = getattr(param, "constType", "qam")
    M = getattr(param, "M", 4)
    shapingFactor = getattr(param, "shapingFactor", 0)
    getattr(param, "prgsBar", True)
    returnResults = getattr(param, "returnResults", False)
    prec = np.dtype(getattr(param, "prec", np.complex64))

    alg = _as_list(alg)
    for a in alg:
        if a in ("rls", "dd-rls"):
            raise ValueError(f"alg = {a!r} is not implemented on the device: use one of {', '.join(ALGS)}")
        if a not in ALGS:
            raise ValueError(f"alg entries must be among {', '.join(ALGS)}, not {a!r}")
    if not alg:
        raise ValueError("alg is empty")
    if runWL:
        raise ValueError("runWL = True (widely-linear mode) is not implemented on the device")
    if storeCoeff:
        raise ValueError("storeCoeff = True is not implemented on the device")
    if prec.name not in _DTYPES:
        raise ValueError(f"prec must be complex64 or complex128, not {prec.name}")
    for name, v, hi in (("nTaps", nTaps, MAX_TAPS), ("SpS", SpS, MAX_SPS)):
        if int(v) != v or v < 1 or v > hi:
            raise ValueError(f"{name} = {v}: it must be an integer between 1 and {hi}")
    nTaps, SpS = int(nTaps), int(SpS)
    if int(numIter) != numIter or numIter < 1:
        raise ValueError(f"numIter = {numIter}: at least one pass over stage 0 is needed")
    M = _check_constellation(M, constType)

    x, input1D = _array(sigIn, "sigIn")
    n, nModes = int(x.shape[0]), int(x.shape[1])
    if nModes < 1 or nModes > MAX_MODES:
        raise ValueError(f"sigIn has {nModes} modes: between 1 and {MAX_MODES} are equalized in one call")
    if n < nModes:
        raise ValueError(f"sigIn has shape {tuple(x.shape)}: the signals go in columns (n >= nModes); a wide array is not transposed")
    if n < nTaps:
        raise ValueError(f"sigIn has {n} samples: at least nTaps = {nTaps} are needed")
    total = total_symbols(n, nTaps, SpS)

    mu = _as_list(mu)
    L = _as_list(L) or [total]
    if not (len(alg) == len(mu) == len(L)):
        raise ValueError(f"alg, mu and L must have one entry per stage: {len(alg)}, {len(mu)} and {len(L)} given")
    for v in L:
        if int(v) != v or v < 1:
            raise ValueError(f"L = {L}: every stage needs at least one symbol")
    L = [int(v) for v in L]
    if sum(L) > total:
        raise ValueError(f"sum(L) = {sum(L)} exceeds the {total} symbols the input gives (totalNumSymb)")
    mu = np.array(mu).astype(np.float32)                      # the reference rounds the step sizes to single precision
    if not np.all(np.isfinite(mu)):
        raise ValueError("mu must be finite")

    ref = None
    if any(a in _AIDED for a in alg):
        if symbRef is None or (not _dev.is_device(symbRef) and np.size(symbRef) == 0):
            raise ValueError(f"a data-aided stage ({' or '.join(_AIDED)}) needs symbRef")
        ref, _ = _array(symbRef, "symbRef")
        if ref.shape[1] != nModes or ref.shape[0] < sum(L):
            raise ValueError(f"symbRef has shape {tuple(ref.shape)}: at least sum(L) = {sum(L)} rows and {nModes} columns are needed")

    if _dev.is_device(H) or np.size(H):
        H0 = np.array(H.get() if _dev.is_device(H) else H, dtype=np.complex128, order="C")
        if H0.shape != (nModes ** 2, nTaps):
            raise ValueError(f"param.H has shape {H0.shape}: ({nModes ** 2}, {nTaps}) expected")
    else:
        H0 = np.zeros((nModes ** 2, nTaps), dtype=np.complex128)
        for k in range(nModes):
            H0[k + k * nModes, nTaps // 2] = 1                # central spike

    constSymb, Rcma, Rrde = _tables(M, constType, shapingFactor, prec)
    stages = (_lib.EqStage * len(alg))(*[_lib.EqStage(L=L[i], alg=_lib.EQ_ALGS[alg[i]], mu=float(mu[i])) for i in range(len(alg))])
    params = _lib.EqParams(n=n, total=total, nref=0 if ref is None else int(ref.shape[0]), nModes=nModes, nTaps=nTaps, SpS=SpS,
                           dtype=_lib.METRICS_DTYPES[x.dtype.name], ref_dtype=0 if ref is None else _lib.METRICS_DTYPES[ref.dtype.name],
                           nStages=len(alg), numIter=int(numIter), M=M, nRadii=len(Rrde), Rcma=Rcma)
    return dict(x=x, ref=ref, params=params, stages=stages, table=np.ascontiguousarray(constSymb.astype(np.complex128)).view(np.float64),
                radii=np.ascontiguousarray(Rrde), H=H0, total=total, input1D=input1D, returnResults=bool(returnResults), alg=alg, L=L,
                mu=[float(m) for m in mu], nModes=nModes)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def mimoAdaptEqualizer(sigIn, param=None, symbRef=None):
    """N x N MIMO adaptive equalizer (optic/dsp/equalization.py:125-351).

    Parameters read from ``param`` with the reference's defaults: numIter (1), nTaps (15), mu ([1e-3]), SpS (2), H, L, alg
    (['nlms']), constType ('qam'), M (4), shapingFactor (0), returnResults (False), prec (complex64); storeCoeff, runWL, lambdaRLS
    and prgsBar are read as well (prgsBar is ignored).  Returns ``sigOut``, or ``(sigOut, H, errSq, Hiter)`` with
    ``param.returnResults``: ``H`` of shape ``(nModes ** 2, nTaps)`` in the reference's row order ``k + N nModes``,
    ``errSq`` float64 of shape ``(nModes, totalNumSymb)``, ``Hiter = H[:, :, None]``."""
    from .models import _state
    q = _prepare(sigIn, param, symbRef)
    lib = _lib.load()
    x, ref, total, nModes = q["x"], q["ref"], q["total"], q["nModes"]
    on_dev = _dev.is_device(x)
    xp, keep_x = _dev.arg(x, x.dtype)
    rp, keep_r = (None, None) if ref is None else _dev.arg(ref, ref.dtype)
    out = _dev.empty(on_dev, (total, nModes), np.complex128)
    H = q["H"]
    errSq = np.empty((nModes, total), dtype=np.float64) if q["returnResults"] else None
    rc = lib.ssf_mimo_eq(_state["device"], C.byref(q["params"]), q["stages"], _dp(q["table"]), _dp(q["radii"]),
                         H.ctypes.data_as(C.c_void_p), xp, rp, _dev.out_ptr(out),
                         None if errSq is None else errSq.ctypes.data_as(C.c_void_p))
    _lib.raise_for(lib, None, rc)
    del keep_x, keep_r
    if q["input1D"]:
        out = out.reshape(total)
    if q["returnResults"]:
        return out, H, errSq, H[:, :, None].copy()
    return out
