"""The first-order intrachannel NLIN model on the device: ``calcPertCoeffMatrix``, ``calcNLINperturbation``,
``calcNLINperturbationSimplified`` and ``perturbationNLIN`` of the reference's ``optic/models/perturbation.py``, the signal
functions through ``engine_nlin.hip`` on numpy arrays or on ``DeviceArray``s without a transfer.

The coefficient matrices are built on the host with numpy alone (``exp1`` by series and continued fraction) and cached per parameter
set.  What the kernels read is a *coefficient plan*: with ``m = j - L`` and ``n = L - i`` the reference's sum over its window is
``dx[t] = sum_m x[t+m] sum_n C_ifwm[L-n, L+m] P[t+n, m]`` with ``P[s, m] = x[s] conj(x[s+m]) + y[s] conj(y[s+m])``, so the plan is
a list of *passes* -- one per ``m`` that has coefficients, plus one per polarisation for the centre column of ``C_ixpm`` -- each
with its coefficients in the order of ``n``, and the centre row of ``C_ixpm`` for the phases.  In mode 'AM' every pass is dense;
in 'AMR' a pass holds only the coefficients the reference's selection keeps, and an ``m`` without any has no pass.  Plans are
cached by the content of the matrices (``plan_cache_info``, ``release_plans``); the library keeps the tables of the plans it saw
last on the device."""
import ctypes as C
import hashlib
import itertools
import logging
import types

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["calcPertCoeffMatrix", "calcNLINperturbation", "calcNLINperturbationSimplified", "perturbationNLIN",
           "plan_cache_info", "release_plans"]

MAX_ORDER = 128                     # nlin_kernels.h: kMaxL
MAX_SYMBOLS = 1 << 32
C_LIGHT = 299792458.0               # scipy.constants.c
EULER_GAMMA = 0.5772156649015329
_COMPLEX = (np.dtype(np.complex64), np.dtype(np.complex128))
PASS_IFWM, PASS_IXPM_X, PASS_IXPM_Y = 0, 1, 2       # nlin_kernels.h


# ------------------------------------------------------------------ exp1 without scipy
def exp1(z):
    """The exponential integral E1(z) for an array of complex ``z`` with ``Re z >= 0`` (here: the imaginary axis and the positive
    real axis): the power series ``-gamma - ln z - sum (-z)^k / (k k!)`` for ``|z| <= 4``, the continued fraction
    ``e^-z / (z + 1 - 1 / (z + 3 - 4 / (z + 5 - ...)))`` by the modified Lentz recurrence beyond.  ``E1(0) = inf``."""
    z = np.asarray(z, dtype=np.complex128)
    out = np.full(z.shape, np.inf + 0j, dtype=np.complex128)
    small = (np.abs(z) <= 4.0) & (z != 0)
    if np.any(small):
        zs = z[small]
        s = np.zeros_like(zs)
        term = np.ones_like(zs)
        for k in range(1, 80):
            term = term * (-zs) / k
            s += term / k
        out[small] = -EULER_GAMMA - np.log(zs) - s
    big = np.abs(z) > 4.0
    if np.any(big):
        zb = z[big]
        b = zb + 1.0
        c = np.full_like(zb, 1e300)
        d = 1.0 / b
        h = d.copy()
        live = np.ones(zb.shape, dtype=bool)
        for i in range(1, 2000):
            a = -float(i) * i
            b = b + 2.0
            d = np.where(live, 1.0 / (a * d + b), d)
            c = np.where(live, b + a / c, c)
            delta = c * d
            h = np.where(live, h * delta, h)
            live = live & (np.abs(delta - 1.0) > 1e-16)
            if not np.any(live):
                break
        out[big] = h * np.exp(-zb)
    return out


# ------------------------------------------------------------------ coefficient matrices
_COEFFS = {}
_COEFF_CAP = 8
_COEFF_FIELDS = (("D", 17), ("alpha", 0.2), ("lspan", 50), ("length", 800), ("pulseWidth", 0.5), ("gamma", 1.3), ("Fc", 193.2e12),
                 ("Rs", 32e9), ("matrixOrder", 25))


def _matrix_order(v):
    if isinstance(v, (bool, np.bool_)) or int(v) != v:
        raise ValueError(f"matrixOrder = {v!r}: an integer is needed")
    v = int(v)
    if v < 1 or v > MAX_ORDER:
        raise ValueError(f"matrixOrder = {v}: between 1 and {MAX_ORDER} is needed")
    return v


def _coeff_matrices(param):
    if bool(getattr(param, "powerWeighted", False)):
        raise ValueError("powerWeighted = True: the power-weighted coefficients are not available (the reference's own "
                         "calculation hands a complex argument to scipy.special.gammaincc, which rejects it)")
    vals = [getattr(param, k, d) for k, d in _COEFF_FIELDS]
    L = _matrix_order(vals[-1])
    key = tuple(float(v) for v in vals[:-1]) + (L,)
    hit = _COEFFS.pop(key, None)
    if hit is not None:
        _COEFFS[key] = hit
        return hit
    D, alpha_dB, lspan, length, width, gamma, Fc, Rs = key[:-1]
    # the fibre in km, s and W: beta2 from D at the carrier's wavelength, the loss per km in nepers, the share of a span that
    # counts (its effective length over its length)
    c_km = C_LIGHT * 1e-3
    T = 1.0 / Rs
    tau = width * T
    beta2 = -D * (c_km / Fc) ** 2 / (2 * np.pi * c_km)
    a_np = alpha_dB * np.log(10.0) / 10.0
    span_share = (1.0 - np.exp(-a_np * lspan)) / (a_np * lspan)
    common = 1j * (8.0 / 9.0) * gamma * tau ** 2 / (np.sqrt(3.0) * abs(beta2)) * span_share
    # row i is n = L - i, column j is m = j - L: the reference's meshgrid of m and of m reversed
    n = np.arange(L, -L - 1, -1, dtype=np.float64)[:, None]
    m = np.arange(-L, L + 1, dtype=np.float64)[None, :]
    cross = (m * n) == 0                                        # the centre row and column: E1(0) there, which the model drops
    with np.errstate(all="ignore"):
        four_wave = exp1(-1j * (m * n) * T ** 2 / (beta2 * length))
        cross_phase = 0.5 * exp1(((n - m) * T * tau / (np.sqrt(3.0) * abs(beta2) * length)) ** 2 + 0j).real
    C_ifwm = common * np.where(cross, 0.0, four_wave)
    # cross-phase terms live on the centre row and column only, and not at the centre itself (E1(0) again)
    C_ixpm = common * np.where(cross & ((n - m) != 0), cross_phase, 0.0)
    # the self-phase integral of 1 / sqrt(c + z^2) over the link, c = tau^4 / (3 beta2^2), in closed form
    C_ispm = common * np.arcsinh(length * np.sqrt(3.0) * abs(beta2) / tau ** 2)
    Cm = C_ifwm + C_ixpm
    Cm[L, L] = C_ispm
    hit = (Cm, C_ifwm, C_ixpm, complex(C_ispm), {})             # the last: this set's plans, by (mode, coeffTol)
    for a in hit[:3]:
        a.setflags(write=False)
    while len(_COEFFS) >= _COEFF_CAP:
        _COEFFS.pop(next(iter(_COEFFS)))
    _COEFFS[key] = hit
    return hit


def calcPertCoeffMatrix(param):
    """Coefficients of the first-order intrachannel perturbation model (optic/models/perturbation.py: calcPertCoeffMatrix):
    ``C, C_ifwm, C_ixpm`` of shape ``(2L+1, 2L+1)`` and the scalar ``C_ispm``, ``L = param.matrixOrder`` (25), from ``D`` (17),
    ``alpha`` (0.2), ``lspan`` (50), ``length`` (800), ``pulseWidth`` (0.5), ``gamma`` (1.3), ``Fc`` (193.2e12), ``Rs`` (32e9).
    Host only, numpy only; cached per parameter set (fresh copies are returned).  As in the reference ``C`` carries ``C_ispm`` at
    its centre.  ``powerWeighted=True`` raises ValueError (the reference itself fails there), as does a ``matrixOrder`` outside
    1 .. 128."""
    Cm, C_ifwm, C_ixpm, C_ispm, _ = _coeff_matrices(param)
    return Cm.copy(), C_ifwm.copy(), C_ixpm.copy(), C_ispm


# ------------------------------------------------------------------ coefficient plans
_PLANS = {}
_PLAN_CAP = 8
_KEYS = itertools.count(1)          # a plan's number never comes back: the library names its device tables by it


def plan_cache_info():
    """Keys ``(digest of the matrices, mode, coeffTol)`` of the cached coefficient plans, oldest first."""
    return list(_PLANS)


def release_plans():
    """Forget every cached coefficient matrix and plan on the host.  The library keeps the tables of the last eight plans it
    saw per device (a few hundred KiB each at most) until the process ends; a plan built anew gets a new number, so those
    tables are never read again and are overwritten in turn."""
    _PLANS.clear()
    _COEFFS.clear()


def _matrices(C_ifwm, C_ixpm, C_ispm):
    A, B = np.asarray(C_ifwm), np.asarray(C_ixpm)
    for name, a in (("C_ifwm", A), ("C_ixpm", B)):
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError(f"{name} has shape {a.shape}: a square matrix is needed")
        if a.shape[0] % 2 == 0:
            raise ValueError(f"{name} has order {a.shape[0]}: an odd order 2 L + 1 is needed")
    if A.shape != B.shape:
        raise ValueError(f"C_ifwm {A.shape} and C_ixpm {B.shape} differ in shape")
    L = (A.shape[0] - 1) // 2
    if L < 1 or L > MAX_ORDER:
        raise ValueError(f"the matrices have order 2 L + 1 with L = {L}: L between 1 and {MAX_ORDER} is needed")
    A = np.ascontiguousarray(A, dtype=np.complex128)
    B = np.ascontiguousarray(B, dtype=np.complex128)
    s = complex(C_ispm)
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B)) and np.isfinite(s)):
        raise ValueError("the coefficient matrices hold values that are not finite")
    return A, B, s, L


def _coeff_plan(C_ifwm, C_ixpm, C_ispm, mode, coeffTol):
    """The tables of one set of matrices.  mode 'AM': every coefficient, dense passes.  'AMR': the reference's selection."""
    A, B, s, L = _matrices(C_ifwm, C_ixpm, C_ispm)
    if mode == "AMR":
        coeffTol = float(coeffTol)
    h = hashlib.blake2b(digest_size=16)
    h.update(A.tobytes()), h.update(B.tobytes()), h.update(np.complex128(s).tobytes())
    key = (h.hexdigest(), mode, coeffTol if mode == "AMR" else None)
    plan = _PLANS.pop(key, None)
    if plan is not None:
        _PLANS[key] = plan
        return plan
    W = 2 * L + 1
    if mode == "AM":
        keep, nred, factor, off = np.ones((W, W), dtype=bool), W * W, 0.0, -L
    else:
        # the reference's own calls, on its C with the scalar in the corner
        Cm = A + B
        Cm[2 * L, 2 * L] = s
        absC = np.abs(Cm.flatten())
        with np.errstate(divide="ignore", invalid="ignore"):
            nred = int(np.sum(20 * np.log10(absC / np.max(absC)) > coeffTol))
        if nred < 1:
            raise ValueError(f"coeffTol = {coeffTol} dB keeps no coefficient (the reference fails there)")
        ind_sort = np.argsort(-absC)[:nred]
        keep = np.zeros(W * W, dtype=bool)
        keep[ind_sort] = True
        keep = keep.reshape(W, W)
        factor = np.round(100 * (1 - nred / len(absC)), 2)
        off = int(ind_sort[0] % W) - L
    dense = mode == "AM"
    passes, coef, nidx = [], [], []

    def add(kind, m, column, kept):
        # column[i] is the coefficient of n = L - i; the pass holds them by rising n
        sel = [i for i in range(W - 1, -1, -1) if dense or (kept[i] and column[i] != 0)]
        if not sel:
            return
        passes.append((kind, m, len(coef), len(sel)))
        for i in sel:
            coef.append(column[i])
            nidx.append(L - i)

    for j in range(W):
        add(PASS_IFWM, j - L, A[:, j], keep[:, j])
    add(PASS_IXPM_X, 0, B[:, L], keep[:, L])
    add(PASS_IXPM_Y, 0, B[:, L], keep[:, L])
    pm = [j - L for j in range(W) if dense or (keep[L, j] and B[L, j] != 0)]
    plan = dict(key=next(_KEYS), cache_key=key, L=L, mode=mode, dense=dense, keep=keep, nReducedCoeffs=nred, reductionFactor=factor, ispm_offset=off,
                ispm=s, passes=np.array(passes, dtype=np.int32).reshape(-1, 4), coef=np.array(coef, dtype=np.complex128),
                nidx=np.array(nidx, dtype=np.int32), phase_m=np.array(pm, dtype=np.int32),
                phase_c=np.array([B[L, m + L] for m in pm], dtype=np.complex128))
    for v in plan.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    while len(_PLANS) >= _PLAN_CAP:
        _PLANS.pop(next(iter(_PLANS)))
    _PLANS[key] = plan
    return plan


# ------------------------------------------------------------------ calls
def _prec(prec):
    try:
        p = np.dtype(prec)
    except TypeError:
        p = None
    if p not in _COMPLEX:
        raise ValueError(f"prec = {prec!r}: complex64 or complex128 is needed")
    return p


def _vector(x, name):
    if _dev.is_device(x):
        if x.ndim != 1:
            raise ValueError(f"{name} has shape {x.shape}: a 1-D array is needed")
        return x
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"{name} has shape {a.shape}: a 1-D array is needed")
    return np.ascontiguousarray(a, dtype=np.complex64 if a.dtype == np.complex64 else np.complex128)


def _prepare_calc(C_ifwm, C_ixpm, C_ispm, x, y, prec, mode, coeffTol=None):
    """Every check and every table of a calcNLINperturbation[Simplified] call, without touching the library."""
    prec = _prec(prec)
    plan = _coeff_plan(C_ifwm, C_ixpm, C_ispm, mode, coeffTol)
    x, y = _vector(x, "x"), _vector(y, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"x has {x.shape[0]} symbols and y has {y.shape[0]}")
    if _dev.is_device(x) != _dev.is_device(y):
        raise ValueError("x and y must both be numpy arrays or both be DeviceArrays")
    if x.dtype != y.dtype:
        if _dev.is_device(x):
            raise TypeError(f"device arrays x ({x.dtype.name}) and y ({y.dtype.name}) differ in dtype")
        x, y = x.astype(np.complex128), y.astype(np.complex128)
    n = x.shape[0]
    if n < 1 or n > MAX_SYMBOLS:
        raise ValueError(f"{n} symbols: between 1 and 2^32 are needed")
    return dict(entry=0, plan=plan, x=x, y=y, n=n, prec=prec, peak=0.0)


def _prepare_nlin(Ein, param):
    """Every check and every table of a perturbationNLIN call, without touching the library.  Writes the defaults into ``param``
    as the reference does -- once everything has been checked, so a call that raises leaves ``param`` as it was."""
    names = _COEFF_FIELDS[:-1] + (("powerWeighted", False), ("powerWeightN", 10), ("matrixOrder", 25))
    filled = types.SimpleNamespace(**{k: getattr(param, k, 193.1e12 if k == "Fc" else d) for k, d in names})
    mode = getattr(param, "mode", "AM")
    if mode not in ("AM", "AMR"):
        raise ValueError(f"mode = {mode!r}: 'AM' or 'AMR' is needed")
    prec = _prec(getattr(param, "prec", np.complex128))
    coeffTol = getattr(param, "coeffTol", -20)
    Pin = float(getattr(param, "Pin", 0))
    if _dev.is_device(Ein):
        E = Ein
    else:
        E = np.asarray(Ein)
        if E.ndim == 2:
            E = np.ascontiguousarray(E, dtype=np.complex64 if E.dtype == np.complex64 else np.complex128)
    if E.ndim != 2 or E.shape[1] != 2:
        raise ValueError(f"Ein has shape {tuple(E.shape)}: (N, 2) is needed")
    n = E.shape[0]
    if n < 1 or n > MAX_SYMBOLS:
        raise ValueError(f"{n} symbols: between 1 and 2^32 are needed")
    _, C_ifwm, C_ixpm, C_ispm, plans = _coeff_matrices(filled)
    which = (mode, float(coeffTol) if mode == "AMR" else None)
    plan = plans.get(which)                                     # (a parameter set names its plan without reading the matrices)
    if plan is None or plan is not _PLANS.get(plan["cache_key"]):
        plan = plans[which] = _coeff_plan(C_ifwm, C_ixpm, C_ispm, mode, coeffTol)
    for k, v in vars(filled).items():
        setattr(param, k, v)
    return dict(entry=1, plan=plan, x=E, y=None, n=n, prec=prec, peak=0.5 * 1e-3 * 10 ** (Pin / 10))


def _params(q):
    plan = q["plan"]
    code = {np.dtype(np.complex64): _lib.SSF_C64, np.dtype(np.complex128): _lib.SSF_C128}
    if q["x"].dtype not in code:
        raise TypeError(f"device array has dtype {q['x'].dtype.name}, this call needs complex64 or complex128")
    return _lib.NlinParams(n=q["n"], L=plan["L"], npass=len(plan["passes"]), ncoef=len(plan["coef"]), nphase=len(plan["phase_m"]),
                           dense=int(plan["dense"]), entry=q["entry"], in_dtype=code[q["x"].dtype], prec=code[q["prec"]],
                           ispm_offset=plan["ispm_offset"], reserved=0, ispm_re=plan["ispm"].real, ispm_im=plan["ispm"].imag,
                           peak_power=q["peak"], plan_key=plan["key"])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a.size else None


def _run(q):
    from .models import _state
    plan, x, y = q["plan"], q["x"], q["y"]
    p = _params(q)
    on_dev = _dev.is_device(x)
    xp, keepx = _dev.arg(x, x.dtype)
    yp, keepy = _dev.arg(y, y.dtype) if y is not None else (None, None)
    lib = _lib.load()
    n = q["n"]
    if q["entry"] == 1:
        outs = [_dev.empty(on_dev, (n, 2), x.dtype)]
    else:
        outs = [_dev.empty(on_dev, (n,), q["prec"]), _dev.empty(on_dev, (n,), q["prec"]), _dev.empty(on_dev, (n,), np.float64),
                _dev.empty(on_dev, (n,), np.float64)]
    ptrs = [_dev.out_ptr(o) for o in outs] + [None] * (4 - len(outs))
    rc = lib.ssf_pert_nlin(_state["device"], C.byref(p), plan["passes"].ctypes.data_as(C.POINTER(C.c_int32)) if len(plan["passes"]) else None,
                           _vp(plan["coef"]), plan["nidx"].ctypes.data_as(C.POINTER(C.c_int32)) if plan["nidx"].size else None,
                           plan["phase_m"].ctypes.data_as(C.POINTER(C.c_int32)) if plan["phase_m"].size else None, _vp(plan["phase_c"]),
                           xp, yp, *ptrs)
    _lib.raise_for(lib, None, rc)
    del keepx, keepy
    return outs


def calcNLINperturbation(C_ifwm, C_ixpm, C_ispm, x, y, prec=np.complex64):
    """First-order perturbation model (optic/models/perturbation.py: calcNLINperturbation): ``dx, dy, phi_ixpm_x, phi_ixpm_y`` for
    the symbols ``x`` and ``y`` (numpy or ``DeviceArray``, complex64 or complex128, never written), each normalised to unit mean
    power first.  ``dx``, ``dy`` have dtype ``prec``, the phases are float64; all four are of the kind ``x`` is.  With
    ``prec=complex64`` the normalised symbols are rounded to single precision, as the reference's are, and everything after that
    runs in double with one rounding of ``dx`` and ``dy`` at the end.  As in the reference the self-phase term of the phases
    takes the symbol ``L`` places before the current one."""
    return tuple(_run(_prepare_calc(C_ifwm, C_ixpm, C_ispm, x, y, prec, "AM")))


def calcNLINperturbationSimplified(C_ifwm, C_ixpm, C_ispm, x, y, coeffTol=-20, prec=np.complex64):
    """The same with the coefficients whose magnitude lies more than ``coeffTol`` dB under the largest left out
    (calcNLINperturbationSimplified): returns ``dx, dy, phi_ixpm_x, phi_ixpm_y, nReducedCoeffs, reductionFactor``.  The selection
    is the reference's, made on the host with its numpy calls on ``C = C_ifwm + C_ixpm`` with ``C_ispm`` in the corner
    ``[2L, 2L]``; the self-phase term of the phases takes the symbol at the column of the largest ``|C|``."""
    q = _prepare_calc(C_ifwm, C_ixpm, C_ispm, x, y, prec, "AMR", coeffTol)
    return tuple(_run(q)) + (q["plan"]["nReducedCoeffs"], q["plan"]["reductionFactor"])


def perturbationNLIN(Ein, param):
    """Intrachannel NLIN by the first-order perturbation model (optic/models/perturbation.py: perturbationNLIN).

    ``Ein``: ``(N, 2)`` complex64 or complex128, numpy or ``DeviceArray``.  ``param.mode`` 'AM' (default) or 'AMR' with
    ``coeffTol`` (-20 dB), ``Pin`` (0 dBm), ``prec`` (complex128), and the fibre parameters of ``calcPertCoeffMatrix`` (``Fc``
    defaults to 193.1e12 here, as in the reference); the defaults are written into ``param``.  Each column is normalised to unit
    power, normalised again inside the calculation, and ``nlin = sqrt(P) E (e^{j P phi} - 1) + P^{3/2} d e^{j P phi}`` with
    ``P`` half the launch power; all of it on the device.  Returns ``nlin`` in the dtype and kind of ``Ein``.

    **``Ein`` is never written.**  The reference overwrites the caller's array with its normalised copy; this function does
    not."""
    q = _prepare_nlin(Ein, param)
    plan = q["plan"]
    if plan["mode"] == "AMR":
        logging.info(f"Reduced complexity perturbation calculation: {plan['nReducedCoeffs']} coefficients used, "
                     f"reduction factor: {plan['reductionFactor']:.2f}%")
    return _run(q)[0]
