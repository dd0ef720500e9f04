"""Theoretical mutual information on the device, the Monte-Carlo ``calcMI``, and the GN-model helpers on the host.

Drop-in for ``theoryMI``, ``calcMI``, ``condEntropy``, ``GN_Model_NyquistWDM``, ``ASE_NyquistWDM``, ``GNmodel_OSNR`` and
``calcLinOSNR`` (optic/comm/metrics.py:497-547, 689-1005), plus ``constellationMI``: the same integral for an arbitrary table.

``theoryMI`` evaluates H(X) - H(X|Y) of the discrete-input AWGN channel by quadrature (``ssf_theory_mi``, include/ssf.h): a
uniform grid in the normalised noise coordinate t, spacing h = 0.1 on [-6.5, 6.5]^2 (131 x 131 nodes), weight e^{-|t|^2} h^2 / pi.
The integrand is analytic with Gaussian decay, the trapezoid rule's best case: the rule is within 1e-10 (absolute, bits) of the
integral, measured against h / 2 in extended precision (profiles/theory_quadrature.json; worst measured case far below that).
The table, Es, sigma and H(X) are formed with the reference's expressions: the table stays complex64 through its normalisation and
is widened afterwards, ``Es`` is the uniform mean power even when ``pX`` is given, sigma = sqrt(1/2 * 1/dB2lin(SNR)).

Deviations from the reference, on purpose:

* ``symmetry`` is accepted and ignored: every point is integrated.  The reference's ``symmetry=True`` groups points by ``|x|``, which
  is wrong for 64-QAM and above: (7 + 1j) and (5 + 5j) share sqrt(50) without being images of each other under any symmetry of the
  grid.  At 64-QAM and 15 dB the reference returns 4.70459 (9 groups); integrating all 64 points gives 4.68143, which is what this
  function returns.
* ``lim`` other than ``np.inf`` raises ``ValueError`` (the rule has its own, fixed range).
* ``tol`` below the rule's bound of 1e-10 raises ``ValueError``; a larger ``tol`` changes nothing (the reference's dblquad needs
  seconds to minutes per point without a JIT, and its error follows ``tol``).
* ``SNR`` may be a 1-D sequence of up to 4096 values: one library call, an array back.  A scalar gives a float.
* ``calcMI`` never writes its inputs and brings one number back; they may be DeviceArrays.

There is no CPU fallback for ``theoryMI``, ``constellationMI`` and ``calcMI``: without the library or without a GPU they raise.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import device as _dev
from .wdm_tx import grayMapping

__all__ = ["theoryMI", "constellationMI", "calcMI", "condEntropy", "GN_Model_NyquistWDM", "ASE_NyquistWDM", "GNmodel_OSNR", "calcLinOSNR"]

RULE_STEP, RULE_RANGE, RULE_BOUND = 0.1, 6.5, 1e-10
MAX_POINTS, MAX_SNRS = 1024, 4096
_C_LIGHT, _H_PLANCK = 299792458.0, 6.62607015e-34           # exact SI values (scipy.constants.c, .h)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _check_px(pX, M):
    if pX is None:
        return 1 / M * np.ones(M)
    pX = np.asarray(pX, dtype=np.float64).reshape(-1)
    if pX.shape != (M,):
        raise ValueError(f"pX must hold M = {M} probabilities")
    if not np.all(np.isfinite(pX)) or not np.all(pX > 0):
        raise ValueError("pX must hold finite values > 0")
    return np.ascontiguousarray(pX)


def _sigma(SNR):
    """(sigma as a 1-D float64 array, whether SNR was a scalar)."""
    snr = np.asarray(SNR, dtype=np.float64)
    scalar = snr.ndim == 0
    snr = snr.reshape(1) if scalar else snr
    if snr.ndim != 1 or not 1 <= snr.shape[0] <= MAX_SNRS:
        raise ValueError(f"SNR must be a scalar or a 1-D sequence of 1 .. {MAX_SNRS} values")
    if not np.all(np.isfinite(snr)):
        raise ValueError("SNR must be finite")
    with np.errstate(over="ignore"):
        sigma = np.sqrt((1 / 2) * 1 / (10 ** (snr / 10)))    # noise deviation per dimension
    if not np.all(np.isfinite(sigma)) or not np.all(sigma > 0):
        raise ValueError("SNR is out of range: sigma is not a positive number")
    return np.ascontiguousarray(sigma), scalar


def _table(constSymb):
    t = np.asarray(constSymb)
    if t.ndim != 1 or not 1 <= t.shape[0] <= MAX_POINTS:
        raise ValueError(f"the table must be a 1-D sequence of 1 .. {MAX_POINTS} points")
    t = np.ascontiguousarray(t.astype(np.complex128))
    if not np.all(np.isfinite(t.view(np.float64))):
        raise ValueError("the table must be finite")
    return t


def _theory_table(M, constType):
    """The reference's table: grayMapping, divided by the square root of its uniform mean power in its own (single) precision,
    then widened."""
    from .metrics import _check_constellation
    M = _check_constellation(M, constType)
    const = grayMapping(M, constType)
    Es = np.sum(np.mean(const * np.conj(const), axis=0).real)
    const = const / np.sqrt(Es)
    assert const.dtype in (np.complex64, np.float32)
    return const.astype(np.complex128)


def _integrate(table, pX, sigma):
    from .models import _state
    lib = _lib.load()
    out = np.empty(sigma.shape[0], dtype=np.float64)
    rc = lib.ssf_theory_mi(_state["device"], table.shape[0], sigma.shape[0], _dp(table.view(np.float64)), _dp(pX), _dp(sigma), _dp(out))
    _lib.raise_for(lib, None, rc)
    return out


def theoryMI(M, constType, SNR, pX=None, symmetry=True, lim=np.inf, tol=1e-3):
    """Mutual information [bits] of the Gray-mapped constellation on the AWGN channel at ``SNR`` [dB]
    (optic/comm/metrics.py:770-848).  ``symmetry`` is ignored: all M points are integrated (see the module's notes)."""
    table = _theory_table(M, constType)
    if lim != np.inf:
        raise ValueError("lim: the rule integrates over its own fixed range; only np.inf is accepted")
    if not tol >= RULE_BOUND:
        raise ValueError(f"tol = {tol} is below the rule's bound of {RULE_BOUND}")
    pX = _check_px(pX, table.shape[0])
    sigma, scalar = _sigma(SNR)
    mi = _integrate(table, pX, sigma)
    return float(mi[0]) if scalar else mi


def constellationMI(constSymb, SNR, pX=None):
    """``theoryMI`` for an arbitrary table of 1 .. 1024 points, real or complex, used as given (no normalisation); sigma from
    ``SNR`` [dB] as in ``theoryMI``, i.e. for a table of unit mean power."""
    table = _table(constSymb)
    pX = _check_px(pX, table.shape[0])
    sigma, scalar = _sigma(SNR)
    mi = _integrate(table, pX, sigma)
    return float(mi[0]) if scalar else mi


def _sequence(x, name):
    if _dev.is_device(x):
        if x.dtype.name not in _lib.METRICS_DTYPES:
            raise TypeError(f"{name} has dtype {x.dtype.name}: complex128, complex64, float64 or float32 expected")
    else:
        x = np.asarray(x)
        if x.dtype.name not in _lib.METRICS_DTYPES:
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if x.ndim != 1 or x.shape[0] < 1:
        raise ValueError(f"{name} must be a non-empty 1-D sequence")
    return x


def calcMI(rx, tx, σ2, constSymb, pX):
    """Monte-Carlo mutual information of ``rx`` against ``tx`` for noise variance ``σ2`` (optic/comm/metrics.py:497-547), the
    reference's direct form in double.  Returns a float64 array of shape (1,), as the reference does."""
    from .models import _state
    table = _table(constSymb)
    pX = _check_px(pX, table.shape[0])
    σ2 = float(σ2)
    if not (σ2 > 0 and np.isfinite(σ2)):
        raise ValueError("σ2 must be a finite number > 0")
    rx, tx = _sequence(rx, "rx"), _sequence(tx, "tx")
    if rx.shape != tx.shape:
        raise ValueError(f"rx and tx differ in length: {rx.shape[0]} and {tx.shape[0]}")
    if rx.dtype != tx.dtype:
        if _dev.is_device(rx) or _dev.is_device(tx):
            raise TypeError(f"rx is {rx.dtype.name}, tx is {tx.dtype.name}: device arrays are not converted")
        both = np.complex128 if (np.iscomplexobj(rx) or np.iscomplexobj(tx)) else np.float64
        rx, tx = rx.astype(both), tx.astype(both)
    lib = _lib.load()
    prx, keep_rx = _dev.arg(rx, rx.dtype)
    ptx, keep_tx = _dev.arg(tx, tx.dtype)
    out = np.zeros(1, dtype=np.float64)
    rc = lib.ssf_calc_mi(_state["device"], rx.shape[0], _lib.METRICS_DTYPES[rx.dtype.name], table.shape[0], σ2,
                         _dp(table.view(np.float64)), _dp(pX), prx, ptx, _dp(out))
    _lib.raise_for(lib, None, rc)
    del keep_rx, keep_tx
    return out


# ---- host numpy: the reference's expressions in the reference's order
def condEntropy(yI, yQ, const, pX, ind, σ):
    """The integrand of the reference's theoryMI at y = yI + j yQ for transmitted point ``ind``
    (optic/comm/metrics.py:689-747); kept for callers that integrate it themselves."""
    π = np.pi
    prob = 0
    for ii in range(len(const)):
        xI = const[ii].real
        xQ = const[ii].imag
        prob += 1 / (2 * π * σ**2) * np.exp(-((yI - xI) ** 2 + (yQ - xQ) ** 2) / (2 * σ**2)) * pX[ii]
    log2pY = np.log2(max([prob, 1e-50]))
    xI = const[ind].real
    xQ = const[ind].imag
    expTerm = 1 / (2 * π * σ**2) * np.exp(-((yI - xI) ** 2 + (yQ - xQ) ** 2) / (2 * σ**2))
    int1 = expTerm * np.log2(max([expTerm, 1e-50]))
    int2 = expTerm * np.log2(pX[ind])
    int3 = expTerm * log2pY
    return -(int1 + int2 - int3) * pX[ind]


def GN_Model_NyquistWDM(Rs, Nch, Δf, α, γ, Ls, Ns, Ptx_dBm, D, Bref, Fc):
    """NLI noise power in ``Bref`` of a Nyquist-WDM comb after ``Ns`` spans by the GN model, Poggiolini JLT 30 (2012) Eq. (15)
    (optic/comm/metrics.py:851-898)."""
    λ = _C_LIGHT / Fc * 1e-3                                  # wavelength [km]
    c = _C_LIGHT / 1.5 * 1e-3                                 # speed of light in the fibre [km/s]
    α = α / (10 * np.log10(np.exp(1)))
    Leff = (1 - np.exp(-2 * α * Ls)) / (2 * α)
    Leffa = 1 / (2 * α)
    Ptx = 10 ** (Ptx_dBm / 10) * 1e-3
    β2 = -D * λ**2 / (2 * np.pi * c)
    var_NLI = (
        (8 / 27) * (γ**2) * Leff**2 * (Ptx / Rs) ** 3
        * (np.arcsinh((np.pi**2) / 2 * np.abs(β2) * Leffa * Nch ** (2 * Rs / Δf) * Rs**2))
        / (np.pi * np.abs(β2) * Leffa) * Bref
    )
    epsilon = (3 / 10) * np.log(1 + 6 / Ls * Leffa / np.arcsinh((np.pi**2 / 2) * np.abs(β2) * Leffa * (Nch**2) ** (2 * Rs / Δf) * Rs**2))
    return 2 * (Ns ** (1 + epsilon)) * var_NLI


def ASE_NyquistWDM(α, Ls, Ns, NF, Bref, Fc):
    """ASE noise power in ``Bref`` after ``Ns`` spans whose amplifiers make up the span loss, Essiambre JLT 28 (2010) Eq. (54)
    (optic/comm/metrics.py:901-914)."""
    G = α * Ls
    NF_lin = 10 ** (NF / 10)
    G_lin = 10 ** (G / 10)
    nsp = (G_lin * NF_lin - 1) / (2 * (G_lin - 1))
    N_ase = Ns * (G_lin - 1) * nsp * _H_PLANCK * Fc
    return 2 * N_ase * Bref


def GNmodel_OSNR(Rs, Nch, Δf, Ptx, paramCh=None, Bref=12.5e9):
    """(OSNR, P_nli, P_ase) per launch power of ``Ptx`` [dBm] (optic/comm/metrics.py:917-939); OSNR is linear."""
    if paramCh is None:
        paramCh = []
    Ltotal = getattr(paramCh, "Ltotal", 800)
    Ls = getattr(paramCh, "Lspan", 50)
    α = getattr(paramCh, "alpha", 0.2)
    D = getattr(paramCh, "D", 16)
    γ = getattr(paramCh, "gamma", 1.3)
    Fc = getattr(paramCh, "Fc", 193.1e12)
    NF = getattr(paramCh, "NF", 4.5)
    Ns = Ltotal // Ls
    OSNR, P_nli, P_ase = np.zeros(len(Ptx)), np.zeros(len(Ptx)), np.zeros(len(Ptx))
    for k, Ptx_dBm in enumerate(Ptx):
        P_nli[k] = GN_Model_NyquistWDM(Rs, Nch, Δf, α, γ, Ls, Ns, Ptx_dBm, D, Bref, Fc)
        P_ase[k] = ASE_NyquistWDM(α, Ls, Ns, NF, Bref, Fc)
        OSNR[k] = 10 ** (Ptx_dBm / 10) * 1e-3 / (P_nli[k] + P_ase[k])
    return OSNR, P_nli, P_ase


def calcLinOSNR(Ns, Pin, α, Ls, OSNRin, NF=4.5, Fc=193.1e12, Bref=12.5e9):
    """OSNR [dB] at the launch and after each of ``Ns`` spans of fibre + EDFA (optic/comm/metrics.py:942-1005)."""
    G = α * Ls
    NF_lin = 10 ** (NF / 10)
    G_lin = 10 ** (G / 10)
    nsp = (G_lin * NF_lin - 1) / (2 * (G_lin - 1))
    N_ase = (G_lin - 1) * nsp * _H_PLANCK * Fc
    P_ase_dBm = 10 * np.log10((2 * N_ase * Bref) / 1e-3)     # ASE power generated per EDFA
    Pn_in_edfa = (Pin - OSNRin) - α * Ls                      # noise power sent to the first EDFA
    OSNR = np.zeros(Ns + 1)
    OSNR[0] = OSNRin
    for spanN in range(1, Ns + 1):
        Pn_out_edfa = 10 * np.log10(10 ** ((Pn_in_edfa + G) / 10) + 10 ** (P_ase_dBm / 10))
        OSNR[spanN] = Pin - Pn_out_edfa
        Pn_in_edfa = Pn_out_edfa - α * Ls
    return OSNR
