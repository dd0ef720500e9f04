"""The first-order perturbation model of the reference (optic/models/perturbation.py) restated in vectorised numpy, in double.

With ``m = j - L``, ``n = L - i`` and ``x`` zero outside ``[0, N)`` the reference's triple-product sum over its (2L+1)^2 window is

    P[s, m]  = x[s] conj(x[s+m]) + y[s] conj(y[s+m])
    A[t, m]  = sum_n C_ifwm[L-n, L+m] P[t+n, m]
    dx[t]    = sum_m x[t+m] A[t, m]  +  x[t] sum_n C_ixpm[L-n, L] |y[t+n]|^2
    dy[t]    = sum_m y[t+m] A[t, m]  +  y[t] sum_n C_ixpm[L-n, L] |x[t+n]|^2
    phi_x[t] = Im( sum_m C_ixpm[L, L+m] (2 |x[t+m]|^2 + |y[t+m]|^2) + (|x[t+o]|^2 + |y[t+o]|^2) C_ispm )

with ``o = -L`` ('AM': ``Xm_flat[0]`` is the window's first column) or the column of the largest ``|C|`` ('AMR').  A ``keep`` mask
over the (2L+1, 2L+1) matrix restricts every sum to the kept coefficients, as ``calcNLINperturbationSimplified`` does."""
import numpy as np


def select(C_ifwm, C_ixpm, C_ispm, coeffTol):
    """The reference's coefficient reduction: (keep mask, nReducedCoeffs, reductionFactor, column offset of Xm_flat[0])."""
    D = C_ifwm.shape[0] - 1
    L = D // 2
    C = np.asarray(C_ifwm, dtype=complex) + np.asarray(C_ixpm, dtype=complex)
    C[D, D] = C_ispm
    absC = np.abs(C.flatten())
    with np.errstate(divide="ignore"):
        n = int(np.sum(20 * np.log10(absC / np.max(absC)) > coeffTol))
    ind = np.argsort(-absC)[:n]
    keep = np.zeros(absC.shape, dtype=bool)
    keep[ind] = True
    return keep.reshape(C.shape), n, np.round(100 * (1 - n / len(absC)), 2), int(ind[0] % (D + 1)) - L


def _shift(v, k, N):
    """v[t + k] for t = 0 .. N - 1, zero outside."""
    out = np.zeros(N, dtype=v.dtype)
    lo, hi = max(0, -k), min(N, N - k)
    if hi > lo:
        out[lo:hi] = v[lo + k:hi + k]
    return out


def _single(v):
    return v.astype(np.complex64).astype(np.complex128)


def nlin(C_ifwm, C_ixpm, C_ispm, x, y, keep=None, ispm_offset=None, in_single=False, prec_single=False):
    """dx, dy, phi_x, phi_y; the normalisation x / sqrt(mean |x|^2) is here.  Everything is double, but: with ``in_single`` (a
    complex64 input) or ``prec_single`` (prec = complex64) the normalised symbols are rounded to single precision, as numpy's
    complex64 arithmetic and the reference's complex64 window do; with ``prec_single`` dx, dy are rounded to complex64 at the end.
    The reference's float32 products and powers in between are not imitated."""
    C_ifwm, C_ixpm = np.asarray(C_ifwm, dtype=complex), np.asarray(C_ixpm, dtype=complex)
    L = (C_ifwm.shape[0] - 1) // 2
    x = np.asarray(x, dtype=complex)
    y = np.asarray(y, dtype=complex)
    x = x / np.sqrt(np.mean(np.abs(x) ** 2))
    y = y / np.sqrt(np.mean(np.abs(y) ** 2))
    if in_single or prec_single:
        x, y = _single(x), _single(y)
    N = len(x)
    if keep is None:
        keep = np.ones(C_ifwm.shape, dtype=bool)
    Ci, Cx = np.where(keep, C_ifwm, 0), np.where(keep, C_ixpm, 0)
    o = -L if ispm_offset is None else ispm_offset
    px, py = np.abs(x) ** 2, np.abs(y) ** 2
    dx, dy = np.zeros(N, dtype=complex), np.zeros(N, dtype=complex)
    phx, phy = np.zeros(N, dtype=complex), np.zeros(N, dtype=complex)
    for m in range(-L, L + 1):
        P = x * np.conj(_shift(x, m, N)) + y * np.conj(_shift(y, m, N))
        A = np.zeros(N, dtype=complex)
        for n in range(-L, L + 1):
            c = Ci[L - n, L + m]
            if c != 0:
                A += c * _shift(P, n, N)
        dx += _shift(x, m, N) * A
        dy += _shift(y, m, N) * A
        c = Cx[L, L + m]
        phx += c * (2 * _shift(px, m, N) + _shift(py, m, N))
        phy += c * (2 * _shift(py, m, N) + _shift(px, m, N))
    Bx, By = np.zeros(N, dtype=complex), np.zeros(N, dtype=complex)
    for n in range(-L, L + 1):
        c = Cx[L - n, L]
        Bx += c * _shift(py, n, N)
        By += c * _shift(px, n, N)
    dx += x * Bx
    dy += y * By
    pw = (_shift(px, o, N) + _shift(py, o, N)) * complex(C_ispm)
    if prec_single:
        dx, dy = dx.astype(np.complex64), dy.astype(np.complex64)
    return dx, dy, np.imag(phx + pw), np.imag(phy + pw)


def pnorm(x):
    return x / np.sqrt(np.mean(x * np.conj(x)).real)


def perturbation_nlin(Ein, Pin_dBm, C_ifwm, C_ixpm, C_ispm, keep=None, ispm_offset=None, prec_single=False):
    """perturbationNLIN's scaling around ``nlin``; Ein (N, 2), never written.  A complex64 Ein is normalised in single precision
    (rounded after pnorm and again inside ``nlin``); the result is complex128 either way, to be rounded by the caller."""
    in_single = np.asarray(Ein).dtype == np.complex64
    E = np.asarray(Ein, dtype=complex)
    E = np.stack([pnorm(E[:, 0]), pnorm(E[:, 1])], axis=1)
    if in_single:
        E = _single(E)
    peak = 0.5 * 1e-3 * 10 ** (Pin_dBm / 10)
    dx, dy, phx, phy = nlin(C_ifwm, C_ixpm, C_ispm, E[:, 0], E[:, 1], keep, ispm_offset, in_single, prec_single)
    out = np.zeros(E.shape, dtype=complex)
    for k, (d, ph) in enumerate(((dx, phx), (dy, phy))):
        e = np.exp(1j * peak * ph)
        out[:, k] = np.sqrt(peak) * E[:, k] * (e - 1) + peak ** 1.5 * d * e
    return out
