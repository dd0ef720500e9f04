"""The theoretical-MI quadrature rule, calcMI and the GN-model helpers restated in numpy, independent of opticommpy_amd.

``rule_mi`` is the rule of include/ssf.h (``ssf_theory_mi``) in ``np.longdouble``: for every table point x_i the noise coordinate t
runs over the uniform grid {-K h .. K h}^2 with weight e^{-|t|^2} h^2 / pi, and

    MI = H(X) - sum_i px_i ( sum_t w(t) log2( sum_j px_j e^{e_ij(t)} ) - W log2 px_i ),     W = sum_t w(t),
    e_ij(t) = -( |d_ij|^2 + 2 sqrt(2) sigma Re(conj(d_ij) t) ) / (2 sigma^2),               d_ij = x_i - x_j.

The weights are not renormalised.  ``point_terms`` gives the bracket for chosen points only (what the large shape rows are held to
on the host), ``rule_mi_separable`` the exact factorisation of the same sums for a product table with uniform px (square QAM),
``rule_mi_real`` the one for a real table (PAM), where the imaginary coordinate integrates to the 1-D weight sum.

``calc_mi`` is optic/comm/metrics.py:497-547 evaluated in long double; the host functions are plain double numpy in the reference's
order of operations."""
import numpy as np

LD = np.longdouble
H_STEP, T_MAX = 0.1, 6.5
C_LIGHT, H_PLANCK = 299792458.0, 6.62607015e-34
_LOG2E = LD(1) / np.log(LD(2))


def nodes_1d(h=H_STEP, T=T_MAX):
    """(t, w): the 1-D nodes k h, |k| <= K = round(T / h), and the weights e^{-t^2} h / sqrt(pi); h is the double h, widened."""
    K = int(round(T / h))
    t = np.arange(-K, K + 1).astype(LD) * LD(h)
    return t, np.exp(-t * t) * LD(h) / np.sqrt(LD(np.pi))


def sigma_of(SNR):
    """The reference's noise standard deviation per dimension, in double as it computes it."""
    return np.sqrt((1 / 2) * 1 / (10 ** (np.asarray(SNR, dtype=np.float64) / 10)))


def entropy(px):
    px = np.asarray(px, dtype=np.float64)
    return -np.sum(px * np.log2(px))


def point_terms(table, px, sigma, idx, h=H_STEP, T=T_MAX):
    """px_i ( sum_t w log2 sum_j px_j e^{e_ij} - W log2 px_i ) for the points i in idx, long double."""
    x = np.asarray(table).astype(np.clongdouble).reshape(-1)
    p = np.asarray(px, dtype=np.float64).astype(LD)
    s = LD(float(sigma))
    t1, w1 = nodes_1d(h, T)
    tr, ti = np.meshgrid(t1, t1, indexing="ij")
    w = np.outer(w1, w1).reshape(-1)
    tr, ti = tr.reshape(-1), ti.reshape(-1)
    W = np.sum(w)
    lnp = np.log(p)
    out = np.zeros(len(idx), dtype=LD)
    r2 = np.sqrt(LD(2))
    for n, i in enumerate(idx):
        d = x[i] - x
        a, b = d.real / s, d.imag / s
        c = -(d.real ** 2 + d.imag ** 2) / (2 * s * s) + lnp
        S = np.zeros(tr.shape, dtype=LD)
        for j0 in range(0, len(x), 64):          # blocks of j: bounded memory
            j = slice(j0, j0 + 64)
            S += np.sum(np.exp(c[j][None, :] - r2 * (a[j][None, :] * tr[:, None] + b[j][None, :] * ti[:, None])), axis=1)
        out[n] = p[i] * (np.sum(w * np.log(S)) * _LOG2E - W * np.log(p[i]) * _LOG2E)
    return out


def point_terms_pair(table, px, sigma, idx, h=H_STEP, T=T_MAX):
    """(point_terms at step h, point_terms at step h / 2) from one pass over the finer grid: its nodes of even index are the
    coarser grid's nodes exactly (2k (h / 2) = k h in binary arithmetic), so the inner sums are shared."""
    x = np.asarray(table).astype(np.clongdouble).reshape(-1)
    p = np.asarray(px, dtype=np.float64).astype(LD)
    s = LD(float(sigma))
    t1, w1 = nodes_1d(h / 2, T)
    tc, wc = nodes_1d(h, T)
    assert np.array_equal(t1[::2], tc)
    lnp = np.log(p)
    r2 = np.sqrt(LD(2))
    Wf, Wc = np.sum(np.outer(w1, w1)), np.sum(np.outer(wc, wc))
    wf2, wc2 = np.outer(w1, w1), np.outer(wc, wc)
    coarse, fine = np.zeros(len(idx), dtype=LD), np.zeros(len(idx), dtype=LD)
    for n, i in enumerate(idx):
        d = x[i] - x
        a, b = d.real / s, d.imag / s
        c = -(d.real ** 2 + d.imag ** 2) / (2 * s * s) + lnp
        S = np.zeros((len(t1), len(t1)), dtype=LD)
        for j in range(len(x)):                   # e^{c - r2 (a tr + b ti)} is a product of a column and a row factor
            S += np.outer(np.exp(c[j] - r2 * a[j] * t1), np.exp(-r2 * b[j] * t1))
        L = np.log(S) * _LOG2E
        fine[n] = p[i] * (np.sum(wf2 * L) - Wf * np.log(p[i]) * _LOG2E)
        coarse[n] = p[i] * (np.sum(wc2 * L[::2, ::2]) - Wc * np.log(p[i]) * _LOG2E)
    return coarse, fine


def d4_orbits(table, tol=1e-6):
    """[(representative index, orbit size)] of a table that the symmetries of the square grid (quarter turns and reflections) map
    onto itself -- asserted, within ``tol`` -- such as PSK: the rule's value is the same for every point of an orbit."""
    x = np.asarray(table).astype(np.complex128).reshape(-1)
    onto = lambda img: np.max(np.min(np.abs(img[:, None] - x[None, :]), axis=1)) <= tol      # noqa: E731
    assert onto(np.conj(x)) and onto(-np.conj(x))                   # the reflections in the two axes
    key = np.stack([np.abs(x.real), np.abs(x.imag)], axis=1)
    if onto(1j * x):                                                # quarter turns as well (not 2-PSK): |re| and |im| may swap
        key = np.sort(key, axis=1)
    key = np.round(key / tol).astype(np.int64)
    seen = {}
    for i, k in enumerate(map(tuple, key)):
        seen.setdefault(k, []).append(i)
    return [(v[0], len(v)) for v in seen.values()]


def rule_mi(table, px, sigma, h=H_STEP, T=T_MAX):
    """The rule over all points; returns a long double."""
    table = np.asarray(table).reshape(-1)
    px = np.ones(len(table)) / len(table) if px is None else np.asarray(px, dtype=np.float64)
    return LD(entropy(px)) - np.sum(point_terms(table, px, sigma, range(len(table)), h, T))


def _terms_1d(x, p, s, h, T):
    """sum_t w1(t) log2 sum_j p_j e^{...} per point of the real table x (1-D), and the 1-D weight sum."""
    t1, w1 = nodes_1d(h, T)
    x, p = np.asarray(x, dtype=np.float64).astype(LD), np.asarray(p, dtype=np.float64).astype(LD)
    r2 = np.sqrt(LD(2))
    out = np.zeros(len(x), dtype=LD)
    for i in range(len(x)):
        d = x[i] - x
        e = -(d * d)[None, :] / (2 * s * s) - r2 * (d / s)[None, :] * t1[:, None]
        out[i] = np.sum(w1 * np.log(np.sum(p[None, :] * np.exp(e), axis=1))) * _LOG2E
    return out, np.sum(w1)


def rule_mi_real(table, px, sigma, h=H_STEP, T=T_MAX):
    """A real table: the sums over the imaginary coordinate are the 1-D weight sum."""
    x = np.asarray(table).real.reshape(-1)
    px = np.ones(len(x)) / len(x) if px is None else np.asarray(px, dtype=np.float64)
    terms, W1 = _terms_1d(x, px, LD(float(sigma)), h, T)
    p = px.astype(LD)
    return LD(entropy(px)) - np.sum(p * (W1 * terms - W1 * W1 * np.log(p) * _LOG2E))


def rule_mi_separable(levels_re, levels_im, sigma, h=H_STEP, T=T_MAX):
    """Uniform px on the product table {a + jb}: log of a product of sums is a sum of logs, each summed against the other
    coordinate's weights."""
    s = LD(float(sigma))
    na, nb = len(levels_re), len(levels_im)
    ta, W1 = _terms_1d(levels_re, np.ones(na) / na, s, h, T)
    tb, _ = _terms_1d(levels_im, np.ones(nb) / nb, s, h, T)
    M = LD(na * nb)
    log2M = np.log(M) * _LOG2E
    # per point (a, b): W1 (ta + tb) + W1^2 log2 M  (the 1-D terms carry 1/na and 1/nb, their product is px_j = 1/M)
    return log2M - (W1 * (np.sum(ta) / na + np.sum(tb) / nb) + W1 * W1 * log2M)


def calc_mi(rx, tx, sigma2, table, px):
    """optic/comm/metrics.py:497-547 in long double: first minimum of |tx - c| for the index, the direct sums of likelihoods."""
    rx, tx = np.asarray(rx).astype(np.clongdouble).reshape(-1), np.asarray(tx).astype(np.clongdouble).reshape(-1)
    c = np.asarray(table).astype(np.clongdouble).reshape(-1)
    p = np.asarray(px, dtype=np.float64).astype(LD)
    s2 = LD(float(sigma2))
    ind = np.argmin(np.abs(tx[:, None] - c[None, :]), axis=1)
    d = rx - tx
    log2_pYgX = -(1 / s2) * (d.real ** 2 + d.imag ** 2) * _LOG2E
    e = rx[:, None] - c[None, :]
    pY = np.sum(np.exp(-(1 / s2) * (e.real ** 2 + e.imag ** 2)) * p[None, :], axis=1)
    H_XgY = -np.sum(log2_pYgX + np.log(p[ind]) * _LOG2E - np.log(pY) * _LOG2E) / len(rx)
    return np.sum(-p * np.log(p) * _LOG2E) - H_XgY


# ---- the host functions, in the reference's order of operations (double)
def cond_entropy(yI, yQ, const, pX, ind, sigma):
    pi = np.pi
    prob = 0
    for ii in range(len(const)):
        xI, xQ = const[ii].real, const[ii].imag
        prob += 1 / (2 * pi * sigma**2) * np.exp(-((yI - xI) ** 2 + (yQ - xQ) ** 2) / (2 * sigma**2)) * pX[ii]
    log2pY = np.log2(max([prob, 1e-50]))
    xI, xQ = const[ind].real, const[ind].imag
    expTerm = 1 / (2 * pi * sigma**2) * np.exp(-((yI - xI) ** 2 + (yQ - xQ) ** 2) / (2 * sigma**2))
    int1 = expTerm * np.log2(max([expTerm, 1e-50]))
    int2 = expTerm * np.log2(pX[ind])
    int3 = expTerm * log2pY
    return -(int1 + int2 - int3) * pX[ind]


def gn_model(Rs, Nch, df, alpha, gamma, Ls, Ns, Ptx_dBm, D, Bref, Fc):
    lam = C_LIGHT / Fc * 1e-3
    c = C_LIGHT / 1.5 * 1e-3
    alpha = alpha / (10 * np.log10(np.exp(1)))
    Leff = (1 - np.exp(-2 * alpha * Ls)) / (2 * alpha)
    Leffa = 1 / (2 * alpha)
    Ptx = 10 ** (Ptx_dBm / 10) * 1e-3
    b2 = -D * lam**2 / (2 * np.pi * c)
    var = ((8 / 27) * (gamma**2) * Leff**2 * (Ptx / Rs) ** 3
           * (np.arcsinh((np.pi**2) / 2 * np.abs(b2) * Leffa * Nch ** (2 * Rs / df) * Rs**2))
           / (np.pi * np.abs(b2) * Leffa) * Bref)
    eps = (3 / 10) * np.log(1 + 6 / Ls * Leffa / np.arcsinh((np.pi**2 / 2) * np.abs(b2) * Leffa * (Nch**2) ** (2 * Rs / df) * Rs**2))
    return 2 * (Ns ** (1 + eps)) * var


def ase(alpha, Ls, Ns, NF, Bref, Fc):
    G = alpha * Ls
    NF_lin, G_lin = 10 ** (NF / 10), 10 ** (G / 10)
    nsp = (G_lin * NF_lin - 1) / (2 * (G_lin - 1))
    return 2 * (Ns * (G_lin - 1) * nsp * H_PLANCK * Fc) * Bref


def lin_osnr(Ns, Pin, alpha, Ls, OSNRin, NF=4.5, Fc=193.1e12, Bref=12.5e9):
    G = alpha * Ls
    NF_lin, G_lin = 10 ** (NF / 10), 10 ** (G / 10)
    nsp = (G_lin * NF_lin - 1) / (2 * (G_lin - 1))
    P_ase_dBm = 10 * np.log10((2 * ((G_lin - 1) * nsp * H_PLANCK * Fc) * Bref) / 1e-3)
    Pn = (Pin - OSNRin) - alpha * Ls
    out = np.zeros(Ns + 1)
    out[0] = OSNRin
    for k in range(1, Ns + 1):
        Pn_out = 10 * np.log10(10 ** ((Pn + G) / 10) + 10 ** (P_ase_dBm / 10))
        out[k] = Pin - Pn_out
        Pn = Pn_out - alpha * Ls
    return out
