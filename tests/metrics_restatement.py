"""The link metrics restated in plain vectorised numpy, from the definitions in the docstrings of opticommpy_amd/metrics.py and the
formulas of opticommpy_amd/csrc/metrics_kernels.h: what tests/test_metrics_restatement.py and tests/test_gpu_metrics_shapes.py
hold the kernels to at shapes no recorded fixture has.

Only the constellation tables (raw, norm, px, Es, H) come from the package (opticommpy_amd.metrics._tables / _evm_tables; they
carry the reference's single-precision quirks and tests/test_metrics_host.py holds them to the reference value for value).
Everything per symbol is written here: the rotation by mean(tx / rx), the per-column unit power, nearest-point decisions, the
Hamming distance of point indices, the residual's variance, the LLRs in the direct form (sums of likelihoods, log p0 - log p1,
+-inf clipped to +-500), the MI term, the data-aided EVM with its joint normalisation and the blind EVM with the single-precision
table and a float32 np.mean in the denominator.  Means are accumulated in np.longdouble.

Besides the values, every function returns what a test needs to know that a comparison is meaningful: the smallest decision
margin (the gap between the distances to the two nearest points, in raw-table units), the number of clipped LLRs, the smallest
likelihood sum that a logarithm was taken of and the bit errors per mode."""
import numpy as np

from opticommpy_amd import metrics as om

LD = np.longdouble
_CHUNK = 1 << 21            # distance-matrix elements held at a time


def as_columns(x, discard=0):
    """(n, nModes) array in double precision under the reference's shape rules, rows [discard : n - discard]."""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    elif x.shape[1] > x.shape[0]:
        x = x.T
    return x[discard:x.shape[0] - discard]


def mean(x):
    """Mean over the first axis, accumulated in extended precision; complex values as two real sums."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return complex(float(np.sum(x.real.astype(LD), axis=0) / x.shape[0]), float(np.sum(x.imag.astype(LD), axis=0) / x.shape[0]))
    return float(np.sum(x.astype(LD), axis=0) / x.shape[0])


def nearest(symb, table):
    """Index of the nearest table point (first minimum) per symbol, and the smallest gap between the nearest and the
    second-nearest distance."""
    symb = np.asarray(symb).reshape(-1)
    table = np.asarray(table)
    idx = np.empty(symb.shape[0], dtype=np.int64)
    gap = np.inf
    step = max(1, _CHUNK // len(table))
    for a in range(0, symb.shape[0], step):
        d = np.abs(symb[a:a + step, None] - table[None, :])
        idx[a:a + step] = np.argmin(d, axis=1)
        two = np.partition(d, 1, axis=1)[:, :2]
        gap = min(gap, float(np.min(two[:, 1] - two[:, 0])))
    return idx, gap


def popcount(v):
    v = np.asarray(v, dtype=np.int64)
    c = np.zeros(v.shape, dtype=np.int64)
    for j in range(11):
        c += (v >> j) & 1
    return c


def _table(c, real):
    return np.ascontiguousarray(c.real) if real else c


def restate(rx, tx, M, constType, px=None, discard=0):
    """BER, SER, SNR [dB], GMI, NGMI, MI, EVM per mode, and 'bit_errors' (per mode), 'margin', 'clipped', 'min_sum'."""
    raw, norm, pxa, Es, H = om._tables(M, constType, px)
    B = int(M).bit_length() - 1
    r_all, t_all = as_columns(rx, discard), as_columns(tx, discard)
    real = not np.iscomplexobj(r_all)
    raw, norm = _table(raw, real), _table(norm, real)
    n, modes = r_all.shape
    rotate = constType in ("qam", "psk")
    labels = np.arange(M)
    out = {k: np.zeros(modes) for k in ("BER", "SER", "SNR", "GMI", "NGMI", "MI", "EVM")}
    out["bit_errors"] = np.zeros(modes, dtype=np.int64)
    margin, clipped, min_sum = np.inf, 0, np.inf

    # data-aided EVM: both arrays to unit power over all modes together, then the rotation, no second normalisation
    jr = np.sqrt(mean(np.abs(r_all.reshape(-1)) ** 2))
    jt = np.sqrt(mean(np.abs(t_all.reshape(-1)) ** 2))

    for k in range(modes):
        r, t = r_all[:, k], t_all[:, k]
        if rotate:
            r = mean(t / r) * r
        r = r / np.sqrt(mean(np.abs(r) ** 2))
        t = t / np.sqrt(mean(np.abs(t) ** 2))
        d = r - t
        out["SNR"][k] = 10 * np.log10(mean(np.abs(t) ** 2) / mean(np.abs(d) ** 2))

        irx, g1 = nearest(np.sqrt(Es) * r, raw)
        itx, g2 = nearest(np.sqrt(Es) * t, raw)
        margin = min(margin, g1, g2)
        errs = int(np.sum(popcount(irx ^ itx)))
        out["bit_errors"][k] = errs
        out["BER"][k] = errs / (n * B)
        out["SER"][k] = int(np.sum(irx != itx)) / n

        sigma2 = mean(np.abs(d - mean(d)) ** 2)
        gsum, msum = LD(0), LD(0)
        step = max(1, _CHUNK // M)
        for a in range(0, n, step):
            ra, ta, ia = r[a:a + step], t[a:a + step], itx[a:a + step]
            like = np.exp(-np.abs(ra[:, None] - norm[None, :]) ** 2 / sigma2) * pxa[None, :]
            for j in range(B):
                one = ((labels >> (B - 1 - j)) & 1).astype(bool)
                p0, p1 = np.sum(like[:, ~one], axis=1), np.sum(like[:, one], axis=1)
                min_sum = min(min_sum, float(np.min(p0)), float(np.min(p1)))
                with np.errstate(divide="ignore"):
                    llr = np.log(p0) - np.log(p1)
                clipped += int(np.sum(np.isinf(llr)))
                llr = np.where(llr == np.inf, 500.0, np.where(llr == -np.inf, -500.0, llr))
                sign = 2.0 * ((ia >> (B - 1 - j)) & 1) - 1.0
                gsum += np.sum(np.log2(1 + np.exp(sign * llr)).astype(LD))
            pY = np.sum(like, axis=1)
            term = -np.abs(ra - ta) ** 2 / sigma2 * np.log2(np.e) + np.log2(pxa[ia]) - np.log2(pY)
            msum += np.sum(term.astype(LD))
        out["GMI"][k] = float(H - gsum / n)
        out["NGMI"][k] = out["GMI"][k] / H
        out["MI"][k] = float(H + msum / n)

        s, v = r_all[:, k] / jr, t_all[:, k] / jt
        if rotate:
            s = mean(v / s) * s
        out["EVM"][k] = mean(np.abs(s - v) ** 2) / mean(np.abs(v) ** 2)
    out.update(margin=margin, clipped=clipped, min_sum=min_sum)
    return out


def restate_blind(rx, M, constType, discard=0):
    """Blind EVM per mode ('EVM') and the smallest decision margin against the single-precision table, rescaled to raw-table
    units ('margin')."""
    table, w32 = om._evm_tables(M, constType)
    raw = om._tables(M, constType)[0]
    r_all = as_columns(rx, discard)
    real = not np.iscomplexobj(r_all)
    table = _table(table, real)
    scale = float(np.abs(raw[0]) / np.abs(table[0]))
    s_all = r_all / np.sqrt(mean(np.abs(r_all.reshape(-1)) ** 2))
    evm, margin = np.zeros(r_all.shape[1]), np.inf
    for k in range(r_all.shape[1]):
        s = s_all[:, k]
        ind, gap = nearest(s, table)
        margin = min(margin, scale * gap)
        den = np.mean(w32[ind])                                         # float32 in, float32 pairwise mean out
        assert den.dtype == np.float32
        evm[k] = mean(np.abs(s - table[ind]) ** 2) / float(den)
    return dict(EVM=evm, margin=margin)


def decisions(symb, M, constType):
    """Hard decisions of a 1-D sequence as bits, most significant first, and the decision margin."""
    raw = om._tables(M, constType)[0]
    symb = as_columns(symb)[:, 0]
    idx, gap = nearest(symb, _table(raw, not np.iscomplexobj(symb)))
    B = int(M).bit_length() - 1
    return ((idx[:, None] >> np.arange(B - 1, -1, -1)) & 1).reshape(-1), gap


def pnorm(x):
    x = np.asarray(x)
    wide = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return wide / np.sqrt(mean(np.abs(wide.reshape(-1)) ** 2))


def signal_power(x):
    """Sum over the columns of their mean power."""
    x = np.asarray(x)
    wide = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    rows = wide.shape[0] if wide.ndim else 1
    return float(np.sum((np.abs(wide.reshape(-1)) ** 2).astype(LD)) / rows)
