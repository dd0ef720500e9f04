"""symbolSync, finddelay and decimate (optic/dsp/core.py:435-491, 552-698) restated line by line, with every correlation taken
directly in the time domain in ``np.longdouble`` -- no transform, so no transform's rounding.  Besides the reference's result it
returns the decisions taken and ``margin``, the smallest relative gap over all of them: a case whose margin is far above the
rounding of a double-precision transform (about 1e-13 at the sizes used) has one right answer, and the device must give it.

``decisions`` works from the list of correlations in the order the reference computes them, whatever computed them: the fixture
generator feeds it what the reference's own scipy calls returned."""
import types

import numpy as np

LD = np.longdouble
ROT = (1, -1, 1j, -1j)


DENSE_LIMIT = 1 << 27      # products a dense direct correlation may take
SPARSE_LIMIT = 1 << 23     # ... and a sparse one


def _constant_plus_sparse(a):
    """(c, indices, values) with a = c + sparse: c is the value most of a holds (its median), if any."""
    c = np.sort(a.real)[len(a) // 2] + (1j * np.sort(a.imag)[len(a) // 2] if a.dtype.kind == "c" else 0)
    c = a.dtype.type(c)
    idx = np.flatnonzero(a != c)
    return c, idx, a[idx] - c


def correlate(a, b):
    """scipy.signal.correlate(a, b, mode='full') for 1-D sequences, directly in the time domain, in extended precision:
    c[k] = sum_l a[l + k - (len(b) - 1)] conj(b[l]).  Long sequences qualify only as a constant plus a few other values; the
    sum is then taken term by term over the sparse parts and in closed form (prefix sums) over the constant ones."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "c" or b.dtype.kind == "c":
        a, b = a.astype(np.clongdouble), b.astype(np.clongdouble)
    else:
        a, b = a.astype(LD), b.astype(LD)
    na, nb = len(a), len(b)
    if na * nb <= DENSE_LIMIT:
        return np.correlate(a, b, mode="full")
    ca, ia, va = _constant_plus_sparse(a)
    cb, ib, vb = _constant_plus_sparse(np.conj(b))
    assert len(ia) * len(ib) <= SPARSE_LIMIT, "too long for a direct correlation and not sparse"
    out = np.zeros(na + nb - 1, dtype=a.dtype)
    np.add.at(out, (ia[:, None] - ib[None, :] + nb - 1).ravel(), (va[:, None] * vb[None, :]).ravel())
    # lag k pairs l in [l0, l1) of b with i = l + s of a, s = k - (nb - 1)
    s = np.arange(na + nb - 1) - (nb - 1)
    l0, l1 = np.maximum(0, -s), np.minimum(nb, na - s)
    sa, sb = np.zeros(na, dtype=a.dtype), np.zeros(nb, dtype=a.dtype)
    sa[ia], sb[ib] = va, vb
    pa = np.concatenate((np.zeros(1, dtype=a.dtype), np.cumsum(sa)))
    pb = np.concatenate((np.zeros(1, dtype=a.dtype), np.cumsum(sb)))
    return out + cb * (pa[l1 + s] - pa[l0 + s]) + ca * (pb[l1] - pb[l0]) + ca * cb * (l1 - l0)


def _argmax_gap(mag):
    """(index of the first maximum, (peak - runner-up) / peak)."""
    i = int(np.argmax(mag))
    if len(mag) < 2:
        return i, 1.0
    rest = np.delete(mag, i)
    peak = mag[i]
    return i, float((peak - np.max(rest)) / peak) if peak > 0 else 0.0


def decisions(mode, nModes, n_tx, corrs):
    """The reference's decisions from its correlations in call order (core.py:603-665).

    'amp': nModes^2 correlations in the order (n, m), then the nModes of finddelay.  'real': (crr, cir) per (n, m), then per
    column k finddelay's and cii.  Returns a namespace with delay, swap, rot (as applied), conj, corrMatrix and margin."""
    corrs = [np.asarray(c) for c in corrs]
    margin = np.inf
    corrMatrix = np.zeros((nModes, nModes))
    rotm = np.ones((nModes, nModes), dtype=np.complex64)
    it = iter(corrs)
    for n in range(nModes):
        for m in range(nModes):
            if mode == "amp":
                mag = np.abs(next(it))
                i, gap = _argmax_gap(mag)
                margin = min(margin, gap)
                corrMatrix[m, n] = float(mag[i])
            else:
                crr, cir = next(it), next(it)
                ir, gr = _argmax_gap(np.abs(crr))
                ii, gi = _argmax_gap(np.abs(cir))
                margin = min(margin, gr, gi)
                pr, pi = crr[ir], cir[ii]
                ar, ai = abs(pr), abs(pi)
                margin = min(margin, float(abs(ar - ai) / max(ar, ai)))
                corrMatrix[m, n] = float(max(ar, ai))
                if ar > ai:
                    rotm[m, n] = 1 if pr > 0 else -1
                else:
                    rotm[m, n] = -1j if pi > 0 else 1j
    swap = np.argmax(corrMatrix, axis=0)
    for n in range(nModes):
        if nModes > 1:
            col = np.sort(corrMatrix[:, n])
            margin = min(margin, float((col[-1] - col[-2]) / col[-1]))
    delay = np.zeros(nModes, dtype=np.int64)
    conj = np.zeros(nModes, dtype=bool)
    rot = np.ones(nModes, dtype=np.complex64)
    for k in range(nModes):
        mag = np.abs(next(it))
        i, gap = _argmax_gap(mag)
        margin = min(margin, gap)
        delay[k] = i - n_tx + 1
        if mode == "real":
            rot[k] = rotm[k, swap[k]]
            cii = next(it)
            j, gap = _argmax_gap(np.abs(cii))
            margin = min(margin, gap)
            conj[k] = cii[j] < 0
    assert next(it, None) is None
    return types.SimpleNamespace(delay=delay, swap=swap.astype(np.int64), rot=rot, conj=conj, corrMatrix=corrMatrix, margin=float(margin))


def decimate(sigIn, SpS):
    """core.py:435-491 with SpSout = 1, on a 2-D array."""
    sigIn = sigIn.copy()
    sampDelay = np.zeros(sigIn.shape[1])
    for k in range(sigIn.shape[1]):
        varVector = np.var(sigIn[:, k].reshape(-1, SpS), axis=0)
        sampDelay[k] = np.where(varVector == np.amax(varVector))[0][0]
    sigOut = sigIn[::SpS, :].copy()
    for k in range(sigIn.shape[1]):
        sigIn[:, k] = np.roll(sigIn[:, k], -int(sampDelay[k]))
        sigOut[:, k] = sigIn[0::SpS, k]
    return sigOut


def finddelay(x, y):
    c = np.abs(correlate(x, y))
    return int(np.argmax(c)) - len(x) + 1


def symbolSync(rx, tx, SpS, mode="amp"):
    """(tx aligned to rx, info): core.py:552-675; info as ``decisions`` returns it."""
    rx, tx = np.asarray(rx), np.asarray(tx)
    shape = tx.shape
    if rx.ndim == 1:
        rx = rx.reshape(len(rx), 1)
    if tx.ndim == 1:
        tx = tx.reshape(len(tx), 1)
    nModes = rx.shape[1]
    if SpS > 1:
        rx = decimate(rx, SpS)
    corrs = []

    def corr(a, b):
        corrs.append(correlate(a, b))
        return corrs[-1]

    if mode == "amp":
        for n in range(nModes):
            for m in range(nModes):
                abs_tx = np.abs(tx[:, m])
                abs_tx -= np.mean(abs_tx)
                abs_rx = np.abs(rx[:, n])
                abs_rx -= np.mean(abs_rx)
                corr(abs_tx, abs_rx)
        info = decisions(mode, nModes, len(tx), corrs + [np.ones(1)] * nModes)       # swap first: the delays need it
        tx = tx[:, info.swap]
        for k in range(nModes):
            abs_tx = np.abs(tx[:, k])
            abs_tx -= np.mean(abs_tx)
            abs_rx = np.abs(rx[:, k])
            abs_rx -= np.mean(abs_rx)
            corr(abs_tx, abs_rx)
    elif mode == "real":
        for n in range(nModes):
            for m in range(nModes):
                corr(np.real(tx[:, m]), np.real(rx[:, n]))
                corr(np.imag(tx[:, m]), np.real(rx[:, n]))
        info = decisions(mode, nModes, len(tx), corrs + [np.ones(1)] * (2 * nModes))
        tx = tx[:, info.swap]
        for k in range(nModes):
            tx[:, k] = info.rot[k] * tx[:, k]
            corr(np.real(tx[:, k]), np.real(rx[:, k]))
            corr(np.imag(tx[:, k]), np.imag(rx[:, k]))
    else:
        raise ValueError(mode)
    info = decisions(mode, nModes, len(tx), corrs)
    for k in range(nModes):
        if info.conj[k]:
            tx[:, k] = tx[:, k].conj()
    for k in range(nModes):
        tx[:, k] = np.roll(tx[:, k], -int(info.delay[k]))
    return tx.reshape(shape), info
