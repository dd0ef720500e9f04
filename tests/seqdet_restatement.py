"""Extended-precision numpy restatement of mlse, detector, autocorr and levinson (optic/comm/modulation.py:412-481, 582-680;
optic/dsp/core.py:1143-1227), vectorised over the trellis states.  tools/gen_golden_seqdet.py holds it to the reference's own
output on every fixture; the tests then hold the kernels to it on shapes the fixtures do not reach.

mlse: state s holds the last L symbols, the newest in the lowest digit.  Next state ns is reached from ns // M + j M^(L-1),
j = 0 .. M-1, with the symbol ns % M (L = 0: the one state's candidates are the M symbols).  The first minimum over j is the
reference's survivor: it walks the predecessors upwards with a strict <."""
import numpy as np


def _wide(a, ext):
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return a.astype(np.clongdouble if ext is np.longdouble else np.complex128)
    return a.astype(ext)


def expected_outputs(h, c, ext=np.longdouble):
    """yExpected[s, k] in the reference's summation order, and the number of states."""
    h, c = _wide(h, ext), _wide(c, ext)
    M, L = len(c), len(h) - 1
    S = M ** L if L > 0 else 1
    s = np.arange(S)
    out = np.empty((S, M), dtype=np.result_type(h.dtype, c.dtype))
    for k in range(M):
        acc = np.full(S, h[0] * c[k], dtype=out.dtype)
        rest = s.copy()
        for i in range(1, L + 1):
            acc = acc + h[i] * c[rest % M]
            rest //= M
        out[:, k] = acc
    return out, S


def mlse(y, h, c, ext=np.longdouble):
    """dict(index: the decided points' indices, seq: the points, metric: final minimum, final_state, gap: smallest non-zero
    (second - best) / (1 + best) over every step and state, final_gap: the same between the two lowest final metrics, ties: the
    number of (step, state) pairs whose two best candidates are exactly equal)."""
    y = _wide(y, ext)
    yexp, S = expected_outputs(h, c, ext)
    M, L, N = len(c), len(h) - 1, len(y)
    ns = np.arange(S)
    if L == 0:
        pred = np.zeros((1, M), dtype=np.int64)
        sym = np.arange(M)[None, :]
    else:
        pred = (ns // M)[:, None] + np.arange(M)[None, :] * (S // M)
        sym = np.broadcast_to((ns % M)[:, None], (S, M))
    ye = yexp[pred, sym]                                  # the expected output of candidate j of next state ns
    pm = np.zeros(S, dtype=ext)
    surv = np.empty((N, S), dtype=np.int64)
    gap, ties = np.inf, 0
    for n in range(N):
        d = y[n] - ye
        bm = d.real * d.real + d.imag * d.imag if np.iscomplexobj(d) else d * d
        cand = pm[pred] + bm
        j = np.argmin(cand, axis=1)
        best = cand[ns, j]
        if M > 1:
            two = np.sort(cand, axis=1)[:, :2]
            diff = two[:, 1] - two[:, 0]
            ties += int(np.sum(diff == 0))
            nz = diff > 0
            if np.any(nz):
                gap = min(gap, float(np.min(diff[nz] / (1 + two[nz, 0]))))
        surv[n], pm = j, best
    state = int(np.argmin(pm))
    srt = np.sort(pm)
    final_gap = float((srt[1] - srt[0]) / (1 + srt[0])) if S > 1 else np.inf
    final_state, metric = state, pm[state]
    index = np.empty(N, dtype=np.int64)
    for n in range(N - 1, -1, -1):
        j = int(surv[n, state])
        index[n] = j if L == 0 else state % M
        state = 0 if L == 0 else state // M + j * (S // M)
    return dict(index=index, seq=np.asarray(c)[index], metric=metric, final_state=final_state, gap=gap, final_gap=final_gap, ties=ties,
                states=S)


def detector(r, sigma2, c, px=None, rule="MAP", ext=np.longdouble):
    """(indices, smallest distance between the best and the second-best metric over all symbols)."""
    r, c = _wide(np.asarray(r).reshape(-1), ext), _wide(c, ext)
    d = r[:, None] - c[None, :]
    d2 = d.real * d.real + d.imag * d.imag if np.iscomplexobj(d) else d * d
    if rule == "ML":
        v = -d2
    else:
        px = np.full(len(c), 1 / len(c)) if px is None else np.asarray(px, dtype=np.float64)
        with np.errstate(divide="ignore"):
            v = -d2 / ext(sigma2) + np.log(px).astype(ext)[None, :]
    ind = np.argmax(v, axis=1)
    gap = np.inf
    if len(c) > 1:
        two = np.sort(v, axis=1)[:, -2:]
        gap = float(np.min(two[:, 1] - two[:, 0]))
    return ind.astype(np.int64), gap


def autocorr(x, nTaps, ext=np.longdouble):
    x = np.asarray(x).astype(ext)
    N = len(x)
    return np.array([np.sum(x[k:] * x[:N - k]) / (N - k) for k in range(nTaps)], dtype=ext)


def levinson(r, nTaps, ext=np.longdouble):
    """(a, reflection coefficients)."""
    r = np.asarray(r).astype(ext)
    a = np.zeros(nTaps, dtype=ext)
    a[0] = 1
    e, ks = r[0], []
    for i in range(1, nTaps):
        k = -(r[i] + np.sum(a[1:i] * r[i - 1:0:-1][:i - 1])) / e
        nxt = a.copy()
        nxt[1:i] += k * a[i - 1:0:-1][:i - 1]
        nxt[i] = k
        a = nxt
        e = e * (1 - k * k)
        ks.append(k)
    return a, np.array(ks, dtype=ext)
