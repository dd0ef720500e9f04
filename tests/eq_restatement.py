"""The adaptive MIMO equalizer restated in plain numpy, one symbol at a time and decoupled per output mode: output mode k owns the
rows k + N nModes of H, and nothing another mode computes enters them.  It shares no code with the package beyond the host-side
argument handling (``equalization._prepare``: stage list, float32-rounded step sizes, constellation, radii, initial H), which
tests/test_eq_host.py pins to the fixtures; tests/test_eq_restatement.py pins the restatement itself to every fixture.  Used for
the geometries no fixture covers (tests/test_gpu_eq_shapes.py, tests/eq_shape_cases.py).

Radius clusters.  ``np.unique(np.abs(constSymb))`` keeps radii that differ only by rounding: 34 values for 256-QAM, which has 32
distinct radii, 123 for 1024-QAM in 109 clusters one ulp wide, and for PSK several "radii" of the unit circle (9, 17 and 129 for
64-, 128- and 1024-PSK, within 7e-8 in all; DESIGN.md 3.14 has the figures).  Distinct QAM radii are at least 3.7e-3 apart.
A cluster is a run of neighbouring values of the sorted radii that lie within CLUSTER = 1e-9 of one another.  Which member of a
cluster an 'rde' decision takes hangs on
the last bit of |y|, so with ``detail=True`` the gap of a radius decision is also measured between clusters, and the decisions
that fall inside one cluster are counted: a pick inside a cluster changes r2 by at most 2 R width."""
import numpy as np

from opticommpy_amd import equalization as oeq


CLUSTER = 1e-9
DECISION = np.dtype([("stage", np.int64), ("rep", np.int64), ("mode", np.int64), ("symbol", np.int64), ("winner", np.int64),
                     ("gap", np.float64), ("cgap", np.float64), ("same", np.bool_)])


def radius_clusters(radii):
    """(cluster number of every sorted radius, largest width of a cluster)."""
    radii = np.asarray(radii, dtype=np.float64)
    cl = np.concatenate(([0], np.cumsum(np.diff(radii) > CLUSTER)))
    width = max(float(radii[cl == c].max() - radii[cl == c].min()) for c in range(cl[-1] + 1))
    return cl, width


def restate(sigIn, param=None, symbRef=None, detail=False):
    """(sigOut, H, errSq, gap): complex128 (total, nModes) (1-D for a 1-D input), complex128 (nModes^2, nTaps), float64
    (nModes, total), and the smallest difference between the two nearest decision candidates any deciding update saw.

    With ``detail`` a fifth value, a dict: ``decisions``, one DECISION record per deciding update in the order they were made
    (``gap`` between the two nearest candidates; ``cgap`` for 'rde' between the nearest radius and the nearest radius of another
    cluster, inf where there is one cluster, and equal to ``gap`` for 'dd-lms'; ``same``: the two nearest radii lie in one
    cluster); ``close``, the records with ``gap`` < 1e-9; ``cluster_gap``, the smallest ``cgap`` of an 'rde' update;
    ``in_cluster``, the number of records with ``same``; ``width``, the largest width of a radius cluster; ``ymax``."""
    q = oeq._prepare(sigIn, param, symbRef)
    x = np.asarray(q["x"]).astype(np.complex128)
    ref = None if q["ref"] is None else np.asarray(q["ref"]).astype(np.complex128)
    prm = q["params"]
    nModes, nTaps, SpS, total = prm.nModes, prm.nTaps, prm.SpS, q["total"]
    Lpad = nTaps // 2
    pad = np.zeros((Lpad, nModes), dtype=np.complex128)
    xp = np.concatenate((pad, x, pad))
    table = q["table"].view(np.complex128)
    radii, Rcma = q["radii"], prm.Rcma
    H = q["H"].copy()
    sigOut = np.zeros((total, nModes), dtype=np.complex128)
    errSq = np.zeros((nModes, total))
    gap = np.inf
    cl, width = radius_clusters(radii)
    dec = []
    start = 0
    for s, (alg, L, mu) in enumerate(zip(q["alg"], q["L"], q["mu"])):
        for k in range(nModes):
            rows = [k + N * nModes for N in range(nModes)]
            h = H[rows].copy()                                   # (input mode, tap)
            for rep in range(prm.numIter if s == 0 else 1):
                for i in range(start, start + L):
                    w = xp[i * SpS:i * SpS + nTaps].T            # (input mode, tap)
                    y = np.sum(h * w)
                    sigOut[i, k] = y
                    if alg == "static":
                        continue
                    if alg == "nlms":
                        e = ref[i, k] - y
                        h += mu * e * np.conj(w) / (np.linalg.norm(w, axis=1) ** 2)[:, None]
                    elif alg == "dd-lms":
                        d = np.abs(y - table)
                        two = np.partition(d, 1)[:2]
                        gap = min(gap, two[1] - two[0])
                        if detail:
                            dec.append((s, rep, k, i, np.argmin(d), two[1] - two[0], two[1] - two[0], False))
                        e = table[np.argmin(d)] - y
                        h += mu * e * np.conj(w)
                    else:
                        if alg == "cma":
                            r2 = Rcma
                        elif alg == "da-rde":
                            r2 = np.abs(ref[i, k]) ** 2
                        else:
                            d = np.abs(radii - np.abs(y))
                            if len(d) > 1:
                                two = np.partition(d, 1)[:2]
                                gap = min(gap, two[1] - two[0])
                            if detail:
                                o = np.argsort(d, kind="stable")
                                other = d[cl != cl[o[0]]]
                                dec.append((s, rep, k, i, o[0], d[o[1]] - d[o[0]] if len(d) > 1 else np.inf,
                                            other.min() - d[o[0]] if other.size else np.inf, len(d) > 1 and cl[o[0]] == cl[o[1]]))
                            r2 = radii[np.argmin(d)] ** 2
                        e = r2 - np.abs(y) ** 2
                        h += mu * e * y * np.conj(w)
                    errSq[k, i] = np.abs(e) ** 2
            H[rows] = h
        start += L
    if q["input1D"]:
        sigOut = sigOut.reshape(total)
    if not detail:
        return sigOut, H, errSq, float(gap)
    dec = np.array(dec, dtype=DECISION)
    rde = np.array([q["alg"][r] == "rde" for r in dec["stage"]], dtype=bool)
    info = dict(decisions=dec, close=dec[dec["gap"] < CLUSTER], cluster_gap=float(np.min(dec["cgap"][rde], initial=np.inf)),
                in_cluster=int(np.count_nonzero(dec["same"])), width=width, ymax=float(np.max(np.abs(sigOut))))
    return sigOut, H, errSq, float(gap), info
