"""The adaptive MIMO equalizer restated in plain numpy, one symbol at a time and decoupled per output mode: output mode k owns the
rows k + N nModes of H, and nothing another mode computes enters them.  It shares no code with the package beyond the host-side
argument handling (``equalization._prepare``: stage list, float32-rounded step sizes, constellation, radii, initial H), which
tests/test_eq_host.py pins to the fixtures; tests/test_eq_restatement.py pins the restatement itself to every fixture.  Used for
the geometries no fixture covers (tests/test_gpu_eq_shapes.py)."""
import numpy as np

from opticommpy_amd import equalization as oeq


def restate(sigIn, param=None, symbRef=None):
    """(sigOut, H, errSq, gap): complex128 (total, nModes) (1-D for a 1-D input), complex128 (nModes^2, nTaps), float64
    (nModes, total), and the smallest difference between the two nearest decision candidates any deciding update saw."""
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
    start = 0
    for s, (alg, L, mu) in enumerate(zip(q["alg"], q["L"], q["mu"])):
        for k in range(nModes):
            rows = [k + N * nModes for N in range(nModes)]
            h = H[rows].copy()                                   # (input mode, tap)
            for _ in range(prm.numIter if s == 0 else 1):
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
                            r2 = radii[np.argmin(d)] ** 2
                        e = r2 - np.abs(y) ** 2
                        h += mu * e * y * np.conj(w)
                    errSq[k, i] = np.abs(e) ** 2
            H[rows] = h
        start += L
    if q["input1D"]:
        sigOut = sigOut.reshape(total)
    return sigOut, H, errSq, float(gap)
