"""Shared by the adaptive-equalizer tests: the fixtures tests/golden/eq/eq_*.npz (tools/gen_golden_eq.py), the bounds the test
files hold in common, the comparison of a result against recorded arrays and the conditions every fixture must meet."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eq")
CASES = sorted(os.path.basename(p)[len("eq_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "eq_*.npz")))
EXPECTED_CASES = ["cma_qpsk_1d", "cma_rde", "darde_rde", "ddlms_qam64_3modes", "default_prec", "nlms_ddlms", "nlms_even_taps",
                  "nlms_static"]
REL = 1e-9          # sigOut and H: rel-L2 and per element against max |ref| (cpr_cases.REL, the project's bound for
#                     double-precision receiver functions against reference fixtures); errSq: per element against max |ref|
DECIDING = ("dd-lms", "rde")


class Param:
    """Stand-in for the reference's parameters object: attributes only."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"eq_{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def param(g, **extra):
    """The fixture's parameter object; ``prec`` is set unless the case leaves it at the default."""
    cfg = g["cfg"]
    kw = dict(cfg["param"], **extra)
    if cfg["prec"] is not None:
        kw.setdefault("prec", np.dtype(cfg["prec"]).type)
    return Param(**kw)


def param128(g, **extra):
    """The parameter object of the run that produced the fixture's sigOut, H and errSq: prec = complex128 in every case
    (`default_prec` stores that run next to the complex64 one, on the same complex64 input)."""
    return param(g, **dict(extra, prec=np.complex128))


def rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def decision_gap(alg, L, sigOut, table, radii):
    """Smallest difference between the two nearest decision candidates over the outputs of every deciding stage."""
    y2 = np.asarray(sigOut).reshape(len(sigOut), -1)
    table, radii = np.asarray(table).astype(np.complex128), np.asarray(radii).real.astype(np.float64)
    gap, start = np.inf, 0
    for a, ln in zip(alg, L):
        y = y2[start:start + ln].reshape(-1)
        if a == "dd-lms":
            d = np.sort(np.abs(y[:, None] - table[None, :]), axis=1)
            gap = min(gap, float(np.min(d[:, 1] - d[:, 0])))
        elif a == "rde" and len(radii) > 1:
            d = np.sort(np.abs(radii[None, :] - np.abs(y)[:, None]), axis=1)
            gap = min(gap, float(np.min(d[:, 1] - d[:, 0])))
        start += ln
    return gap


def spike(nModes, nTaps):
    H0 = np.zeros((nModes ** 2, nTaps), dtype=np.complex128)
    for k in range(nModes):
        H0[k + k * nModes, nTaps // 2] = 1
    return H0


def check_conditions(g):
    """The fixture cannot make a test pass emptily (asserted by the generator, re-checked on the stored values)."""
    cfg = g["cfg"]
    modes, nTaps = cfg["modes"], cfg["param"].get("nTaps", 15)
    H = g["H"]
    assert H.shape == (modes ** 2, nTaps) and g["sigOut"].shape[0] == cfg["total"] and g["errSq"].shape == (modes, cfg["total"])
    if any(a in DECIDING for a in cfg["alg"]):
        gap = decision_gap(cfg["alg"], cfg["L"], g["sigOut"], g["table"], g["Rrde"])
        assert gap >= 1e-6 and abs(gap - float(g["gap"])) <= 1e-12, gap
    H0 = spike(modes, nTaps)
    assert np.linalg.norm(H - H0) / np.linalg.norm(H0) >= 0.1
    if modes > 1:
        off = [r for r in range(modes ** 2) if r % (modes + 1)]
        assert np.sum(np.abs(H[off]) ** 2) / np.sum(np.abs(H) ** 2) >= 0.01
    if cfg["name"] == "default_prec":
        assert g["sigIn"].dtype == np.complex64 and g["symbRef"].dtype == np.complex64 and g["sigOut64"].dtype == np.complex64
        assert abs(rel_l2(g["sigOut64"].astype(np.complex128), g["sigOut"]) - float(g["self_err"])) <= 1e-12
        assert 1e-8 < float(g["self_err"]) < 1e-5


def compare(got, want, label, bound=REL):
    """rel-L2 and the largest element error against max |ref|, both within ``bound``."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    e2, emax = rel_l2(got, want), float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{label}: rel-L2 {e2:.2e}, max element error / max |ref| {emax:.2e}")
    assert e2 <= bound and emax <= bound, (label, e2, emax)


def compare_results(sigOut, H, errSq, g, label, static_from=None):
    """A (sigOut, H, errSq) triple against the fixture's complex128 result.  errSq of a static stage is 0 here and
    uninitialised in the reference: from symbol ``static_from`` on it is held to 0 instead."""
    sigOut, H, errSq = np.asarray(sigOut), np.asarray(H), np.asarray(errSq)
    assert sigOut.dtype == np.complex128 and H.dtype == np.complex128 and errSq.dtype == np.float64, label
    compare(sigOut, g["sigOut"], f"{label} sigOut")
    compare(H, g["H"], f"{label} H")
    want = g["errSq"]
    if static_from is not None:
        assert np.all(errSq[:, static_from:] == 0), label
        errSq, want = errSq[:, :static_from], want[:, :static_from]
    e = float(np.max(np.abs(errSq - want)) / np.max(np.abs(want)))
    print(f"{label} errSq: max element error / max |ref| {e:.2e}")
    assert errSq.shape == want.shape and e <= REL, (label, e)


def static_start(g):
    """First symbol of the first static stage of a fixture, or None."""
    start = 0
    for a, ln in zip(g["cfg"]["alg"], g["cfg"]["L"]):
        if a == "static":
            return start
        start += ln
    return None


def write_emu_input(path, sigIn, param, symbRef):
    """The input file of tests/emu/emu_eq.cpp: the arguments as the package hands them to the library.  Returns what
    ``equalization._prepare`` made of them."""
    from opticommpy_amd import equalization as oeq
    q = oeq._prepare(sigIn, param, symbRef)
    p = q["params"]
    with open(path, "wb") as f:
        f.write(np.array([p.n, p.total, p.nref, p.nModes, p.nTaps, p.SpS, p.dtype, p.ref_dtype, p.nStages, p.numIter, p.M, p.nRadii],
                         dtype=np.int64).tobytes())
        f.write(np.array([p.Rcma], dtype=np.float64).tobytes())
        for st in q["stages"]:
            f.write(np.array([st.L, st.alg], dtype=np.int64).tobytes())
            f.write(np.array([st.mu], dtype=np.float64).tobytes())
        f.write(q["table"].tobytes())
        f.write(q["radii"].tobytes())
        f.write(q["H"].tobytes())
        f.write(np.ascontiguousarray(q["x"]).tobytes())
        if q["ref"] is not None:
            f.write(np.ascontiguousarray(q["ref"]).tobytes())
    return q
