#!/usr/bin/env python3
"""Generate the perturbation-model fixtures tests/golden/nlin/*.npz by IMPORTING THE REFERENCE's optic/models/perturbation.py.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_eq.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity,
``prange`` = ``range``): ``calcNLINperturbation`` and ``calcNLINperturbationSimplified`` are then the plain Python loops, seconds
per call at these sizes (a minute at matrixOrder 75).  The reference needs scipy (``quad``, ``exp1``); the package does not.

``<case>.npz``:
    Ein                      (N, 2) input as handed to perturbationNLIN (a copy: the reference overwrites its argument)
    C_ifwm, C_ixpm, C_ispm   the reference's calcPertCoeffMatrix(param) (C is their sum with C_ispm at the centre)
    nlin128, nlin64          the reference's perturbationNLIN(Ein.copy(), param) with param.prec complex128 / complex64
    x, y                     what that call handed to calcNLINperturbation[Simplified]: the columns after pnorm
    dx128, dy128, phx128, phy128, dx64, dy64, phx64, phy64     what it got back, per prec
    nReducedCoeffs, reductionFactor     'AMR' only
    dist_nlin64, dist_d64, dist_phi64   max |.64 - .128| / max |.128| of nlin, of (dx, dy) and of the phases
    cfg                      JSON: every parameter value, N, seed, numpy and scipy versions
A case with ``ein64`` also holds ``nlin128_e64``: perturbationNLIN(Ein.astype(complex64), prec complex128) and its distance
``dist_e64`` to nlin128.

Conditions asserted here and re-asserted by tests/nlin_cases.py:check_conditions: max |C| (with C_ispm in the corner, as the
calculation forms it) is attained once; no coefficient lies within 1e-9 (relative) of the 'AMR' threshold.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_nlin.py [case ...]
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True

_nb = types.ModuleType("numba")


def _identity_decorator(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f


_nb.njit = _nb.jit = _identity_decorator
_nb.prange = range
_nb_typed = types.ModuleType("numba.typed")
_nb_typed.List = list
_nb.typed = _nb_typed
sys.modules["numba"] = _nb
sys.modules["numba.typed"] = _nb_typed
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(HERE, "..", "..", "reference")))

import numpy as np  # noqa: E402
import scipy  # noqa: E402

import optic.models.perturbation as ref  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "nlin")
MAX_BYTES = 400 * 1024

# param: what is set on the parameter object (everything else is the reference's default)
CASES = {
    "am_l3": dict(N=64, M=16, seed=1, param=dict(mode="AM", matrixOrder=3)),
    "am_default": dict(N=512, M=16, seed=2, param=dict(mode="AM")),
    "amr_default": dict(N=512, M=16, seed=2, param=dict(mode="AMR", coeffTol=-20)),
    # examples/test_perturbation_models.ipynb
    "nb_amr": dict(N=256, M=16, seed=3, param=dict(mode="AMR", coeffTol=-30, matrixOrder=75, length=1600, lspan=80, Pin=2)),
    "tiny": dict(N=5, M=4, seed=4, param=dict(mode="AM", matrixOrder=4)),
    "noisy": dict(N=200, M=16, seed=5, snr_dB=18, param=dict(mode="AM", matrixOrder=10, Pin=3, alpha=0.25, gamma=1.6, D=16, pulseWidth=0.4)),
    "amr_all": dict(N=100, M=16, seed=6, param=dict(mode="AMR", coeffTol=-400, matrixOrder=5)),
    "amr_corner": dict(N=100, M=16, seed=7, param=dict(mode="AMR", coeffTol=-0.1, matrixOrder=5)),
    "ein64": dict(N=128, M=16, seed=8, ein64=True, param=dict(mode="AM", matrixOrder=6, Pin=1)),
}


class Param:
    pass


def make_param(d, prec):
    p = Param()
    for k, v in d.items():
        setattr(p, k, v)
    p.prec = prec
    return p


def qam(rng, n, M):
    side = int(round(np.sqrt(M)))
    lv = np.arange(-(side - 1), side, 2)
    return (rng.choice(lv, n) + 1j * rng.choice(lv, n)).astype(np.complex128)


def conditions(C_ifwm, C_ixpm, C_ispm, coeffTol):
    D = C_ifwm.shape[0] - 1
    C = C_ifwm + C_ixpm
    C[D, D] = C_ispm
    a = np.abs(C.flatten())
    assert np.sum(a == a.max()) == 1, "max |C| is attained more than once"
    if coeffTol is not None:
        thr = a.max() * 10 ** (coeffTol / 20)
        nz = a[a > 0]
        assert np.min(np.abs(nz / thr - 1)) > 1e-9 if thr > 0 else True, "a coefficient sits on the threshold"


def run(Ein, d, prec):
    """perturbationNLIN of the reference, with what it hands to and gets from its calculation recorded."""
    rec = {}
    names = ("calcNLINperturbation", "calcNLINperturbationSimplified")
    orig = {k: getattr(ref, k) for k in names}

    def wrap(f):
        def g(C_ifwm, C_ixpm, C_ispm, x, y, *a):
            rec["x"], rec["y"] = np.array(x), np.array(y)
            out = f(C_ifwm, C_ixpm, C_ispm, x, y, *a)
            rec["out"] = out
            return out
        return g
    for k in names:
        setattr(ref, k, wrap(orig[k]))
    try:
        nlin = ref.perturbationNLIN(Ein.copy(), make_param(d, prec))
    finally:
        for k in names:
            setattr(ref, k, orig[k])
    return nlin, rec


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=complex) - np.asarray(b, dtype=complex))) / np.max(np.abs(b)))


def generate(name):
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    N = c["N"]
    Ein = np.stack([qam(rng, N, c["M"]), qam(rng, N, c["M"])], axis=1)
    if "snr_dB" in c:
        sigma = np.sqrt(np.mean(np.abs(Ein) ** 2) * 10 ** (-c["snr_dB"] / 10) / 2)
        Ein = Ein + sigma * (rng.standard_normal(Ein.shape) + 1j * rng.standard_normal(Ein.shape))
    d = c["param"]
    full = make_param(d, np.complex128)
    full.Fc = getattr(full, "Fc", 193.1e12)                  # perturbationNLIN's default, not calcPertCoeffMatrix's
    C, C_ifwm, C_ixpm, C_ispm = ref.calcPertCoeffMatrix(full)
    conditions(C_ifwm, C_ixpm, C_ispm, d.get("coeffTol", -20) if d["mode"] == "AMR" else None)
    out = dict(Ein=Ein, C_ifwm=C_ifwm, C_ixpm=C_ixpm, C_ispm=np.complex128(C_ispm))
    for tag, prec in (("128", np.complex128), ("64", np.complex64)):
        nlin, rec = run(Ein, d, prec)
        assert nlin.dtype == np.complex128
        out["nlin" + tag] = nlin
        o = rec["out"]
        assert o[0].dtype == prec and o[2].dtype == np.float64
        out["dx" + tag], out["dy" + tag], out["phx" + tag], out["phy" + tag] = o[:4]
        if tag == "128":
            out["x"], out["y"] = rec["x"], rec["y"]
            if d["mode"] == "AMR":
                out["nReducedCoeffs"], out["reductionFactor"] = np.int64(o[4]), np.float64(o[5])
    out["dist_nlin64"] = np.float64(rel(out["nlin64"], out["nlin128"]))
    out["dist_d64"] = np.float64(max(rel(out["dx64"], out["dx128"]), rel(out["dy64"], out["dy128"])))
    out["dist_phi64"] = np.float64(max(rel(out["phx64"], out["phx128"]), rel(out["phy64"], out["phy128"])))
    if c.get("ein64"):
        nlin, _ = run(Ein.astype(np.complex64), d, np.complex128)
        assert nlin.dtype == np.complex64
        out["nlin128_e64"] = nlin
        out["dist_e64"] = np.float64(rel(nlin, out["nlin128"]))
    cfg = dict(name=name, N=N, M=c["M"], seed=c["seed"], snr_dB=c.get("snr_dB"), param=d, numpy=np.__version__, scipy=scipy.__version__)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, cfg=json.dumps(cfg), **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes, dist_nlin64 {out['dist_nlin64']:.2e}, dist_d64 {out['dist_d64']:.2e}, dist_phi64 {out['dist_phi64']:.2e}"
          + (f", kept {int(out['nReducedCoeffs'])}" if "nReducedCoeffs" in out else ""), flush=True)


if __name__ == "__main__":
    for n in (sys.argv[1:] or CASES):
        generate(n)
