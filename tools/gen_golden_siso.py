#!/usr/bin/env python3
"""Generate the ffe / dfe / volterra fixtures tests/golden/siso/siso_*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_eq.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity), and one
for ``tqdm.notebook`` if that is missing: the cores are then plain Python loops, 0.1 - 0.2 s for 1500 symbols.  No bytecode is written.

Each file holds
    sigIn, symbRef   the input at SpS samples per symbol and the transmitted symbols, as handed to the equalizer
    sigOut, mse      what the reference returns with prec = float64 / complex128 (mse: the real part)
    c0, c1, c2       the final coefficients: f | f, b | h1, h2, h3;  i0, i1, i2 the initial ones where the case gives them
    table            the decision table as the reference computes it in the case's ``prec``
    gap              smallest distance between the two nearest table points over the decided symbols of every pass (read off
                     tests/siso_restatement.py, which is held to the reference's sigOut at 1e-9 first)
    change           ||f - f0|| (f0 the initial linear part), and norm_b, norm_h2, norm_h3 where they exist
    cfg              JSON: kind, the parameters set on the parameter object, seed, numpy version, ...
and, for `*_default_prec` (prec left unset, sigIn and symbRef stored in single precision): sigOut32, mse32, c0_32 .., the
reference's single-precision result on that input, and self_err, the rel-L2 distance between its two results (sigOut, mse and
c0 .. are the double run's: prec = float64 on the stored input widened to double).

Synthetic input: unit-power PAM-4 / PAM-8 with the DC removed, held for SpS samples and smoothed, a short ISI filter plus a small
x^2 term, white noise at 26 dB for the real cases; 16-QAM with ISI and a fixed rotation for the complex ones.

Conditions asserted here, re-asserted by tests/siso_cases.py:check_conditions, so that no fixture lets a test pass emptily:
gap >= 1e-6; change >= 0.1; norm_b >= 0.03; norm_h2 >= 0.1; norm_h3 >= 0.02 at order 3.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_siso.py [case ...]
"""
import importlib.util
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
if importlib.util.find_spec("tqdm") is None:
    _tq = types.ModuleType("tqdm")
    _tq.tqdm = lambda it, **k: it
    _tqn = types.ModuleType("tqdm.notebook")
    _tqn.tqdm = _tq.tqdm
    _tq.notebook = _tqn
    sys.modules["tqdm"] = _tq
    sys.modules["tqdm.notebook"] = _tqn
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "reference")))

import numpy as np  # noqa: E402

import optic.dsp.equalization as ref_eq  # noqa: E402
from optic.comm.modulation import grayMapping as ref_gray  # noqa: E402

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[1:1] = [_ROOT, os.path.join(_ROOT, "tests")]
from siso_restatement import restate  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "siso")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py
SNR_DB = 26

_F = dict(nTaps=9, SpS=2, mu=8e-3, nTrain=900, M=4, constType="pam")
_D = dict(nTapsFF=9, nTapsFB=4, SpS=2, mu=8e-3, nTrain=900, M=4, constType="pam")
_V = dict(n1Taps=9, n2Taps=5, n3Taps=3, SpS=2, mu=2e-2, nTrain=900, M=4, constType="pam")
_Q = dict(M=16, constType="qam", mu=6e-3)
# name: kind, symbols, param (what is set on the parameter object), prec ("real" / "complex" double, None: left unset), init
CASES = {
    "ffe_real": dict(kind="ffe", nsym=1500, param=_F),
    "ffe_fulltime": dict(kind="ffe", nsym=1500, param=dict(_F, trainingMode="fulltime", nTrain=500)),
    "ffe_preconv3": dict(kind="ffe", nsym=1300, param=dict(_F, preconvIters=3, nTrain=400, M=8, mu=5e-3)),
    "ffe_qam": dict(kind="ffe", nsym=1500, param=dict(_F, **_Q)),
    "dfe_real": dict(kind="dfe", nsym=1500, param=_D),
    "dfe_fulltime": dict(kind="dfe", nsym=1500, param=dict(_D, trainingMode="fulltime", nTrain=500)),
    "dfe_preconv3": dict(kind="dfe", nsym=1300, param=dict(_D, preconvIters=3, nTrain=400)),
    "dfe_qam": dict(kind="dfe", nsym=1500, param=dict(_D, **_Q)),
    "volterra_order2": dict(kind="volterra", nsym=1500, param=dict(_V, order=2)),
    "volterra_order3": dict(kind="volterra", nsym=1500, param=dict(_V, order=3)),
    "volterra_order3_fulltime": dict(kind="volterra", nsym=1200, param=dict(_V, order=3, trainingMode="fulltime", nTrain=500)),
    "volterra_preconv2": dict(kind="volterra", nsym=1200, param=dict(_V, order=3, preconvIters=2, nTrain=500)),
    "ffe_even_taps_sps3": dict(kind="ffe", nsym=1200, param=dict(_F, nTaps=8, SpS=3)),
    "dfe_given_coefficients": dict(kind="dfe", nsym=1200, param=_D, init=True),
    "volterra_train_all": dict(kind="volterra", nsym=1200, param=dict(_V, order=3, nTrain=1300, preconvIters=2)),
    "ffe_default_prec": dict(kind="ffe", nsym=1500, param=_F, prec=None),
    "dfe_default_prec": dict(kind="dfe", nsym=1500, param=_D, prec=None),
    "volterra_default_prec": dict(kind="volterra", nsym=1500, param=dict(_V, order=3), prec=None),
}


class Param:
    pass


def make_param(d, prec, init):
    p = Param()
    for k, v in d.items():
        setattr(p, k, v)
    if prec is not None:
        p.prec = prec
    for k, v in (init or {}).items():
        setattr(p, k, [a.copy() for a in v] if isinstance(v, list) else v.copy())      # (the reference updates them in place)
    return p


def make_signal(case, seed):
    prm = case["param"]
    rng = np.random.default_rng(seed)
    nsym, SpS, M, cx = case["nsym"], prm["SpS"], prm["M"], prm["constType"] == "qam"
    table = ref_gray(M, prm["constType"]).astype(np.complex128 if cx else np.float64)
    table = table / np.sqrt(np.mean(np.abs(table) ** 2))
    tx = table[rng.integers(0, M, size=nsym)]
    up = np.repeat(tx, SpS)
    if SpS > 1:
        up = np.convolve(up, [0.2, 0.6, 0.2], mode="same")
    isi = np.array([0.08 - 0.05j, 1.0, 0.22 + 0.12j, -0.06j]) if cx else np.array([0.1, 1.0, 0.3, -0.08])
    taps = np.zeros((len(isi) - 1) * SpS + 1, dtype=isi.dtype)
    taps[::SpS] = isi
    x = np.convolve(up, taps, mode="full")[SpS:SpS + len(up)]
    if cx:
        x = x * np.exp(0.3j) * 0.7
        sigma2 = np.mean(np.abs(x) ** 2) * 10 ** (-SNR_DB / 10)
        x = x + (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape)) * np.sqrt(sigma2 / 2)
    else:
        x = x + 0.08 * x ** 2
        x = (x - np.mean(x)) * 0.7
        x = x + rng.normal(size=x.shape) * np.sqrt(np.mean(x ** 2) * 10 ** (-SNR_DB / 10))
    return x, tx


def initial(case, seed):
    """Non-trivial initial coefficients (not symmetric, nothing zero) for the case that gives them."""
    if not case.get("init"):
        return None
    rng = np.random.default_rng(seed + 1000)
    prm = case["param"]
    f = 0.02 * rng.normal(size=prm["nTapsFF"])
    f[prm["nTapsFF"] // 2] += 0.9
    return dict(f=f, b=0.02 * rng.normal(size=prm["nTapsFB"]))


def run_reference(case, x, tx, prec, init):
    keep_x, keep_t = x.copy(), tx.copy()
    res = getattr(ref_eq, case["kind"])(x, tx, make_param(case["param"], prec, init))
    assert np.array_equal(x, keep_x) and np.array_equal(tx, keep_t)
    if case["kind"] == "ffe":
        return res[0], [res[1]], res[2]
    if case["kind"] == "dfe":
        return res[0], [res[1], res[2]], res[3]
    return res[0], list(res[1]), res[2]


def measures(case, coef, init):
    prm, kind = case["param"], case["kind"]
    n1 = prm.get("nTaps", prm.get("nTapsFF", prm.get("n1Taps")))
    f0 = np.zeros(n1)
    f0[n1 // 2] = 1
    if init:
        f0 = init["f"]
    v = dict(change=float(np.linalg.norm(coef[0] - f0)))
    if kind == "dfe":
        v["norm_b"] = float(np.linalg.norm(coef[1]))
    if kind == "volterra":
        v["norm_h2"] = float(np.linalg.norm(coef[1]))
        if prm["order"] == 3:
            v["norm_h3"] = float(np.linalg.norm(coef[2]))
    return v


def acceptable(v):
    return (v["gap"] >= 1e-6 and v["change"] >= 0.1 and v.get("norm_b", 1) >= 0.03 and v.get("norm_h2", 1) >= 0.1
            and v.get("norm_h3", 1) >= 0.02)


def generate(name):
    case = CASES[name]
    prm, kind = case["param"], case["kind"]
    cx = prm["constType"] == "qam"
    single = "prec" in case and case["prec"] is None
    wide = np.complex128 if cx else np.float64
    narrow = np.complex64 if cx else np.float32
    N = case["nsym"]
    first = 5000 + 10 * sorted(CASES).index(name)
    for seed in range(first, first + 50):
        x, tx = make_signal(case, seed)
        if single:
            x, tx = x.astype(narrow), tx.astype(narrow)
        init = initial(case, seed)
        sigOut, coef, mse = run_reference(case, x.astype(wide), tx.astype(wide), wide, init)
        table = ref_eq.pnorm(ref_gray(prm["M"], prm["constType"]).astype(wide))
        v = measures(case, coef, init)
        # the decisions are taken inside the walk (volterra's are on the output before its final scaling): the restatement
        # (tests/siso_restatement.py), held to the reference's result here, gives the smallest gap over every decided symbol
        rs = restate(kind, x.astype(wide), tx.astype(wide), make_param(prm, wide, init))
        assert np.linalg.norm(rs["sigOut"] - sigOut) <= 1e-9 * np.linalg.norm(sigOut), name
        v["gap"] = float(rs["gap"])
        if acceptable(v):
            break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 50}) meets the conditions: {v}")
    assert sigOut.dtype == wide and sigOut.shape == (N,) and all(c.dtype == wide for c in coef)
    out = dict(sigIn=x, symbRef=tx, sigOut=sigOut, mse=np.ascontiguousarray(np.asarray(mse).real.astype(np.float64)), table=table, **v)
    for i, c in enumerate(coef):
        out[f"c{i}"] = c
    if init:
        out.update(i0=init["f"], i1=init["b"])
    if single:
        s32, c32, m32 = run_reference(case, x, tx, None, init)
        assert s32.dtype == narrow and all(c.dtype == narrow for c in c32)
        out.update(sigOut32=s32, mse32=np.ascontiguousarray(np.asarray(m32).real),
                   self_err=float(np.linalg.norm(s32.astype(wide) - sigOut) / np.linalg.norm(sigOut)))
        for i, c in enumerate(c32):
            out[f"c{i}_32"] = c
    cfg = dict(name=name, kind=kind, param=prm, single=single, complex=cx, n=int(len(x)), N=N, dtype=x.dtype.name, snr_dB=SNR_DB, seed=seed,
               numpy=np.__version__, init=bool(init))
    out["cfg"] = json.dumps(cfg)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"siso_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size >> 10} KiB  seed {seed}  " + "  ".join(f"{k} {val:.3g}" for k, val in v.items())
          + (f"  self_err {out['self_err']:.2e}" if single else ""), flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        generate(case)
