#!/usr/bin/env python3
"""Generate the adaptive-equalizer fixtures tests/golden/eq/eq_*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_cpr.py does, it
registers a throw-away ``numba`` stub first (``njit`` = identity), and one for ``tqdm.notebook`` if that is missing:
``coreAdaptEq`` is then the plain Python loop, well under a second for 1500 symbols.  No bytecode is written.

Each file holds
    sigIn, symbRef   the input at SpS samples per symbol and the transmitted symbols, as handed to mimoAdaptEqualizer
    sigOut, H, errSq what the reference returns with returnResults and prec = complex128 (errSq: the real part)
    table, Rcma, Rrde   the constellation, the CMA radius and the RDE radii as the reference computes them in the case's ``prec``
    gap              smallest distance between the two nearest decision candidates over the output symbols of dd-lms / rde stages
    h_change, offdiag   ||H - H0|| / ||H0||; share of ||H||^2 in the rows k + N nModes with k != N (multi-mode cases)
    cfg              JSON: the parameters set on the parameter object, shapes, seed, numpy version, ...
and, for `default_prec` (prec left at complex64, sigIn and symbRef stored as complex64): sigOut64, H64, errSq64, the reference's
complex64 result on the same input, self_err, the rel-L2 distance between its two results, and table128, Rcma128, Rrde128, the
tables of the complex128 run (sigOut, H and errSq are that run's: prec = complex128 on the complex64 input).

Synthetic input: unit-power QAM at SpS samples per symbol (a raised-cosine-like pulse), a short ISI filter, a fixed polarisation
rotation of about 0.6 rad with a phase between neighbouring modes, white noise at 22 dB.

Conditions asserted here, re-asserted by tests/eq_cases.py:check_conditions, so that no fixture lets a test pass emptily:
gap >= 1e-6 where a stage decides; h_change >= 0.1; offdiag >= 0.01 for more than one mode.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_eq.py [case ...]
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

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "eq")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py
SNR_DB = 22

# name: symbols, modes (0 = 1-D input), param (what is set on the parameter object; L as shares of totalNumSymb), prec
_TWO = dict(nTaps=15, SpS=2, numIter=2, mu=[5e-3, 2e-3], L=[0.3, 0.7], M=16, constType="qam")
CASES = {
    "nlms_ddlms": dict(nsym=1500, modes=2, param=dict(_TWO, alg=["nlms", "dd-lms"]), prec="complex128"),
    "darde_rde": dict(nsym=1500, modes=2, param=dict(_TWO, alg=["da-rde", "rde"]), prec="complex128"),
    "cma_rde": dict(nsym=1500, modes=2, param=dict(_TWO, alg=["cma", "rde"]), prec="complex128"),
    "nlms_static": dict(nsym=1500, modes=2, param=dict(_TWO, alg=["nlms", "static"]), prec="complex128"),
    "cma_qpsk_1d": dict(nsym=1500, modes=0, param=dict(alg=["cma"], M=4, nTaps=7, SpS=2), prec="complex128"),
    "nlms_even_taps": dict(nsym=1000, modes=2, param=dict(alg=["nlms"], M=16, nTaps=4, SpS=3, mu=[5e-3], L=[900]), prec="complex128"),
    "ddlms_qam64_3modes": dict(nsym=1200, modes=3, param=dict(_TWO, alg=["nlms", "dd-lms"], M=64), prec="complex128"),
    "default_prec": dict(nsym=1500, modes=2, param=dict(_TWO, alg=["nlms", "dd-lms"]), prec=None),
}


class Param:
    pass


def make_param(d, prec):
    p = Param()
    for k, v in d.items():
        setattr(p, k, v)
    p.returnResults = True
    p.prgsBar = False
    if prec is not None:
        p.prec = np.dtype(prec).type
    return p


def reference_tables(M, constType, prec):
    """The constellation, Rcma and Rrde with the reference's expressions (equalization.py:234-241, 453-456)."""
    c = ref_gray(M, constType).astype(prec)
    px = np.exp(-0 * np.abs(c) ** 2)
    px = px / np.sum(px)
    c /= np.sqrt(np.sum(np.abs(c) ** 2 * px))
    Rcma = ((np.mean(np.abs(c) ** 4) / np.mean(np.abs(c) ** 2)) * np.ones((1, 1)).astype(prec))[0, 0]
    return c, Rcma, np.unique(np.abs(c)).astype(prec)


def make_signal(name, seed):
    c = CASES[name]
    prm = c["param"]
    rng = np.random.default_rng(seed)
    nsym, cols, SpS, M = c["nsym"], max(c["modes"], 1), prm["SpS"], prm["M"]
    table = reference_tables(M, prm.get("constType", "qam"), np.complex128)[0]
    tx = table[rng.integers(0, M, size=(nsym, cols))]
    up = np.zeros((nsym * SpS, cols), dtype=np.complex128)
    up[::SpS] = tx
    t = np.arange(-2 * SpS, 2 * SpS + 1) / SpS
    pulse = np.sinc(t) * np.cos(np.pi * 0.35 * t) / (1 - (2 * 0.35 * t) ** 2)                # raised cosine, roll-off 0.35
    isi = np.array([0.08 - 0.05j, 1.0, 0.22 + 0.12j, -0.06j])
    x = np.empty_like(up)
    for m in range(cols):
        x[:, m] = np.convolve(np.convolve(up[:, m], pulse, mode="same"), isi, mode="full")[1:1 + len(up)]
    th, ph = 0.6, 0.4
    rot = np.array([[np.cos(th), -np.sin(th) * np.exp(1j * ph)], [np.sin(th) * np.exp(-1j * ph), np.cos(th)]])
    for m in range(cols - 1):                                                                # neighbouring modes, in turn
        x[:, m:m + 2] = x[:, m:m + 2] @ rot.T
    x = x * 0.7                                                                              # (the equalizer has a gain to find)
    sigma2 = np.mean(np.abs(x) ** 2) * 10 ** (-SNR_DB / 10)
    x = x + (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape)) * np.sqrt(sigma2 / 2)
    if c["modes"] == 0:
        x, tx = x[:, 0].copy(), tx[:, 0].copy()
    return x, tx


def stage_list(name, total):
    prm = dict(CASES[name]["param"])
    if "L" in prm and all(isinstance(v, float) for v in prm["L"]):
        first = int(round(prm["L"][0] * total))
        prm["L"] = [first, total - first]
    return prm


def decision_gap(alg, L, sigOut, table, Rrde):
    """Smallest difference between the two nearest candidates over the stored outputs of every deciding stage."""
    y2 = sigOut.reshape(len(sigOut), -1)
    gap, start = np.inf, 0
    for a, ln in zip(alg, L):
        y = y2[start:start + ln].reshape(-1)
        if a == "dd-lms":
            d = np.sort(np.abs(y[:, None] - table[None, :]), axis=1)
            gap = min(gap, float(np.min(d[:, 1] - d[:, 0])))
        elif a == "rde" and len(Rrde) > 1:
            d = np.sort(np.abs(Rrde[None, :] - np.abs(y)[:, None]), axis=1)
            gap = min(gap, float(np.min(d[:, 1] - d[:, 0])))
        start += ln
    return gap


def coefficient_measures(H, nModes, nTaps):
    H0 = np.zeros_like(H)
    for k in range(nModes):
        H0[k + k * nModes, nTaps // 2] = 1
    diag = [k + k * nModes for k in range(nModes)]
    off = [r for r in range(nModes ** 2) if r not in diag]
    total = float(np.sum(np.abs(H) ** 2))
    return (float(np.linalg.norm(H - H0) / np.linalg.norm(H0)), float(np.sum(np.abs(H[off]) ** 2) / total) if off else 0.0)


def run_reference(x, tx, prm, prec):
    keep_x, keep_t = x.copy(), tx.copy()
    sigOut, H, errSq, Hiter = ref_eq.mimoAdaptEqualizer(x, make_param(prm, prec), tx)
    assert np.array_equal(x, keep_x) and np.array_equal(tx, keep_t)
    return sigOut, H, errSq


def acceptable(v, modes):
    return v["gap"] >= 1e-6 and v["h_change"] >= 0.1 and (modes < 2 or v["offdiag"] >= 0.01)


def generate(name):
    c = CASES[name]
    nTaps, SpS = c["param"].get("nTaps", 15), c["param"].get("SpS", 2)
    n = c["nsym"] * SpS
    total = int(np.fix((n + 2 * (nTaps // 2) - nTaps) / SpS + 1))
    prm = stage_list(name, total)
    modes = max(c["modes"], 1)
    prec = c["prec"] or "complex64"
    table, Rcma, Rrde = reference_tables(prm["M"], prm.get("constType", "qam"), prec)
    first = 3000 + sorted(CASES).index(name)
    for seed in range(first, first + 50):
        x, tx = make_signal(name, seed)
        if c["prec"] is None:
            x, tx = x.astype(np.complex64), tx.astype(np.complex64)
        sigOut, H, errSq = run_reference(x, tx, prm, "complex128")
        L = prm.get("L", [total])
        v = dict(gap=decision_gap(prm["alg"], L, sigOut, table.astype(np.complex128), Rrde.real.astype(np.float64)))
        v["h_change"], v["offdiag"] = coefficient_measures(H, modes, nTaps)
        if acceptable(v, modes):
            break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 50}) meets the conditions: {v}")
    assert sigOut.dtype == np.complex128 and H.dtype == np.complex128 and H.shape == (modes ** 2, nTaps)
    assert sigOut.shape[0] == total and errSq.shape == (modes, total) and np.all(errSq.imag == 0)
    assert np.all(sigOut.reshape(total, -1)[sum(L):] == 0)
    errSq = np.array(errSq.real)
    if "static" in prm["alg"]:                       # the reference leaves np.empty garbage there: stored as 0, never compared
        errSq[:, sum(L[:prm["alg"].index("static")]):] = 0
    out = dict(sigIn=x, symbRef=tx, sigOut=sigOut, H=H, errSq=np.ascontiguousarray(errSq), table=table, Rcma=np.asarray(Rcma),
               Rrde=Rrde, gap=v["gap"], h_change=v["h_change"], offdiag=v["offdiag"])
    if c["prec"] is None:
        s64, H64, e64 = run_reference(x, tx, prm, None)
        assert s64.dtype == np.complex64 and H64.dtype == np.complex64
        self_err = float(np.linalg.norm(s64.astype(np.complex128) - sigOut) / np.linalg.norm(sigOut))
        t128, R128, r128 = reference_tables(prm["M"], prm.get("constType", "qam"), "complex128")
        out.update(sigOut64=s64, H64=H64, errSq64=np.ascontiguousarray(e64.real), self_err=self_err, table128=t128, Rcma128=np.asarray(R128),
                   Rrde128=r128)
    cfg = dict(name=name, param=prm, prec=c["prec"], n=int(n), total=total, modes=modes, input1D=c["modes"] == 0, shape=list(x.shape),
               dtype=x.dtype.name, snr_dB=SNR_DB, seed=seed, numpy=np.__version__, L=L, alg=prm["alg"])
    out["cfg"] = json.dumps(cfg)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"eq_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size >> 10} KiB  seed {seed}  gap {v['gap']:.2e}  H change {v['h_change']:.3f}  off-diagonal {v['offdiag']:.3f}"
          + (f"  self_err {out['self_err']:.2e}" if c["prec"] is None else ""), flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        generate(case)
