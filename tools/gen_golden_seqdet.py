#!/usr/bin/env python3
"""Generate the mlse / detector / whitening-filter fixtures tests/golden/seqdet/*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_siso.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity), and one
for ``tqdm.notebook`` if that is missing: the reference is then plain Python (0.8 s for 256 states and 500 symbols).  No bytecode is
written.

mlse_*.npz   y, h, c (the constellation), tx (transmitted indices), out (the reference's mlse output), det (the indices its
             detector decides under 'ML' on the same y), index / metric / gap / final_gap / ties (read off
             tests/seqdet_restatement.py, which is held to the reference's output here), ser_mlse, ser_det, cfg (JSON)
det_*.npz    r, c, px (where given), decided, ind (the reference's), gap (restatement), cfg
white_*.npz  x, r, w (the reference's autocorr and estimateWhiteningFilter), kmax (largest reflection coefficient), cfg

mlse input: unit-power Gray constellations, np.convolve(s, h)[:N] plus white Gaussian noise (numpy.random.default_rng).
Conditions asserted here and re-asserted by tests/seqdet_cases.py:check_conditions, so that no fixture lets a test pass emptily:
the restatement reproduces the reference's sequence exactly; every non-zero gap between the best and the second-best candidate,
and between the two lowest final metrics, is at least 1e-9 (1 + best); `*_ties` hold exact ties, the others none; the detected
sequence differs from the transmitted one somewhere and from detector's in at least 10 % of the symbols (except at L = 0, and
except for the two 4-QAM cases: at sigma = 0.15 per part their eye is open, over thirty seeds mlse made no symbol error and
differed from detector in 1.5 ... 10.8 % of the symbols, so these two only have to differ from detector somewhere -- `open_eye`);
detector metrics differ by at least 1e-6 at every symbol; every reflection coefficient is below 0.95 in magnitude.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_seqdet.py [case ...]
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

import optic.comm.modulation as ref_mod  # noqa: E402
import optic.dsp.core as ref_core  # noqa: E402

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[1:1] = [_ROOT, os.path.join(_ROOT, "tests")]
import seqdet_restatement as rs  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "seqdet")
MAX_BYTES = 282045          # the cap of tools/gen_golden_siso.py
GAP = 1e-9

_H1 = [1, .7]
MLSE = {
    "pam4_L3": dict(const=(4, "pam"), h=[1, .6, .3, .1], N=1200, sigma=0.2),
    "pam4_L4": dict(const=(4, "pam"), h=[1, .5, .3, .2, .1], N=500, sigma=0.2),
    "pam4_L0": dict(const=(4, "pam"), h=[0.9], N=1200, sigma=0.2),
    "pam4_L1": dict(const=(4, "pam"), h=_H1, N=1200, sigma=0.2),
    "pam8_L2": dict(const=(8, "pam"), h=[1, .5, .2], N=1000, sigma=0.1),
    "pam2_L10": dict(const=(2, "pam"), h=[1, .6, .5, .4, .3, .3, .2, .2, .1, .1, .05], N=250, sigma=0.3),
    "pam4_ties": dict(const=(4, "pam"), h=[1, .6, 0, 0], N=600, sigma=0.2, ties=True),
    "qpsk_L2": dict(const=(4, "qam"), h=[1, .5 + .2j, .2j], N=800, sigma=0.15, open_eye=True),
    "qpsk_ties": dict(const=(4, "qam"), h=[1, .5 + .2j, 0, 0], N=400, sigma=0.15, ties=True, open_eye=True),
    "pam4_f32": dict(const=(4, "pam"), h=_H1, N=1200, sigma=0.2, dtype="float32"),
}
DET = {
    "qam16_ml": dict(const=(16, "qam"), n=2000, sigma=0.25, rule="ML"),
    "qam16_map_uniform": dict(const=(16, "qam"), n=2000, sigma=0.25, rule="MAP"),
    "qam4_map_px": dict(const=(4, "qam"), n=2000, sigma=0.6, rule="MAP", px=[.4, .3, .2, .1]),
    "pam4_ml_real": dict(const=(4, "pam"), n=2000, sigma=0.3, rule="ML"),
    "two_point_map": dict(table=[-1.0 + 0j, 1.0 + 0j], r=[0.05 + 0j], sigma2=1.0, rule="MAP", px=[.99, .01]),
}
WHITE = {"white_2": 2, "white_5": 5, "white_16": 16}


def constellation(M, kind):
    c = ref_core.pnorm(ref_mod.grayMapping(M, kind))
    return np.asarray(c).astype(np.complex128 if kind == "qam" else np.float64)


def save(name, out, cfg):
    out["cfg"] = json.dumps(dict(cfg, name=name, numpy=np.__version__))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    return size


def gen_mlse(name, first):
    case = MLSE[name]
    M, kind = case["const"]
    c, h, N, sigma = constellation(M, kind), np.array(case["h"]), case["N"], case["sigma"]
    cx, L = kind == "qam", len(case["h"]) - 1
    why = "no seed tried"
    for seed in range(first, first + 50):
        rng = np.random.default_rng(seed)
        tx = rng.integers(0, M, size=N)
        y = np.convolve(c[tx], h)[:N]
        y = y + sigma * ((rng.normal(size=N) + 1j * rng.normal(size=N)) if cx else rng.normal(size=N))
        y = y.astype(case.get("dtype", y.dtype))
        keep = y.copy()
        out = ref_mod.mlse(y, h, c)
        assert np.array_equal(y, keep) and out.dtype == y.dtype and out.shape == (N,)
        r = rs.mlse(y, h, c)
        _, det = ref_mod.detector(y, 1.0, c, rule="ML")
        ser_mlse, ser_det, differ = float(np.mean(r["index"] != tx)), float(np.mean(det != tx)), float(np.mean(det != r["index"]))
        if not np.array_equal(c[r["index"]].astype(y.dtype), out):
            why = "the restatement does not reproduce the reference"
        elif r["gap"] < GAP or r["final_gap"] < GAP:
            why = f"gap {r['gap']:.2e}, final gap {r['final_gap']:.2e}"
        elif bool(r["ties"]) != bool(case.get("ties")):
            why = f"{r['ties']} ties"
        elif L > 0 and (differ == 0 if case.get("open_eye") else (ser_mlse == 0 or differ < 0.1)):
            why = f"ser {ser_mlse}, differs from detector in {differ}"
        else:
            break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 50}) meets the conditions: {why}")
    cfg = dict(kind="mlse", M=M, constType=kind, L=L, N=N, sigma=sigma, seed=seed, dtype=y.dtype.name, states=r["states"], ties=bool(case.get("ties")),
               open_eye=bool(case.get("open_eye")))
    size = save(f"mlse_{name}", dict(y=y, h=h, c=c, tx=tx, out=out, det=det, index=r["index"], metric=np.float64(r["metric"]),
                                     gap=np.float64(r["gap"]), final_gap=np.float64(r["final_gap"]), ties=np.int64(r["ties"]),
                                     ser_mlse=np.float64(ser_mlse), ser_det=np.float64(ser_det), differ=np.float64(differ)), cfg)
    print(f"mlse_{name}: {size >> 10} KiB  seed {seed}  states {r['states']}  gap {r['gap']:.2e}  final gap {r['final_gap']:.2e}  ties {r['ties']}  "
          f"ser {ser_mlse:.3f} (detector {ser_det:.3f})", flush=True)


def gen_det(name, first):
    case = DET[name]
    px = None if "px" not in case else np.array(case["px"])
    for seed in range(first, first + 50):
        if "table" in case:
            c, r, sigma2 = np.array(case["table"]), np.array(case["r"]), case["sigma2"]
        else:
            rng = np.random.default_rng(seed)
            M, kind = case["const"]
            c, n, sigma = constellation(M, kind), case["n"], case["sigma"]
            tx = rng.choice(M, size=n, p=px)
            noise = (rng.normal(size=n) + 1j * rng.normal(size=n)) / np.sqrt(2) if kind == "qam" else rng.normal(size=n)
            r, sigma2 = c[tx] + sigma * noise, sigma ** 2
        keep = r.copy()
        decided, ind = ref_mod.detector(r, sigma2, c, px=px, rule=case["rule"])
        assert np.array_equal(r, keep) and decided.dtype == r.dtype and ind.dtype == np.int64
        got, gap = rs.detector(r, sigma2, c, px, case["rule"])
        if np.array_equal(got, ind) and gap >= 1e-6:
            break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 50}) meets the conditions (gap {gap:.2e})")
    out = dict(r=r, c=c, decided=decided, ind=ind, gap=np.float64(gap))
    if px is not None:
        out["px"] = px
    cfg = dict(kind="detector", rule=case["rule"], sigma2=float(sigma2), seed=seed, M=len(c), has_px=px is not None)
    size = save(f"det_{name}", out, cfg)
    print(f"det_{name}: {size >> 10} KiB  seed {seed}  gap {gap:.2e}  decisions off the nearest point: "
          f"{int(np.sum(ind != rs.detector(r, sigma2, c, None, 'ML')[0]))}", flush=True)


def gen_white(name, first):
    nTaps, n = WHITE[name], 4000
    for seed in range(first, first + 50):
        rng = np.random.default_rng(seed)
        e = rng.normal(size=n + 200)
        x = np.zeros(n + 200)
        for i in range(2, n + 200):                       # AR(2): poles at 0.8 exp(+-0.9j)
            x[i] = e[i] + 2 * 0.8 * np.cos(0.9) * x[i - 1] - 0.64 * x[i - 2]
        x = x[200:].copy()
        r = ref_core.autocorr(x, nTaps)
        w = ref_core.estimateWhiteningFilter(x, nTaps)
        assert r.dtype == np.float64 and w.dtype == np.float64 and r.shape == w.shape == (nTaps,)
        _, ks = rs.levinson(rs.autocorr(x, nTaps), nTaps)
        kmax = float(np.max(np.abs(ks))) if len(ks) else 0.0
        if kmax < 0.95:
            break
    else:
        raise SystemExit(f"{name}: no seed meets the conditions (kmax {kmax})")
    size = save(name, dict(x=x, r=r, w=w, kmax=np.float64(kmax)), dict(kind="white", nTaps=nTaps, n=n, seed=seed))
    print(f"{name}: {size >> 10} KiB  seed {seed}  largest reflection coefficient {kmax:.3f}", flush=True)


if __name__ == "__main__":
    names = [f"mlse_{k}" for k in MLSE] + [f"det_{k}" for k in DET] + list(WHITE)
    for i, full in enumerate(names):
        if sys.argv[1:] and full not in sys.argv[1:]:
            continue
        first = 7000 + 50 * i
        if full.startswith("mlse_"):
            gen_mlse(full[5:], first)
        elif full.startswith("det_"):
            gen_det(full[4:], first)
        else:
            gen_white(full, first)
