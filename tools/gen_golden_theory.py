#!/usr/bin/env python3
"""Generate the theoretical-MI fixtures tests/golden/theory/*.npz by IMPORTING THE REFERENCE, and measure the quadrature rule.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As its siblings do, it registers a throw-away ``numba`` stub first (``njit`` = identity: the reference runs
without a JIT, which is why theoryMI takes seconds to minutes here).  No bytecode is written.

<theoryMI case>.npz  table (the reference's normalised table, widened) and pX bit for bit, sigma, ref (one value per entry of
                     cfg.symmetry, at cfg.tol), ref_default (the same at the default tol = 1e-3), restatement (the long-double rule
                     of tests/theory_restatement.py, rounded to double), seconds (the reference's run times)
calc_*.npz           rx, tx, sigma2 (np.var(rx - tx)), table, pX, mi (the reference's calcMI)
gn_model.npz         GNmodel_OSNR and calcLinOSNR at the settings of examples/test_metrics.ipynb, one condEntropy value
shape_rows.npz       the restatement's values of the rows of tests/theory_cases.py (the large ones take minutes in long double)

Conditions asserted here: |ref(tol = 1e-9) - restatement| <= 1e-7; for 64-QAM the symmetry=False value is within 0.01 of the
restatement (so that the 0.023 between it and the symmetry=True value stays visible).

--sweep  measures the rule (h = 0.1, T = 6.5) against h / 2 in long double and writes profiles/theory_quadrature.json.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_theory.py [--sweep | case ...]
"""
import importlib.util
import json
import multiprocessing
import os
import sys
import time
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

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[1:1] = [os.path.join(_ROOT, "tests")]
import theory_cases as tc  # noqa: E402
import theory_restatement as rs  # noqa: E402

MAX_BYTES = 300000


def _ref():
    import optic.comm.metrics as ref_metrics
    import optic.comm.modulation as ref_mod
    import optic.dsp.core as ref_core
    from optic.utils import parameters
    return ref_metrics, ref_mod, ref_core, parameters


def save(name, cfg, **arrays):
    os.makedirs(tc.GOLDEN, exist_ok=True)
    path = os.path.join(tc.GOLDEN, f"{name}.npz")
    np.savez_compressed(path, cfg=json.dumps(dict(cfg, name=name, numpy=np.__version__)), **arrays)
    assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
    print(f"{name}: {os.path.getsize(path) >> 10} KiB", flush=True)


def ref_table(M, constType):
    """The table as the reference's theoryMI forms it: complex64 through the normalisation."""
    ref_metrics, ref_mod, ref_core, _ = _ref()
    const = ref_mod.grayMapping(M, constType)
    return const / np.sqrt(ref_core.signalPower(const))


def generate_mi(name):
    ref_metrics = _ref()[0]
    c = tc.MI_CASES[name]
    table = ref_table(c["M"], c["constType"])
    px = tc.maxwell_boltzmann(table) if c["px"] == "mb" else None
    sigma = float(rs.sigma_of(c["SNR"]))
    pxa = np.ones(c["M"]) / c["M"] if px is None else px
    restated = rs.rule_mi(table, pxa, sigma)
    ref, ref_default, seconds = [], [], []
    for sym in c["symmetry"]:
        t0 = time.time()
        ref_default.append(float(ref_metrics.theoryMI(c["M"], c["constType"], c["SNR"], pX=px, symmetry=sym)))
        seconds.append(time.time() - t0)
        if c["tol"] is not None:
            t0 = time.time()
            ref.append(float(ref_metrics.theoryMI(c["M"], c["constType"], c["SNR"], pX=px, symmetry=sym, tol=c["tol"])))
            seconds.append(time.time() - t0)
        else:
            ref.append(ref_default[-1])
        print(f"    {name} symmetry={sym}: ref {ref[-1]:.12f} default {ref_default[-1]:.12f} restatement {float(restated):.12f}", flush=True)
    dist = [abs(r - float(restated)) for r in ref]
    if c["tol"] is not None:
        assert max(dist) <= tc.REF_FIX, (name, dist)
    else:
        k = c["symmetry"].index(False)
        assert dist[k] < tc.QUIRK, (name, dist)
    save(name, dict(c, kind="mi"), table=table.astype(np.complex128), px=pxa, sigma=sigma, ref=np.array(ref), ref_default=np.array(ref_default),
         restatement=np.float64(restated), distance=np.array(dist), seconds=np.array(seconds))


def generate_calc(name):
    ref_metrics, ref_mod, ref_core, _ = _ref()
    c = tc.CALC_CASES[name]
    rng = np.random.default_rng(4000 + sorted(tc.CALC_CASES).index(name))
    const = ref_mod.grayMapping(c["M"], c["constType"])
    px = np.ones(c["M"]) / c["M"]
    if c["shaped"]:
        px = tc.maxwell_boltzmann(const / np.sqrt(np.mean(np.abs(const) ** 2)), 0.8)
    Es = np.sum(np.abs(const) ** 2 * px)
    table = const / np.sqrt(Es)
    wide = np.complex128 if np.iscomplexobj(const) else np.float64
    tx = table.astype(wide)[rng.choice(c["M"], size=tc.CALC_N, p=px)]
    s = float(rs.sigma_of(c["SNR"]))
    noise = rng.normal(size=tc.CALC_N) * s
    if wide is np.complex128:
        noise = noise + 1j * rng.normal(size=tc.CALC_N) * s
    rx = (tx + noise).astype(c["dtype"])
    tx = tx.astype(c["dtype"])
    sigma2 = float(np.var(rx - tx))
    mi = ref_metrics.calcMI(rx, tx, sigma2, table, px)
    restated = float(rs.calc_mi(rx, tx, sigma2, table, px))
    assert mi.shape == (1,) and mi.dtype == np.float64
    # (single-precision data: the reference's distances are single-precision too)
    assert abs(mi[0] - restated) <= (1e-5 if c["dtype"] == "complex64" else 1e-12) * abs(restated), (name, mi[0], restated)
    save(name, dict(c, kind="calc"), rx=rx, tx=tx, sigma2=sigma2, table=table, px=px, mi=mi, restatement=restated)
    print(f"    {name}: ref {mi[0]:.12f} restatement {restated:.12f}", flush=True)


def generate_gn():
    ref_metrics, _, _, parameters = _ref()
    p = parameters()
    p.Ltotal, p.Lspan, p.alpha, p.D, p.gamma, p.Fc = 700, 50, 0.2, 16, 1.3, 193.1e12
    Ptx = np.arange(-10, 1.5, 0.5)
    OSNR, P_nli, P_ase = ref_metrics.GNmodel_OSNR(32e9, 80, 37.5e9, Ptx, p, 12.5e9)
    OSNR_default = ref_metrics.GNmodel_OSNR(32e9, 80, 37.5e9, Ptx)[0]
    lin = ref_metrics.calcLinOSNR(14, -4, 0.2, 50, 35, 6, 193.1e12, 12.5e9)
    table = ref_table(16, "qam")
    ce = ref_metrics.condEntropy(0.3, -0.2, table, np.ones(16) / 16, 5, 0.25)
    save("gn_model", dict(kind="gn"), Ptx=Ptx, OSNR=OSNR, P_nli=P_nli, P_ase=P_ase, OSNR_default=OSNR_default, lin=lin,
         gn_one=ref_metrics.GN_Model_NyquistWDM(32e9, 80, 37.5e9, 0.2, 1.3, 50, 14, -2.0, 16, 12.5e9, 193.1e12),
         ase_one=ref_metrics.ASE_NyquistWDM(0.2, 50, 14, 4.5, 12.5e9, 193.1e12), cond_entropy=np.float64(ce), table16=table.astype(np.complex128))


def _terms(job):
    table, px, sigma, idx = job
    return rs.point_terms(table, px, sigma, idx)


def generate_rows():
    out = {}
    with multiprocessing.Pool(8) as pool:
        for row in tc.SHAPE_ROWS:
            table, px, sigma = tc.row_input(row)
            vals = []
            for s in sigma:
                chunks = [list(range(i, row["M"], 8)) for i in range(min(8, row["M"]))]
                terms = pool.map(_terms, [(table, px, s, ch) for ch in chunks])
                tot = rs.LD(0)
                for i in range(row["M"]):                       # points in their order
                    tot += terms[i % 8][i // 8]
                vals.append(float(rs.LD(rs.entropy(px)) - tot))
            out[row["name"]] = np.array(vals)
            print(f"    {row['name']}: {vals[:3]}", flush=True)
    save("shape_rows", dict(kind="rows"), **out)


def _pair(job):
    table, px, sigma, idx = job
    return rs.point_terms_pair(table, px, sigma, idx)


def _psk_errors(pool, table, snrs):
    """|rule(h) - rule(h / 2)| per SNR from one point per orbit of the grid's symmetries (M / 8 + 1 points from M = 8 on)."""
    orbits = rs.d4_orbits(table)
    px = np.ones(len(table)) / len(table)
    reps, mult = [i for i, _ in orbits], np.array([m for _, m in orbits]).astype(rs.LD)
    chunks = [reps[k::4] for k in range(4) if reps[k::4]]
    jobs = [(table, px, float(rs.sigma_of(snr)), ch) for snr in snrs for ch in chunks]
    out = pool.map(_pair, jobs, chunksize=1)
    errs = []
    for n in range(len(snrs)):
        diff = rs.LD(0)
        for k, ch in enumerate(chunks):
            coarse, fine = out[n * len(chunks) + k]
            diff += np.sum(mult[k::4] * (coarse - fine))
        errs.append(float(abs(diff)))
    return errs, len(reps)


def sweep():
    snrs = np.arange(-10.0, 40.01, 2.5)
    worst, cases = dict(err=0.0), []
    pool = multiprocessing.Pool(8)
    for M in (2, 4, 8, 16, 64, 256, 1024):
        for ct in ("qam", "psk", "pam"):
            if ct == "qam" and int(round(np.sqrt(M))) ** 2 != M:
                continue
            table = ref_table(M, ct).astype(np.complex128)
            errs, points = [], None
            if ct == "psk":
                errs, points = _psk_errors(pool, table, snrs)
            for snr in (snrs if ct != "psk" else ()):
                s = float(rs.sigma_of(snr))
                if ct == "qam":
                    lv = np.unique(table.real)
                    f = lambda h: rs.rule_mi_separable(lv, np.unique(table.imag), s, h)     # noqa: E731
                else:
                    f = lambda h: rs.rule_mi_real(table, None, s, h)                        # noqa: E731
                errs.append(float(abs(f(rs.H_STEP) - f(rs.H_STEP / 2))))
            k = int(np.argmax(errs))
            cases.append(dict(M=M, constType=ct, worst=errs[k], at_dB=float(snrs[k]), **({} if points is None else {"points": points})))
            print(f"    {ct}{M}: worst {errs[k]:.2e} at {snrs[k]} dB", flush=True)
            if errs[k] > worst["err"]:
                worst = dict(err=errs[k], M=M, constType=ct, at_dB=float(snrs[k]))
    path = os.path.join(_ROOT, "profiles", "theory_quadrature.json")
    with open(path, "w") as f:
        json.dump(dict(h=rs.H_STEP, T=rs.T_MAX, against="h/2 in np.longdouble", snr_dB=list(map(float, snrs)), bound=tc.RULE_BOUND,
                       worst=worst, cases=cases,
                       forms="qam by the exact separable form, pam by the 1-D form, psk by one point per orbit of the grid's symmetries"),
                  f, indent=1)
    pool.close()
    assert worst["err"] <= tc.RULE_BOUND, worst


if __name__ == "__main__":
    if sys.argv[1:] == ["--sweep"]:
        sweep()
        sys.exit(0)
    for nm in sys.argv[1:] or list(tc.MI_CASES) + list(tc.CALC_CASES) + ["gn_model", "shape_rows"]:
        if nm in tc.MI_CASES:
            generate_mi(nm)
        elif nm in tc.CALC_CASES:
            generate_calc(nm)
        elif nm == "gn_model":
            generate_gn()
        else:
            generate_rows()
