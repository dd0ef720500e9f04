#!/usr/bin/env python3
"""Generate the carrier-recovery fixtures tests/golden/cpr/cpr_*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE); never on the GPU box.  As tools/gen_golden_metrics.py does, it
registers a throw-away ``numba`` stub first (``njit`` = identity): ``bps`` is then the plain Python loop, a few seconds per mode.
No bytecode is written.

Each file holds
    sigIn         the symbols as handed to cpr: noisy QAM / PSK with a Wiener phase walk (and a frequency offset in the FOE cases)
    table         cpr's normalised constellation (complex64, as the reference computes it)
    sigOut, phaseEst   what the reference's cpr returns with returnPhases
    raw           the raw test phases bps returned inside that call, (n, nModes)
    sig_foe, fo   fourthPowerFOE(sigIn, 1 / Ts, P) in the FOE cases
    min_margin    smallest (second-smallest - smallest) / smallest window sum over the test phases, of any symbol
    unwrap_margin smallest | |diff(4 raw)| - pi |
    distinct, max_step    number of distinct raw phases; largest |diff(raw)|
    foe_margin    FOE cases: smallest relative excess of the peak's squared magnitude over any other bin
    cfg           JSON: the parameters set on the parameter object (`param`), n, shape, dtype, snr_dB, seed, numpy version, ...

Conditions asserted here, re-asserted by tests/cpr_cases.py:check_conditions, so that the tests cannot pass emptily:
min_margin >= 1e-7; unwrap_margin >= 1e-3; except for `short_window`, distinct >= B / 4 and max_step > pi / 4; in the FOE cases
fo != 0 and foe_margin >= 1e-6.  The seed of a case is the first one from 2000 + its position in the sorted list of names at
which a numpy restatement of the search (bpsGPU's formulation) meets these conditions; the reference then runs once on that signal
and the conditions are asserted on what it returned.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_cpr.py [case ...]
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
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

import optic.dsp.carrierRecovery as ref_cr  # noqa: E402
from optic.comm.modulation import grayMapping as ref_gray  # noqa: E402
from optic.dsp.core import pnorm as ref_pnorm  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "cpr")
MAX_BYTES = 282045          # the largest file of tests/golden/metrics/
RS = 32e9

# name: n, modes (0 = 1-D input), param (what is set on the parameter object), snr_dB, linewidth [Hz], frequency offset [Hz], extras
CASES = {
    "qam16_bps": dict(n=3000, modes=2, param=dict(M=16, constType="qam", N=35, B=64, runFOE=False), snr=20, lw=2e6, fo=0.0),
    "qam64_foe": dict(n=2000, modes=2, param=dict(M=64, constType="qam", N=85, B=64, runFOE=True, Ts=1 / RS), snr=26, lw=1e6,
                      fo=61.3e6),
    "qam16_defaults_1d": dict(n=2048, modes=0, param=dict(M=16), snr=20, lw=2e6, fo=-38.7e6),
    "qpsk_b32": dict(n=1500, modes=1, param=dict(M=4, constType="qam", N=25, B=32, runFOE=False), snr=12, lw=4e6, fo=0.0),
    "psk4_foe": dict(n=1500, modes=1, param=dict(M=4, constType="psk", N=25, B=21, runFOE=True, Ts=1 / RS), snr=14, lw=3e6,
                     fo=23.1e6),
    "qam256_c64": dict(n=2000, modes=1, param=dict(M=256, constType="qam", N=85, B=64, runFOE=False), snr=32, lw=1e6, fo=0.0,
                       dtype="complex64"),
    "qam64_shaped": dict(n=2000, modes=1, param=dict(M=64, constType="qam", N=35, B=64, runFOE=False, shapingFactor=0.03), snr=24,
                         lw=2e6, fo=0.0),
    "qam16_4modes": dict(n=1200, modes=4, param=dict(M=16, constType="qam", N=75, B=64, runFOE=False), snr=18, lw=4e6, fo=0.0),
    "short_window": dict(n=20, modes=2, param=dict(M=16, constType="qam", N=35, B=64, runFOE=False), snr=20, lw=2e6, fo=0.0),
}


class Param:
    pass


def make_param(d, returnPhases=True):
    p = Param()
    for k, v in d.items():
        setattr(p, k, v)
    p.returnPhases = returnPhases
    return p


def reference_table(M, constType, shapingFactor):
    c = ref_gray(M, constType)
    px = np.exp(-shapingFactor * np.abs(c) ** 2)
    px = px / np.sum(px)
    c /= np.sqrt(np.sum(np.abs(c) ** 2 * px))
    return c, px


def make_signal(name, seed):
    c = CASES[name]
    rng = np.random.default_rng(seed)
    prm = c["param"]
    n, cols = c["n"], max(c["modes"], 1)
    table, px = reference_table(prm["M"], prm.get("constType", "qam"), prm.get("shapingFactor", 0))
    idx = rng.choice(prm["M"], size=(n, cols), p=px.astype(np.float64) / np.sum(px.astype(np.float64)))
    tx = table.astype(np.complex128)[idx]
    sigma2 = 10 ** (-c["snr"] / 10)
    noise = (rng.normal(size=(n, cols)) + 1j * rng.normal(size=(n, cols))) * np.sqrt(sigma2 / 2)
    walk = np.cumsum(rng.normal(size=(n, cols)) * np.sqrt(2 * np.pi * c["lw"] / RS), axis=0) + rng.uniform(0, np.pi / 2, size=(1, cols))
    k = np.arange(n)[:, None]
    x = (tx + noise) * np.exp(1j * (walk + 2 * np.pi * c["fo"] * k / RS))
    if c["modes"] == 0:
        x = x[:, 0].copy()
    return x.astype(c.get("dtype", "complex128"))


def window_margins(x2d, Nh, table, B):
    """Per symbol the index of the smallest window sum and (second-smallest - smallest) / smallest, in bpsGPU's formulation."""
    n, modes = x2d.shape
    phases = np.arange(0, B) * (np.pi / 2) / B
    tab = table.astype(np.complex128)
    idx = np.zeros((n, modes), dtype=np.int64)
    margin = np.zeros((n, modes))
    for m in range(modes):
        xp = np.concatenate((np.zeros(Nh, complex), x2d[:, m].astype(np.complex128), np.zeros(Nh, complex)))
        dmin = np.empty((len(xp), B))
        for s in range(0, len(xp), 256):
            rot = xp[s:s + 256, None] * np.exp(1j * phases)[None, :]
            dmin[s:s + 256] = np.min(np.abs(rot[:, :, None] - tab[None, None, :]) ** 2, axis=2)
        sums = np.lib.stride_tricks.sliding_window_view(dmin, 2 * Nh + 1, axis=0).sum(axis=-1)
        order = np.sort(sums, axis=1)
        idx[:, m] = np.argmin(sums, axis=1)
        margin[:, m] = (order[:, 1] - order[:, 0]) / order[:, 0] if B > 1 else np.inf
    return idx, margin


def measure(raw, margin):
    steps4 = np.abs(np.diff(4 * raw, axis=0))
    return dict(min_margin=float(np.min(margin)), unwrap_margin=float(np.min(np.abs(steps4 - np.pi))),
                distinct=int(len(np.unique(raw))), max_step=float(np.max(np.abs(np.diff(raw, axis=0)))))


def acceptable(name, v, B):
    ok = v["min_margin"] >= 1e-7 and v["unwrap_margin"] >= 1e-3
    if name != "short_window":
        ok = ok and v["distinct"] >= B / 4 and v["max_step"] > np.pi / 4
    return ok


def pick_seed(name, table, N, B, foe, Ts, P):
    """First seed at which the numpy restatement meets the conditions."""
    first = 2000 + sorted(CASES).index(name)
    for seed in range(first, first + 200):
        x = make_signal(name, seed)
        x2d = x.reshape(len(x), -1).astype(np.complex128)
        if foe:
            x2d = ref_pnorm(ref_cr.fourthPowerFOE(x2d, 1 / Ts, P)[0])
        idx, margin = window_margins(x2d, N // 2, table, B)
        if acceptable(name, measure((np.arange(0, B) * (np.pi / 2) / B)[idx], margin), B):
            return seed
    raise SystemExit(f"{name}: no seed in [{first}, {first + 200}) meets the conditions")


def generate(name):
    c = CASES[name]
    prm = c["param"]
    M, ct = prm["M"], prm.get("constType", "qam")
    N, B = prm.get("N", 35), prm.get("B", 64)
    Ts, foe = prm.get("Ts", 1 / 32e9), prm.get("runFOE", True)
    table, _ = reference_table(M, ct, prm.get("shapingFactor", 0))
    assert table.dtype == np.complex64
    seed = pick_seed(name, table, N, B, foe, Ts, M if ct == "psk" else 4)
    x = make_signal(name, seed)

    # the reference's cpr, with its bps recorded on the way
    seen = {}
    real_bps = ref_cr.bps

    def recording_bps(sigIn, Nhalf, constSymb, nB):
        seen["in"], seen["Nh"], seen["table"] = sigIn.copy(), Nhalf, constSymb.copy()
        seen["raw"] = real_bps(sigIn, Nhalf, constSymb, nB)
        return seen["raw"].copy()

    ref_cr.bps = recording_bps
    try:
        keep = x.copy()
        sigOut, phaseEst = ref_cr.cpr(x, make_param(prm))
    finally:
        ref_cr.bps = real_bps
    assert np.array_equal(x, keep)
    assert np.array_equal(seen["table"], table) and seen["Nh"] == N // 2
    raw = seen["raw"]

    idx, margin = window_margins(seen["in"], N // 2, table, B)
    phases = np.arange(0, B) * (np.pi / 2) / B
    assert np.array_equal(phases[idx], raw), name                                  # the restatement decides as the reference does
    v = measure(raw, margin)
    assert acceptable(name, v, B), (name, v)
    min_margin, unwrap_margin, distinct, max_step = v["min_margin"], v["unwrap_margin"], v["distinct"], v["max_step"]

    out = dict(sigIn=x, table=table, sigOut=sigOut, phaseEst=phaseEst, raw=raw.reshape(phaseEst.shape), min_margin=min_margin,
               unwrap_margin=unwrap_margin, distinct=distinct, max_step=max_step)
    if foe:
        P = M if ct == "psk" else 4
        x2d = x.reshape(len(x), -1)
        sig_foe, fo = ref_cr.fourthPowerFOE(x2d.astype(np.complex128), 1 / Ts, P)
        spec = np.abs(np.fft.fftshift(np.fft.fft(x2d.astype(np.complex128) ** P, axis=0), axes=0)) ** 2
        top = np.sort(spec, axis=0)
        foe_margin = float(np.min((top[-1] - top[-2]) / top[-2]))
        assert np.all(fo != 0) and foe_margin >= 1e-6, (name, fo, foe_margin)
        if x.dtype == np.complex128:                                               # (cpr's own FOE ran on the same values)
            assert np.array_equal(ref_pnorm(sig_foe), seen["in"]), name
        out.update(sig_foe=sig_foe.reshape(x.shape), fo=fo, foe_margin=foe_margin)

    cfg = dict(name=name, param=prm, n=c["n"], shape=list(x.shape), dtype=x.dtype.name, snr_dB=c["snr"], linewidth=c["lw"],
               offset=c["fo"], seed=seed, numpy=np.__version__, foe=bool(foe), N=N, B=B, M=M, constType=ct, Ts=Ts,
               P=(M if ct == "psk" else 4))
    out["cfg"] = json.dumps(cfg)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"cpr_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size >> 10} KiB  margin {min_margin:.2e}  unwrap margin {unwrap_margin:.3f}  distinct {distinct}  "
          f"max step {max_step:.3f}" + (f"  fo {out['fo']}  peak margin {out['foe_margin']:.2e}" if foe else ""), flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        generate(case)
