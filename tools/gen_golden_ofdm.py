#!/usr/bin/env python3
"""Generate the OFDM fixtures tests/golden/ofdm/*.npz by IMPORTING THE REFERENCE's optic/comm/ofdm.py.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  The module is loaded from its file: it needs numpy and scipy only, so no stub is registered.

``<case>.npz``:
    symb        complex128 data symbols, a whole number of frames
    tx          the reference's modulateOFDM(symb, param): complex64
    rx          complex128, one sample per symbol: sqrt(SpS) tx[::SpS] through the FIR channel [1, 0.2 + 0.1j, 0.05] (np.convolve,
                cut to the signal's length).  The other taps sum to 0.274 in magnitude, so every pilot's phase stays within
                asin 0.274 = 0.28 rad of zero; sqrt(SpS) keeps the pilots' magnitude at the channel's (without it the decimated
                signal's carriers are 1 / sqrt(SpS) of the transmitted ones)
    dem128, H128   the reference's demodulateOFDM(rx.copy(), param) with returnChannel: complex128 (H128 is [0j] without pilots)
    dem64, H64     the same for rx.astype(complex64): dem64 complex64, H64 complex128
    dist_mod    max |tx - restatement| / max |restatement|, the restatement (tests/ofdm_restatement.py) in double, not rounded
    dist_dem64, dist_H64   max |dem64 - dem128| / max |dem128|, and the same for H
    cfg         JSON: the parameters, frames, seed, numpy and scipy versions

Conditions asserted here and re-asserted by tests/ofdm_cases.py:check_conditions: with pilots every frame's |angle(H_est)| <= 0.5
and |H_est| >= 0.5 at every pilot; the data are not constant.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ofdm.py [case ...]
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(HERE, "..", "..", "reference"))
OUT = os.path.join(HERE, "..", "tests", "golden", "ofdm")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py
CHANNEL = np.array([1, 0.2 + 0.1j, 0.05])


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load(os.path.join(REFERENCE, "optic", "comm", "ofdm.py"), "reference_ofdm")
rs = _load(os.path.join(HERE, "..", "tests", "ofdm_restatement.py"), "ofdm_restatement")

# pilot None: the notebook's 0.52 (max Re + j max Im) of the constellation
CASES = {
    # the notebook's first cell
    "nb_pilots": dict(Nfft=256, G=4, SpS=2, hermitSymmetry=False, pilotCarriers=[0, 85, 170, 255], nullCarriers=[128], frames=6, seed=1),
    # the same with Hermitian symmetry and no null: Ns = 127, so the four pilots are linspace(0, 126, 4)
    "nb_hermit": dict(Nfft=256, G=4, SpS=2, hermitSymmetry=True, pilotCarriers=[0, 42, 84, 126], nullCarriers=[], frames=6, seed=2),
    # the notebook's second cell
    "nb_nopilot": dict(Nfft=256, G=0, SpS=1, hermitSymmetry=False, pilotCarriers=[], nullCarriers=[128], frames=6, seed=3),
    "n512_sps4": dict(Nfft=512, G=16, SpS=4, hermitSymmetry=False, pilotCarriers=[3, 70, 140, 210, 280, 350, 420, 500], nullCarriers=[256],
                      frames=3, seed=4),
    "n250_sps2": dict(Nfft=250, G=8, SpS=2, hermitSymmetry=False, pilotCarriers=[0, 60, 125, 190, 249], nullCarriers=[124], frames=4, seed=5),
    # odd Nfft: the reference's fftshift pair is one carrier apart there, so a pilot would land on data -- no pilots
    "n255_sps3": dict(Nfft=255, G=5, SpS=3, hermitSymmetry=False, pilotCarriers=[], nullCarriers=[10, 100], frames=4, seed=6),
    "unsorted": dict(Nfft=256, G=4, SpS=2, hermitSymmetry=False, pilotCarriers=[200, 3, 90], nullCarriers=[128], frames=5, seed=7),
    "one_frame": dict(Nfft=64, G=4, SpS=2, hermitSymmetry=False, pilotCarriers=[5, 30, 60], nullCarriers=[32], frames=1, seed=8),
}


class Param:
    pass


def param_of(c, pilot, **kw):
    p = Param()
    for k in ("Nfft", "G", "SpS", "hermitSymmetry"):
        setattr(p, k, c[k])
    p.pilot = pilot
    p.pilotCarriers = np.array(c["pilotCarriers"], dtype=np.int64)
    p.nullCarriers = np.array(c["nullCarriers"], dtype=np.int64)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def qam64(rng, n):
    lv = np.arange(-7, 8, 2)
    return (rng.choice(lv, n) + 1j * rng.choice(lv, n)) / np.sqrt(42.0)


def generate(name):
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    Ns, data = rs.layout(c["Nfft"], c["hermitSymmetry"], c["pilotCarriers"], c["nullCarriers"])
    symb = qam64(rng, c["frames"] * len(data))
    pilot = complex(0.52 * (7 + 7j) / np.sqrt(42.0))
    kw = dict(Nfft=c["Nfft"], G=c["G"], hermitSymmetry=c["hermitSymmetry"], pilot=pilot, SpS=c["SpS"], pilotCarriers=c["pilotCarriers"],
              nullCarriers=c["nullCarriers"])
    tx = ref.modulateOFDM(symb.copy(), param_of(c, pilot))
    assert tx.dtype == np.complex64
    mine = rs.modulate(symb, **kw)
    dist_mod = float(np.max(np.abs(tx - mine)) / np.max(np.abs(mine)))
    rx = np.convolve(np.sqrt(c["SpS"]) * tx[::c["SpS"]].astype(np.complex128), CHANNEL)[:len(tx) // c["SpS"]]
    dem128, H128 = ref.demodulateOFDM(rx.copy(), param_of(c, pilot, returnChannel=True))
    dem64, H64 = ref.demodulateOFDM(rx.astype(np.complex64), param_of(c, pilot, returnChannel=True))
    assert dem128.dtype == np.complex128 and dem64.dtype == np.complex64
    H128, H64 = np.atleast_1d(np.asarray(H128, dtype=np.complex128)), np.atleast_1d(np.asarray(H64, dtype=np.complex128))
    dist_dem64 = float(np.max(np.abs(dem64 - dem128)) / np.max(np.abs(dem128)))
    dist_H64 = float(np.max(np.abs(H64 - H128)) / np.max(np.abs(H128))) if c["pilotCarriers"] else 0.0
    # the conditions
    assert len(np.unique(symb)) > 8
    if c["pilotCarriers"]:
        F = c["frames"]
        Y = np.array([np.fft.fftshift(np.fft.fft(fr[c["G"]:])) / np.sqrt(c["Nfft"]) for fr in rx.reshape(F, -1)])
        if c["hermitSymmetry"]:
            Y = Y[:, 1:1 + Ns]
        est = Y[:, c["pilotCarriers"]] / pilot
        assert np.max(np.abs(np.angle(est))) <= 0.5 and np.min(np.abs(est)) >= 0.5, (name, np.max(np.abs(np.angle(est))), np.min(np.abs(est)))
    cfg = dict(name=name, Nfft=c["Nfft"], G=c["G"], SpS=c["SpS"], hermitSymmetry=c["hermitSymmetry"], pilot=[pilot.real, pilot.imag],
               pilotCarriers=c["pilotCarriers"], nullCarriers=c["nullCarriers"], frames=c["frames"], seed=c["seed"], M=64,
               channel=[[z.real, z.imag] for z in CHANNEL], numpy=np.__version__, scipy=scipy.__version__)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, symb=symb, tx=tx, rx=rx, dem128=dem128, H128=H128, dem64=dem64, H64=H64, dist_mod=np.float64(dist_mod),
                        dist_dem64=np.float64(dist_dem64), dist_H64=np.float64(dist_H64), cfg=json.dumps(cfg))
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes, dist_mod {dist_mod:.2e}, dist_dem64 {dist_dem64:.2e}, dist_H64 {dist_H64:.2e}")


if __name__ == "__main__":
    for n in (sys.argv[1:] or CASES):
        generate(n)
