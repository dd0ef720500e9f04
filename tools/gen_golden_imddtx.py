#!/usr/bin/env python3
"""Generate the IM/DD transmitter and AWGN fixtures tests/golden/imddtx/*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository); never
on the GPU box.  As tools/gen_golden_siso.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity), and one for
``tqdm.notebook`` if that is missing.  The reference's noise generators are ``@njit``: with the stub their draws are numpy's, and
those draws are the definition the fixtures hold.  No bytecode is written.  Data only; every file stays under MAX_BYTES.

Files (every one carries cfg, a JSON string with the parameters set and the numpy version):
    pam_<row>      symbTx, sigTxo as pamTransmitter returns them, pulse (the taps), peak_margin (second largest |shaped sample| over
                   the largest, per mode, read off tests/imddtx_restatement.py), written (the parameter object after the call);
                   pam_rrc also holds ipd, the ideal photodiode's current of sigTxo
    mod_<row>      u, Ei (an array, or one value for a scalar), out of pm / mzm / iqm
    awgn_<row>     sig, out, zr and zi: the unit normals of the same stream (np.random.standard_normal in the reference's draw order),
                   sigma2, global_seed (np.random.seed before the call; the parameter's own seed is in cfg)
    sources        bits of bitSource in both modes (PRBS orders 7 and 23), prbsGenerator, symbolSource rows, upsample rows
    cell_ook       the notebook cell bitSource -> modulateGray -> upsample -> firFilter -> mzm -> linearFiberChannel -> photodiode
                   (ideal), every intermediate array

Conditions asserted here and re-asserted by tests/imddtx_cases.py:check_conditions, so that no fixture lets a test pass emptily:
the ER = 10 output differs from the ER = 80 output by more than 1e-3 of its peak; the awgn noise power is within 10 % of sigma2;
the peak of every shaped signal is unique by a relative margin of at least 1e-9 -- as a value: an NRZ pulse under three equal outer
symbols in a row is a flat top, whose samples are the same number to rounding (within 1e-12) and count as one peak.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_imddtx.py
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

import optic.comm.sources as ref_src  # noqa: E402
import optic.dsp.core as ref_core  # noqa: E402
import optic.models.channels as ref_ch  # noqa: E402
import optic.models.devices as ref_dev  # noqa: E402
import optic.models.tx as ref_tx  # noqa: E402
from optic.comm.modulation import modulateGray as ref_modulate  # noqa: E402
from optic.utils import parameters as ref_parameters  # noqa: E402

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[1:1] = [os.path.join(_ROOT, "tests")]
import imddtx_restatement as ir  # noqa: E402

OUT = os.path.join(_ROOT, "tests", "golden", "imddtx")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py

# pamTransmitter: name -> what is set on the parameter object
PAM = {
    "default": dict(nBits=2048, seed=11),
    "rrc": dict(nBits=256, seed=12, pulseType="rrc", nFilterTaps=256, SpS=16),
    "pam2": dict(nBits=128, seed=13, M=2),
    "pam8": dict(nBits=384, seed=14, M=8),
    "sps1": dict(nBits=512, seed=15, SpS=1),
    "sps3": dict(nBits=512, seed=16, SpS=3),
    "sps16": dict(nBits=256, seed=17, SpS=16),
    "pol2": dict(nBits=256, seed=18, nPolModes=2),
    "mb": dict(nBits=510, seed=19, M=8, SpS=4, probDist="maxwell-boltzmann", shapingFactor=0.08),
    "mzm": dict(nBits=256, seed=20, mzmER=10, mzmVb=0.7, mzmScale=0.9),
    "retparam": dict(nBits=256, seed=21, SpS=8, returnParam=True, power=2),
}


def make_param(d):
    p = ref_parameters()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def cfg_json(kind, d, **extra):
    return np.array(json.dumps(dict(kind=kind, param=d, numpy=np.__version__, **extra)))


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size} bytes")


def peak_margin(symbols, taps, SpS):
    return ir.peak_margin(ir.shaped(symbols, taps, SpS))


def gen_pam():
    for name, d in PAM.items():
        p = make_param(d)
        res = ref_tx.pamTransmitter(p)
        sig, symb = res[0], res[1]
        assert (len(res) == 3) == bool(d.get("returnParam", False))
        pp = ref_parameters()
        pp.pulseType, pp.nFilterTaps, pp.rollOff, pp.SpS = p.pulseType, p.nFilterTaps, p.pulseRollOff, p.SpS
        pulse = ref_core.pulseShape(pp)
        margins = [peak_margin(symb[:, m], pulse, p.SpS) for m in range(p.nPolModes)]
        assert min(margins) >= 1e-9, (name, margins)
        written = {k: (v if not isinstance(v, (np.integer, np.floating)) else v.item()) for k, v in vars(p).items()}
        extra = {}
        if name == "rrc":
            pd = ref_parameters()
            pd.ideal = True
            extra["ipd"] = ref_dev.photodiode(sig, pd)
        save("pam_" + name, symbTx=symb, sigTxo=sig, pulse=pulse, peak_margin=np.array(margins), written=np.array(json.dumps(written)),
             cfg=cfg_json("pam", d), **extra)
    a, b = ref_tx.pamTransmitter(make_param(dict(PAM["mzm"], mzmER=10)))[0], ref_tx.pamTransmitter(make_param(dict(PAM["mzm"], mzmER=80)))[0]
    assert np.max(np.abs(a - b)) > 1e-3 * np.max(np.abs(b))


def gen_mod():
    rng = np.random.default_rng(2024)
    n = 1000
    ur = rng.uniform(-20, 20, n)                          # in units of Vpi, scaled per row
    uc = ur + 1j * rng.uniform(-0.2, 0.2, n)              # a complex drive: the imaginary part sets the modulus, keep it moderate
    ei = np.sqrt(rng.uniform(0.5, 2, n)) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    rows = {
        "mzm_default": ("mzm", 1.0, ur * 2, {}),
        "mzm_er10": ("mzm", 1.0, ur * 3, dict(Vpi=3, Vb=-1.5, ER=10)),
        "mzm_er80_array": ("mzm", ei, ur * 3, dict(Vpi=3, Vb=0.4, ER=80)),
        "mzm_complex_drive": ("mzm", ei, uc * 2, dict(Vpi=2, Vb=-0.3, ER=60)),
        "mzm_complex_scalar": ("mzm", 0.5 - 0.25j, uc * 2, dict(Vpi=2, Vb=-1, ER=10)),
        "pm_scalar": ("pm", 1.0, ur * 2.5, dict(Vpi=2.5)),
        "pm_array_complex": ("pm", ei, uc * 2.5, dict(Vpi=2.5)),
        "iqm_default": ("iqm", 1.0, (ur + 1j * ur[::-1]) * 0.1, {}),
        "iqm_biased": ("iqm", ei, (ur + 1j * ur[::-1]) * 2, dict(Vpi=2, VbI=-1.7, VbQ=-2.2, Vphi=0.9, ERI=10, ERQ=80)),
        "iqm_real_drive": ("iqm", 1.0, ur * 2, dict(Vpi=2, VbI=-2, VbQ=-2, Vphi=1, ERI=60, ERQ=60)),
        "mzm_2d": ("mzm", ei.reshape(-1, 2), (ur * 2).reshape(-1, 2), dict(Vpi=2, Vb=-1, ER=60)),
    }
    for name, (kind, Ei, u, d) in rows.items():
        if kind == "pm":
            out = ref_dev.pm(Ei, u, d["Vpi"])
        else:
            out = getattr(ref_dev, kind)(Ei, u, make_param(d) if d else None)
        assert out.shape == u.shape and np.all(np.isfinite(out))
        save("mod_" + name, u=u, Ei=np.asarray(Ei), out=out, cfg=cfg_json(kind, d))
    a = ref_dev.mzm(1.0, ur * 3, make_param(dict(Vpi=3, Vb=-1.5, ER=10)))
    b = ref_dev.mzm(1.0, ur * 3, make_param(dict(Vpi=3, Vb=-1.5, ER=80)))
    assert np.max(np.abs(a - b)) > 1e-3 * np.max(np.abs(b))


def gen_awgn():
    rng = np.random.default_rng(77)
    n = 1200
    cx1 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    cx2 = (rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))) * np.array([1.0, 0.5])
    re1 = rng.standard_normal(n) * 2 + 0.3
    re2 = rng.standard_normal((n, 2))
    rows = {
        "complex_on_complex": (cx1, dict(snr=15, seed=5), None),
        "real_on_complex": (cx1, dict(snr=12, complexNoise=False, seed=6), None),
        "complex_on_real": (re1, dict(snr=10, seed=7), None),
        "real_on_real": (re1, dict(snr=20, complexNoise=False, seed=8), None),
        "two_columns": (cx2, dict(snr=18, Fs=4.0, B=1.5, seed=9), None),
        "two_columns_real": (re2, dict(snr=14, Fs=2.0, B=0.5, complexNoise=False, seed=10), None),
        "defaults_global_stream": (cx1, dict(), 31),
        "real_global_stream": (re2, dict(snr=9, complexNoise=False), 32),
    }
    for name, (sig, d, gseed) in rows.items():
        cplx = d.get("complexNoise", True)
        if gseed is not None:
            np.random.seed(gseed)
        out = ref_ch.awgn(sig, make_param(d))
        state_after = np.random.get_state()[2]
        np.random.seed(gseed if gseed is not None else d["seed"])       # the same stream as unit normals, in the reference's draw order
        zr = np.random.standard_normal(sig.shape)
        zi = np.random.standard_normal(sig.shape) if cplx else np.zeros(0)
        assert np.random.get_state()[2] == state_after
        sigma2 = (d.get("Fs", 1) / d.get("B", 1)) * (np.mean(np.abs(sig) ** 2) / 10 ** (d.get("snr", 20) / 10))     # channels.py:556-558
        s = np.sqrt(sigma2 / 2)
        assert np.array_equal(out, sig + (s * zr + 1j * (s * zi) if cplx else s * zr))          # normal(0, s) is s * standard_normal
        pn = np.mean(np.abs(out - sig) ** 2)
        want = sigma2 if cplx else sigma2 / 2
        assert abs(pn / want - 1) <= 0.1, (name, pn, want)
        assert out.dtype == (np.complex128 if (cplx or np.iscomplexobj(sig)) else np.float64)
        save("awgn_" + name, sig=sig, out=out, zr=zr, zi=zi, sigma2=np.array(sigma2), global_seed=np.array(-1 if gseed is None else gseed),
             cfg=cfg_json("awgn", d))


def gen_sources():
    arrays = {}
    rows = {"bits_random": dict(nBits=777, seed=3), "bits_random_default": dict(seed=4),
            "bits_prbs7": dict(nBits=400, mode="prbs", order=7), "bits_prbs23": dict(nBits=3000, mode="prbs", order=23, seed=5),
            "bits_prbs_default_order": dict(nBits=300, mode="prbs")}
    for name, d in rows.items():
        arrays[name] = ref_src.bitSource(make_param(d))
    arrays["prbs7_full"] = ref_src.prbsGenerator(7, None, 1)
    arrays["prbs23_head"] = ref_src.prbsGenerator(23, 2500, 9)
    srows = {"symb_qam16": dict(nSymbols=500, M=16, seed=6), "symb_pam4": dict(nSymbols=500, M=4, constType="pam", seed=7),
             "symb_psk8": dict(nSymbols=300, M=8, constType="psk", seed=8),
             "symb_mb": dict(nSymbols=500, M=16, dist="maxwell-boltzmann", shapingFactor=0.05, seed=9),
             "symb_px": dict(nSymbols=400, M=4, constType="pam", px=[0.1, 0.4, 0.4, 0.1], seed=10)}
    for name, d in srows.items():
        arrays[name] = ref_src.symbolSource(make_param(d))
    rng = np.random.default_rng(5)
    ups = {"up_f64_3": (rng.standard_normal(101), 3), "up_c128_4": (rng.standard_normal(77) + 1j * rng.standard_normal(77), 4),
           "up_c64_2": ((rng.standard_normal(50) + 1j * rng.standard_normal(50)).astype(np.complex64), 2),
           "up_2d_5": (rng.standard_normal((40, 3)) + 1j * rng.standard_normal((40, 3)), 5), "up_f64_1": (rng.standard_normal(33), 1)}
    for name, (x, f) in ups.items():
        arrays[name + "_in"] = x
        arrays[name] = ref_core.upsample(x, f)
    rows_json = dict(bits=rows, symbols=srows, upsample={k: v[1] for k, v in ups.items()})
    save("sources", cfg=np.array(json.dumps(dict(kind="sources", rows=rows_json, numpy=np.__version__))), **arrays)


def gen_cell():
    SpS, M, Rs = 8, 2, 10e9
    Fs = SpS * Rs
    bits = ref_src.bitSource(make_param(dict(nBits=256, mode="random", seed=123)))
    # the reference keeps its Gray table in single precision, so its PAM symbols are float32 and the whole cell would run in single
    # precision; PAM-2's -1 and +1 are exact, and widening them to what this package's modulateGray returns makes the cell double
    symb = ref_modulate(bits, M, "pam").astype(np.complex128)
    up = ref_core.upsample(symb, SpS)
    pulse = ref_core.pulseShape(make_param(dict(pulseType="nrz", SpS=SpS)))
    sigTx = ref_core.firFilter(pulse, up)
    Ai = np.sqrt(1e-3 * 10 ** (3 / 10))
    sigTxo = ref_dev.mzm(Ai, sigTx, make_param(dict(Vpi=2, Vb=-1)))
    ch = dict(L=100, alpha=0.2, D=16, Fc=193.1e12, Fs=Fs)
    sigCh = ref_ch.linearFiberChannel(sigTxo, make_param(ch))
    ipd = ref_dev.photodiode(sigCh, make_param(dict(ideal=True)))
    save("cell_ook", bits=bits, symbTx=symb, symbolsUp=up, pulse=pulse, sigTx=sigTx, sigTxo=sigTxo, sigCh=sigCh, ipd=ipd,
         cfg=cfg_json("cell", dict(SpS=SpS, M=M, Rs=Rs, Pi_dBm=3, Vpi=2, Vb=-1, ch=ch)))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    gen_pam()
    gen_mod()
    gen_awgn()
    gen_sources()
    gen_cell()
