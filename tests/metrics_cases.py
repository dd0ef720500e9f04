"""Shared by the link-metrics tests: the fixtures tests/golden/metrics/metrics_*.npz (tools/gen_golden_metrics.py; a directory of
their own because the fibre tests take every tests/golden/*.npz without a known prefix for a propagation case) and the comparison of
a result set against the reference's recorded values, at the bounds the three test files hold in common."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics")
CASES = sorted(os.path.basename(p)[len("metrics_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))
EXPECTED_CASES = ["bpsk_6dB", "pam128", "pam4_12dB", "psk32", "psk8_12dB", "qam1024_1d", "qam16_12dB", "qam16_4modes", "qam16_clip",
                  "qam16_transposed", "qam256_24dB_1d", "qam64_18dB", "qam64_c64", "qam64_shaped", "qpsk_8dB"]
REL = 1e-9          # SNR [dB], GMI, NGMI, MI, EVM against the reference: the project's bound for double-precision receiver functions
EXACT = ("BER", "SER")
CLOSE = ("SNR", "GMI", "NGMI", "MI", "EVM")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"metrics_{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    g["px"] = g.get("px")
    return g


def n_modes(g):
    s = g["rx"].shape
    return 1 if len(s) == 1 else min(s)


def check_conditions(g):
    """The fixture cannot make a test pass emptily (asserted by the generator, re-checked on the stored values)."""
    cfg = g["cfg"]
    assert float(g["min_margin"]) >= 1e-6
    if cfg["clip"]:
        assert int(g["clipped_wrong"]) >= 1 and np.all(g["GMI"] < np.log2(cfg["M"]) - 0.01)
    else:
        assert np.all(g["bit_errors"] >= 20)
    assert np.all(np.isfinite(g["GMI"])) and np.all(np.isfinite(g["MI"]))


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def compare(got, g, suffix="", label=""):
    """got: dict name -> array per mode (any subset of the seven names and 'EVM_blind'); g: fixture."""
    for name, val in got.items():
        want = g[name + suffix]
        val = np.asarray(val)
        assert val.shape == want.shape, (label, name, val.shape, want.shape)
        if name in EXACT:
            print(f"{label} {name}{suffix}: {val} (reference {want})")
            assert np.array_equal(val, want), (label, name, val, want)
        else:
            e = rel_err(val, want)
            print(f"{label} {name}{suffix}: rel {e:.2e}")
            assert e <= REL, (label, name, e, val, want)


def demod_input(g):
    """The 1-D sequence whose hard decisions the fixture stores in 'bits'."""
    rx = g["rx"]
    first = rx if rx.ndim == 1 else (rx[0] if rx.shape[1] > rx.shape[0] else rx[:, 0])
    re, im = g["cfg"]["demod_scale"]
    if np.iscomplexobj(rx):
        return np.ascontiguousarray(first.astype(np.complex128) * complex(re, im))
    return np.ascontiguousarray(first.astype(np.float64) * re)
