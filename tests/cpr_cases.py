"""Shared by the carrier-recovery tests: the fixtures tests/golden/cpr/cpr_*.npz (tools/gen_golden_cpr.py; a directory of their
own because the fibre tests take every tests/golden/*.npz for a propagation case), the bounds the test files hold in common, the
comparison of a result against the reference's recorded arrays, and a chunked numpy restatement of the search in ``bpsGPU``'s
formulation for the sizes no fixture covers."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpr")
CASES = sorted(os.path.basename(p)[len("cpr_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "cpr_*.npz")))
EXPECTED_CASES = ["psk4_foe", "qam16_4modes", "qam16_bps", "qam16_defaults_1d", "qam256_c64", "qam64_foe", "qam64_shaped", "qpsk_b32",
                  "short_window"]
RAW_ABS = 1e-12     # raw test phases [rad]: grid values, the fixtures' conditions rule out a flipped decision
PHASE_ABS = 1e-9    # unwrapped phases [rad]
REL = 1e-9          # sigOut, fourthPowerFOE output: rel-L2 and per element against max |ref| (metrics_cases.REL, the project's bound
#                     for double-precision receiver functions against reference fixtures)
FO_REL = 1e-12      # frequency offsets


class Param:
    """Stand-in for the reference's parameters object: attributes only."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"cpr_{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def param(g, **extra):
    return Param(**dict(g["cfg"]["param"], **extra))


def check_conditions(g):
    """The fixture cannot make a test pass emptily (asserted by the generator, re-checked on the stored values)."""
    cfg = g["cfg"]
    assert float(g["min_margin"]) >= 1e-7
    assert float(g["unwrap_margin"]) >= 1e-3
    if cfg["name"] != "short_window":
        assert int(g["distinct"]) >= cfg["B"] / 4 and float(g["max_step"]) > np.pi / 4
    if cfg["foe"]:
        assert np.all(g["fo"] != 0) and float(g["foe_margin"]) >= 1e-6


def bps_input(g):
    """What the reference's cpr handed to bps: the input itself, or pnorm of the frequency-compensated signal."""
    if not g["cfg"]["foe"]:
        return g["sigIn"]
    s = g["sig_foe"]
    return s / np.sqrt(np.mean(s * np.conj(s)).real)


def rel_l2(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def compare_signal(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.complex128, (label, got.shape, got.dtype)
    e2, emax = rel_l2(got, want), float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{label}: rel-L2 {e2:.2e}, max element error / max |ref| {emax:.2e}")
    assert e2 <= REL and emax <= REL, (label, e2, emax)


def compare_phases(got, want, bound, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (label, got.shape, got.dtype)
    e = float(np.max(np.abs(got - want)))
    print(f"{label}: max |error| {e:.2e} rad")
    assert e <= bound, (label, e)


def compare_fo(got, want, label):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape)
    e = float(np.max(np.abs(got - want) / np.abs(want)))
    print(f"{label}: fo {got} rel {e:.2e}")
    assert e <= FO_REL, (label, e)


def noisy_qam16(n, modes, snr_dB, step_sigma, seed):
    """16-QAM symbols of unit power with white noise and a Wiener phase walk; also the normalised table (complex64)."""
    import opticommpy_amd as oa
    rng = np.random.default_rng(seed)
    table = oa.grayMapping(16, "qam")
    table = table / np.sqrt(np.mean(np.abs(table) ** 2))
    assert table.dtype == np.complex64
    tx = table.astype(np.complex128)[rng.integers(0, 16, size=(n, modes))]
    noise = (rng.normal(size=(n, modes)) + 1j * rng.normal(size=(n, modes))) * np.sqrt(10 ** (-snr_dB / 10) / 2)
    walk = np.cumsum(rng.normal(size=(n, modes)) * step_sigma, axis=0)
    return (tx + noise) * np.exp(1j * walk), table


def numpy_bps(x, Nh, table, B, chunk=4096):
    """bpsGPU's formulation in numpy, chunked over the symbols: zero padding, minimum distances, a window sum over 2 Nh + 1
    symbols, argmin.  Returns (index, relative margin between the two smallest window sums), both (n, nModes)."""
    n, modes = x.shape
    rot = np.exp(1j * (np.arange(0, B) * (np.pi / 2) / B))
    tab = np.asarray(table).astype(np.complex128)
    W = 2 * Nh + 1
    idx = np.empty((n, modes), dtype=np.int64)
    margin = np.empty((n, modes))
    for m in range(modes):
        xp = np.concatenate((np.zeros(Nh, complex), x[:, m].astype(np.complex128), np.zeros(Nh, complex)))
        for s in range(0, n, chunk):
            seg = xp[s:min(s + chunk, n) + 2 * Nh]
            dmin = np.empty((len(seg), B))
            rows = max(1, (1 << 22) // (B * len(tab)))
            for q in range(0, len(seg), rows):
                r = seg[q:q + rows, None] * rot[None, :]
                dmin[q:q + rows] = np.min(np.abs(r[:, :, None] - tab[None, None, :]) ** 2, axis=2)
            sums = np.lib.stride_tricks.sliding_window_view(dmin, W, axis=0).sum(axis=-1)
            order = np.partition(sums, 1, axis=1)
            idx[s:s + len(sums), m] = np.argmin(sums, axis=1)
            margin[s:s + len(sums), m] = (order[:, 1] - order[:, 0]) / order[:, 0]
    return idx, margin
