"""Shared by the theoretical-MI tests: the fixtures tests/golden/theory/*.npz (tools/gen_golden_theory.py), the shape rows, the
bounds and the host emulator (tests/emu/emu_theory.cpp).

Bounds (none of them read off the device code):
  RULE_BOUND 1e-10   the quadrature rule (h = 0.1, T = 6.5) against h / 2 in long double: profiles/theory_quadrature.json
  REF_FIX    1e-7    reference at tol = 1e-9 against the long-double restatement of the rule, asserted when a fixture is made
  REF_TOL    2e-7    device against the reference at tol = 1e-9: REF_FIX plus RULE_BOUND, rounded up
  RS_TOL     1e-12   device against the restatement: exp / log at a few ulp of values <= 10, against weights that sum to 1
  CALC_TOL   1e-9    calcMI, relative: the project's bound for double-precision receiver functions
  HOST_TOL   1e-14   the host functions, relative: a handful of double operations in the same order"""
import json
import os
import subprocess

import numpy as np

import theory_restatement as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "theory")
RULE_BOUND, REF_FIX, REF_TOL, RS_TOL, CALC_TOL, HOST_TOL = 1e-10, 1e-7, 2e-7, 1e-12, 1e-9, 1e-14
QUIRK = 0.01               # the reference's symmetry=True value for 64-QAM is further than this from the integral over all points

# name -> M, constType, SNR, pX ('mb': Maxwell-Boltzmann), tol of the accurate reference run (None: default only), symmetry flags
MI_CASES = {
    "qpsk_5dB": dict(M=4, constType="qam", SNR=5.0, px=None, tol=1e-9, symmetry=[True]),
    "qam16_10dB": dict(M=16, constType="qam", SNR=10.0, px=None, tol=1e-9, symmetry=[True, False]),
    "psk8_8dB": dict(M=8, constType="psk", SNR=8.0, px=None, tol=1e-9, symmetry=[True]),
    "pam4_10dB": dict(M=4, constType="pam", SNR=10.0, px=None, tol=1e-9, symmetry=[True]),
    "qam16_mb_10dB": dict(M=16, constType="qam", SNR=10.0, px="mb", tol=1e-9, symmetry=[False]),
    "qam64_15dB": dict(M=64, constType="qam", SNR=15.0, px=None, tol=None, symmetry=[True, False]),
}
CALC_CASES = {
    "calc_qam16": dict(M=16, constType="qam", dtype="complex128", shaped=False, SNR=12.0),
    "calc_qam64": dict(M=64, constType="qam", dtype="complex128", shaped=False, SNR=18.0),
    "calc_pam4": dict(M=4, constType="pam", dtype="float64", shaped=False, SNR=10.0),
    "calc_qam64_shaped_c64": dict(M=64, constType="qam", dtype="complex64", shaped=True, SNR=14.0),
}
CALC_N = 4096
CALC_ROWS = (1, 255, 256, 257, 65537)          # one lane, a workgroup less one / exactly / plus one, more than one grid pass


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def maxwell_boltzmann(table, lam=0.6):
    """p_i ~ exp(-lam |x_i|^2) on the unit-energy table, normalised."""
    p = np.exp(-lam * np.abs(np.asarray(table).astype(np.complex128)) ** 2)
    return p / np.sum(p)


# ---- shape rows through constellationMI.  Scattered points: no two coincide, mean power about 1.
def scattered(M, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=M) + 1j * rng.normal(size=M)) / np.sqrt(2)


def six_decades(M):
    p = 10.0 ** (-6.0 * np.arange(M) / (M - 1))
    return p / np.sum(p)


SNR_GRID21 = np.linspace(-10.0, 30.0, 21)
SHAPE_ROWS = [dict(name=f"M{M}", M=M, seed=100 + M, SNR=[8.0], px=None) for M in (1, 2, 3, 63, 64, 65, 257, 1024)]
SHAPE_ROWS += [dict(name=f"nS{n}", M=8, seed=7, SNR=list(np.linspace(-5.0, 27.0, n)) if n > 1 else [6.0], px=None) for n in (1, 2, 65)]
SHAPE_ROWS += [dict(name="px_six_decades", M=16, seed=16, SNR=[9.0], px="six"),
               dict(name="snr_m40", M=16, seed=16, SNR=[-40.0], px=None),
               dict(name="snr_p60", M=16, seed=16, SNR=[60.0], px=None),
               dict(name="grid21", M=16, seed=16, SNR=list(SNR_GRID21), px=None)]
ROW = {r["name"]: r for r in SHAPE_ROWS}
EMU_SUBSET = {"M257": (0, 128, 256), "M1024": (0, 1023)}        # points the host emulator walks where all of them take minutes


def row_input(row):
    """(table, px, sigma[nS]) of a shape row."""
    table = scattered(row["M"], row["seed"])
    px = six_decades(row["M"]) if row["px"] == "six" else np.ones(row["M"]) / row["M"]
    return table, px, rs.sigma_of(np.array(row["SNR"]))


def calc_input(n, seed=5):
    """16-QAM-like symbols with noise for the calcMI rows: (rx, tx, sigma2, table, px)."""
    rng = np.random.default_rng(seed)
    lv = np.array([-3.0, -1.0, 1.0, 3.0]) / np.sqrt(10.0)
    table = (lv[:, None] + 1j * lv[None, :]).reshape(-1)
    tx = table[rng.integers(0, 16, size=n)]
    rx = tx + 0.15 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return rx, tx, 0.045, table, np.ones(16) / 16


# ---- the host emulator
def build_emu(exe, flags=("-O2",)):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(root, "opticommpy_amd", "csrc"),
                           os.path.join(root, "tests", "emu", "emu_theory.cpp"), "-o", str(exe)])
    return str(exe)


def _run(exe, tmp, head, arrays):
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")])
    return np.fromfile(tmp / "out.bin", dtype=np.float64)


def emu_theory(exe, tmp, table, px, sigma, points=None):
    """Without ``points``: MI per sigma.  With them: the bracket px_i (sum_t w log2 S - W log2 px_i) of those points, (nS, len)."""
    table = np.asarray(table).astype(np.complex128).reshape(-1)
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    pts = np.array([] if points is None else points, dtype=np.int64)
    out = _run(exe, tmp, [0, len(table), len(sigma), len(pts)], [table, np.asarray(px, dtype=np.float64), sigma, pts])
    return out if points is None else out.reshape(len(sigma), len(pts))


_CODES = {"complex128": 0, "complex64": 1, "float64": 2, "float32": 3}


def emu_calc_mi(exe, tmp, rx, tx, sigma2, table, px):
    table = np.asarray(table).astype(np.complex128).reshape(-1)
    out = _run(exe, tmp, [1, len(rx), len(table), _CODES[rx.dtype.name]],
               [np.array([sigma2], dtype=np.float64), table, np.asarray(px, dtype=np.float64), rx, tx])
    return out[0]
