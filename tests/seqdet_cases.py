"""Shared by the mlse / detector / whitening-filter tests: the fixtures tests/golden/seqdet/*.npz (tools/gen_golden_seqdet.py), the
bounds, the host emulator (tests/emu/emu_seqdet.cpp) and the shape rows that are checked against the restatement
(tests/seqdet_restatement.py).

Bounds: mlse's output and detector's decided / indDec equal the reference's (np.array_equal); the final path metric within 1e-9
relative of the restatement's; autocorr within 1e-9 of r[0]; the whitening filter within 1e-9 of max |w|.  1e-9 is the project's
own TOL.  Exact equality of decisions is a fair demand because every fixture and every row keeps its candidates at least
1e-9 (1 + best) apart (detector: 1e-6) or exactly equal: a double-precision walk is 1e-16-close to the extended-precision one.

T is the survivor chunk and C the staging chunk of y, read from the package so that the rows follow the build."""
import functools
import json
import os
import subprocess

import numpy as np

import seqdet_restatement as rs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seqdet")
MLSE_CASES = ("pam4_L3", "pam4_L4", "pam4_L0", "pam4_L1", "pam8_L2", "pam2_L10", "pam4_ties", "qpsk_L2", "qpsk_ties", "pam4_f32")
DET_CASES = ("qam16_ml", "qam16_map_uniform", "qam4_map_px", "pam4_ml_real", "two_point_map")
WHITE_CASES = ("white_2", "white_5", "white_16")
TOL, GAP, DET_GAP = 1e-9, 1e-9, 1e-6


def _chunks():
    from opticommpy_amd import seqdet
    return seqdet.T, seqdet.CHUNK


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def check_conditions(g):
    """What tools/gen_golden_seqdet.py asserted, once more, from the values the file holds."""
    cfg = g["cfg"]
    if cfg["kind"] == "mlse":
        assert float(g["gap"]) >= GAP and float(g["final_gap"]) >= GAP, cfg["name"]
        assert (int(g["ties"]) > 0) == cfg["ties"], cfg["name"]
        assert np.array_equal(g["c"][g["index"]].astype(g["y"].dtype), g["out"]) and g["out"].dtype == g["y"].dtype
        differ = float(np.mean(g["det"] != g["index"]))
        if cfg["L"] > 0 and cfg["open_eye"]:
            assert differ > 0, cfg["name"]
        elif cfg["L"] > 0:
            assert np.any(g["index"] != g["tx"]) and differ >= 0.1, cfg["name"]
    elif cfg["kind"] == "detector":
        assert float(g["gap"]) >= DET_GAP and g["ind"].dtype == np.int64 and len(g["r"]) <= 2000
    else:
        assert float(g["kmax"]) < 0.95 and g["r"].shape == g["w"].shape == (cfg["nTaps"],)


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


# ---- the host emulator
def build_emu(exe, flags=("-O2",)):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(root, "opticommpy_amd", "csrc"), os.path.join(root, "tests", "emu", "emu_seqdet.cpp"), "-o", str(exe)])
    return str(exe)


def _run(exe, tmp, head, sigma2, arrays):
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array(head, dtype=np.int64).tobytes())
        f.write(np.float64(sigma2).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a).view(np.float64).tobytes())
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")])
    return np.fromfile(tmp / "out.bin", dtype=np.float64)


def emu_mlse(exe, tmp, y, h, c, reps=1):
    """The emulator on a call as the package would hand it to the library: (out, final metrics, info)."""
    from opticommpy_amd import seqdet
    q = seqdet._prepare_mlse(np.asarray(y), h, c)
    wide = np.complex128 if q["cx"] else np.float64
    raw = _run(exe, tmp, [0, q["N"], q["cols"], int(q["cx"]), q["M"], q["taps"], 0, 0, reps], 0.0, [q["h"], q["c"], np.asarray(y).astype(wide)])
    n = q["N"] * q["cols"] * (2 if q["cx"] else 1)
    out = raw[:n].view(wide).reshape(np.asarray(y).shape).astype(q["out_dtype"])
    info = raw[n + q["cols"]:]
    return out, raw[n:n + q["cols"]].copy(), dict(states=int(info[0]), kernel=int(info[1]), chunk=int(info[2]), survivor_bytes=int(info[3]),
                                                 seconds=float(info[4]))


def emu_detector(exe, tmp, r, sigma2, c, px=None, rule="MAP"):
    from opticommpy_amd import seqdet
    q = seqdet._prepare_detector(np.asarray(r), sigma2, c, px, rule)
    wide = np.complex128 if q["cx"] else np.float64
    flat = np.asarray(r).astype(wide).reshape(-1)
    raw = _run(exe, tmp, [1, flat.size, 1, int(q["cx"]), q["M"], 0, q["rule"], 0, 1], q["sigma2"], [q["c"], q["logpx"], flat])
    n = flat.size * (2 if q["cx"] else 1)
    decided = raw[:n].view(wide)
    decided = decided.real if q["widen"] else decided
    return decided.astype(q["out_dtype"]).reshape(np.asarray(r).shape), raw[n:].astype(np.int64).reshape(np.asarray(r).shape)


def emu_autocorr(exe, tmp, x, nTaps):
    x = np.asarray(x, dtype=np.float64)
    return _run(exe, tmp, [2, x.size, 1, 0, 0, 0, 0, nTaps, 1], 0.0, [x])


# ---- synthetic inputs for the shape rows
def pam_table(M):
    t = np.arange(-(M - 1), M, 2).astype(np.float64)
    return t / np.sqrt(np.mean(t ** 2))


def qam_table(M):
    side = int(np.sqrt(M))
    lv = np.arange(-(side - 1), side, 2)
    t = (lv[None, :] + 1j * lv[:, None]).reshape(-1).astype(np.complex128)
    return t / np.sqrt(np.mean(np.abs(t) ** 2))


_TAPS = np.array([1, .61, .29, .13, .083, .061, .047, .037, .029, .019, .011])       # (no two sums of taps times levels coincide)


def response(L, cx):
    h = _TAPS[:L + 1].astype(np.complex128 if cx else np.float64)
    return h * np.exp(0.4j * np.arange(L + 1)) if cx else h


def _n(expr):
    T, C = _chunks()
    return expr if isinstance(expr, int) else eval(expr, dict(T=T, C=C))


# mlse rows: id -> M, L, N (an integer or an expression in T and C), columns, complex, tail (the final state forced: 'last' | 'zero')
def _row(M, L, N="2 * T + 1", cols=1, cx=False, tail=None):
    return dict(M=M, L=L, N=N, cols=cols, cx=cx, tail=tail)


MLSE_ROWS = {
    # states 1, 2, 3, 4, 9, 16, 64 (one wavefront), 128, 256, 1024 (several); M = 2, 3, 4, 8, 16, 64
    "s1_m4": _row(4, 0), "s1_m1": _row(1, 3), "s2": _row(2, 1), "s3": _row(3, 1), "s4_m4": _row(4, 1), "s4_m2": _row(2, 2),
    "s9": _row(3, 2), "s16_m4": _row(4, 2), "s16_m16": _row(16, 1, cx=True), "s64_m4": _row(4, 3), "s64_m8": _row(8, 2),
    "s64_m64": _row(64, 1, cx=True), "s64_m2": _row(2, 6), "s128": _row(2, 7), "s256_m4": _row(4, 4), "s256_m16": _row(16, 2, cx=True),
    "s1024_m2": _row(2, 10), "s1024_m4": _row(4, 5), "s64_m64_L0": _row(64, 0, cx=True),
    # N = 1, 2, L, L + 1 (fewer symbols than the memory), T - 1, T, T + 1, 2 T + 1, C - 1, C, C + 1
    "n1": _row(4, 3, 1), "n2": _row(4, 3, 2), "nL": _row(4, 3, 3), "nL1": _row(4, 3, 4), "nTm1": _row(4, 3, "T - 1"), "nT": _row(4, 3, "T"),
    "nT1": _row(4, 3, "T + 1"), "nCm1": _row(4, 3, "C - 1"), "nC": _row(4, 3, "C"), "nC1": _row(4, 3, "C + 1"),
    "n1_256": _row(4, 4, 1), "nL_256": _row(4, 4, 4), "nT_256": _row(4, 4, "T"), "nT1_256": _row(4, 4, "T + 1"), "nC1_256": _row(4, 4, "C + 1"),
    "nC1_cx": _row(4, 2, "C + 1", cx=True), "nC_1024": _row(2, 10, "C"),
    # columns
    "c2": _row(4, 2, 70, cols=2), "c3": _row(4, 2, 70, cols=3), "c3_cx": _row(4, 2, 70, cols=3, cx=True), "c2_256": _row(4, 4, 40, cols=2),
    # the final state is the last state / state 0
    "fin_last": _row(4, 3, tail="last"), "fin_zero": _row(4, 3, tail="zero"), "fin_last_256": _row(4, 4, tail="last"),
}
MLSE_ROW_IDS = list(MLSE_ROWS)


@functools.lru_cache(maxsize=None)
def mlse_row(rid):
    """(y, h, c, restatement per column) of a row; the seed is kept only if every column meets the gap condition."""
    r = MLSE_ROWS[rid]
    M, L, cols, cx, N = r["M"], r["L"], r["cols"], r["cx"], _n(r["N"])
    c = qam_table(M) if cx and M > 1 else pam_table(M) if M > 1 else np.array([1.0])
    c = c.astype(np.complex128) if cx else c
    h = response(L, cx)
    step = abs(c[1] - c[0]) if M > 1 else 1.0
    base = sum(map(ord, rid)) * 100
    for seed in range(base, base + 50):
        rng = np.random.default_rng(seed)
        tx = rng.integers(0, M, size=(N, cols))
        if r["tail"]:
            tx[max(0, N - L - 2):] = M - 1 if r["tail"] == "last" else 0
        sigma = (0.05 if r["tail"] else 0.3) * step
        y = np.stack([np.convolve(c[tx[:, k]], h)[:N] for k in range(cols)], axis=1)
        y = y + sigma * ((rng.normal(size=y.shape) + 1j * rng.normal(size=y.shape)) if cx else rng.normal(size=y.shape))
        want = [rs.mlse(y[:, k], h, c) for k in range(cols)]
        if all(w["gap"] >= GAP and w["final_gap"] >= GAP and w["ties"] == 0 for w in want):
            break
    else:
        raise AssertionError(f"{rid}: no seed meets the gap condition")
    for a in (y, h, c):
        a.setflags(write=False)
    return (y[:, 0] if cols == 1 else y), h, c, want


def expected_kernel(states):
    return "forward_wave64" if states <= 64 else "forward_multiwave"


# detector rows: id -> n, M, complex, rule, priors ('random' | 'zero': one prior is zero | None)
DET_ROWS = {
    "n1": (1, 4, False, "ML", None), "n63": (63, 2, False, "MAP", "random"), "n64": (64, 3, False, "ML", None),
    "n65": (65, 8, False, "MAP", "random"), "share_p1": ("B + 1", 16, True, "MAP", "random"), "m64": (300, 64, True, "ML", None),
    "m64_map": (300, 64, True, "MAP", "zero"), "m1": (10, 1, False, "MAP", None), "two_d": ((33, 3), 4, True, "MAP", None),
}
DET_ROW_IDS = list(DET_ROWS)


@functools.lru_cache(maxsize=None)
def det_row(rid):
    """(r, sigma2, c, px, rule, expected indices)."""
    from opticommpy_amd import _lib
    n, M, cx, rule, prior = DET_ROWS[rid]
    shape = (eval(n, dict(B=_lib.SEQDET_DET_BLOCK)),) if isinstance(n, str) else n if isinstance(n, tuple) else (n,)
    c = qam_table(M) if cx else pam_table(M) if M > 1 else np.array([1.0])
    step = abs(c[1] - c[0]) if M > 1 else 1.0
    base = sum(map(ord, rid)) * 100 + 7
    for seed in range(base, base + 50):
        rng = np.random.default_rng(seed)
        px = None
        if prior:
            px = rng.uniform(0.2, 1.0, size=M)
            if prior == "zero":
                px[M // 3] = 0.0
            px = px / px.sum()
        sigma = 0.45 * step
        r = c[rng.integers(0, M, size=shape)] + sigma * ((rng.normal(size=shape) + 1j * rng.normal(size=shape)) if cx else rng.normal(size=shape))
        want, gap = rs.detector(r, sigma ** 2, c, px, rule)
        if gap >= DET_GAP:
            break
    else:
        raise AssertionError(f"{rid}: no seed meets the gap condition")
    r.setflags(write=False)
    return r, sigma ** 2, c, px, rule, want.reshape(shape)


# autocorr rows: (N, nTaps) with N an integer or an expression in the tile (a workgroup's share is whole tiles)
AC_ROWS = [(1, 1), (2, 1), (2, 2), (3, 2), (64, 64), (65, 64), (65, 65), (66, 65), (256, 256), (257, 256), ("TILE - 1", 5), ("TILE", 64),
           ("TILE + 1", 256), ("2 * TILE + 5", 16)]
AC_ROW_IDS = [f"{n}-{k}".replace(" ", "") for n, k in AC_ROWS]


@functools.lru_cache(maxsize=None)
def ac_row(i):
    from opticommpy_amd import _lib
    n, nTaps = AC_ROWS[i]
    n = eval(n, dict(TILE=_lib.SEQDET_AC_TILE)) if isinstance(n, str) else n
    return coloured(n, 300 + i), nTaps


def coloured(n, seed):
    """AR(2)-coloured real noise."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=n + 50)
    x = np.zeros(n + 50)
    for i in range(2, n + 50):
        x[i] = e[i] + 1.0 * x[i - 1] - 0.6 * x[i - 2]
    x = x[50:].copy()
    x.setflags(write=False)
    return x


def check_autocorr(got, x, nTaps, what):
    want = rs.autocorr(x, nTaps)
    assert got.dtype == np.float64 and got.shape == (nTaps,), what
    d = float(np.max(np.abs(got - want)) / abs(want[0]))
    print(f"{what}: autocorr within {d:.2e} of r[0]")
    assert d <= TOL, (what, d)
    return d
