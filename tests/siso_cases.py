"""Shared by the ffe / dfe / volterra tests: the fixtures tests/golden/siso/siso_*.npz (tools/gen_golden_siso.py), the bounds the
tests hold the kernels to, and the shape rows that are checked against the restatement (tests/siso_restatement.py).

Bounds (the project's own, tests/test_gpu_eq.py): sigOut and every coefficient array within 1e-9 rel-L2 and each element within
1e-9 of max |ref|; mse within 1e-9 of max |ref|.

`*_default_prec`: prec is left unset, so the normalised input is rounded to single precision and the table is the
single-precision one.  The reference then also runs its recursion in single precision, the device in double: the two differ by
what single-precision arithmetic does to the recursion.  The fixture holds the reference's own distance between its
single-precision run and its double run (self_err, 1.2e-7 .. 2.2e-7); a double recursion on the same rounded input and table can
be no further from the single-precision run than about that, and 2 x self_err is the bound."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "siso")
EXPECTED_CASES = ("ffe_real", "ffe_fulltime", "ffe_preconv3", "ffe_qam", "dfe_real", "dfe_fulltime", "dfe_preconv3", "dfe_qam",
                  "volterra_order2", "volterra_order3", "volterra_order3_fulltime", "volterra_preconv2", "ffe_even_taps_sps3",
                  "dfe_given_coefficients", "volterra_train_all", "ffe_default_prec", "dfe_default_prec", "volterra_default_prec")
TOL = 1e-9


class Param:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"siso_{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def coefficients(g, suffix=""):
    return [g[f"c{i}{suffix}"] for i in range(3) if f"c{i}{suffix}" in g]


def check_conditions(g):
    """What tools/gen_golden_siso.py asserted, once more: the decisions are not ties, and every coefficient section has moved."""
    cfg = g["cfg"]
    assert float(g["gap"]) >= 1e-6 and float(g["change"]) >= 0.1, cfg["name"]
    if cfg["kind"] == "dfe":
        assert float(g["norm_b"]) >= 0.03
    if cfg["kind"] == "volterra":
        assert float(g["norm_h2"]) >= 0.1
        if cfg["param"]["order"] == 3:
            assert float(g["norm_h3"]) >= 0.02
    if cfg["single"]:
        assert 0 < float(g["self_err"]) < 1e-5
    assert g["sigOut"].shape == (cfg["N"],) and g["mse"].shape == (cfg["N"],)


def param(g, double=True):
    """The parameter object of a fixture; double: prec = float64 / complex128 (the run sigOut holds), else prec left unset."""
    cfg = g["cfg"]
    p = Param(**cfg["param"])
    if double:
        p.prec = np.complex128 if cfg["complex"] else np.float64
    if cfg["init"]:
        p.f, p.b = g["i0"].copy(), g["i1"].copy()
    return p


def inputs(g, double=True):
    """(sigIn, symbRef) as the run was given them: the stored arrays, widened for the double run of a single-precision case."""
    wide = np.complex128 if g["cfg"]["complex"] else np.float64
    return (g["sigIn"].astype(wide), g["symbRef"].astype(wide)) if double else (g["sigIn"], g["symbRef"])


def call(mod, kind, sigIn, symbRef, prm):
    """(sigOut, [coefficient arrays], mse) of the package's ffe / dfe / volterra."""
    r = getattr(mod, kind)(sigIn, symbRef, prm)
    if kind == "ffe":
        return r[0], [r[1]], r[2]
    if kind == "dfe":
        return r[0], [r[1], r[2]], r[3]
    return r[0], list(r[1]), r[2]


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def compare(got, want, what, tol=TOL, elementwise_only=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = float(np.max(np.abs(want))) if want.size else 0.0
    if scale == 0.0:
        assert not np.any(got), what
        return 0.0
    d = float(np.max(np.abs(got - want))) / scale
    r = rel_l2(got, want)
    print(f"{what}: rel-L2 {r:.2e}, max element {d:.2e} of max |ref|")
    assert d <= tol and (elementwise_only or r <= tol), (what, r, d)
    return r


def compare_results(got, want, what):
    """got, want: (sigOut, [coefficients], mse)."""
    compare(got[0], want[0], f"{what} sigOut")
    assert len(got[1]) == len(want[1])
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        compare(a, b, f"{what} coefficients {i}")
    compare(got[2], want[2], f"{what} mse", elementwise_only=True)


# ---- the host emulator (tests/emu/emu_siso.cpp)
def build_emu(exe, flags=("-O2",)):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(root, "opticommpy_amd", "csrc"), os.path.join(root, "tests", "emu", "emu_siso.cpp"), "-o", str(exe)])
    return str(exe)


def run_emu(exe, tmp, kind, sigIn, symbRef, prm, reps=1, frozen=True):
    """The emulator on a call as the package would hand it to the library: (sigOut, [coefficients], mse, info) with info =
    dict(serial_symbols, parallel_symbols, R, seconds)."""
    import subprocess
    from opticommpy_amd import sisoeq
    q = sisoeq._prepare(kind, np.asarray(sigIn), np.asarray(symbRef), prm)
    p, cx = q["params"], q["cx"]
    wide = np.complex128 if cx else np.float64
    used = q["parts"] if not (kind == "volterra" and q["order"] == 2) else q["parts"][:2]
    head = np.array([p.n, p.nref, p.nTrain, p.kind, p.mode, int(cx), p.prec32, p.order, p.nTaps, p.nFB, p.n2, p.n3, p.SpS, p.M, p.preconvIters,
                     p.ncoef, int(not frozen), 0, 0, 0], dtype=np.int64)
    with open(tmp / "in.bin", "wb") as f:
        f.write(head.tobytes())
        f.write(np.float64(p.mu).tobytes())
        for a in [q["table"]] + [np.concatenate([u.reshape(-1) for u in used]), np.asarray(q["x"]).astype(wide), np.asarray(q["ref"]).astype(wide)]:
            f.write(np.ascontiguousarray(a).view(np.float64).tobytes())
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin"), str(reps)])
    raw = np.fromfile(tmp / "out.bin", dtype=np.float64)
    w, N = (2 if cx else 1), q["N"]
    sig = raw[:w * N].view(wide)
    flat = raw[w * N:w * (N + p.ncoef)].view(wide)
    coef, at = [], 0
    for a in q["parts"]:
        if at < flat.size:
            coef.append(flat[at:at + a.size].reshape(a.shape).copy())
            at += a.size
        else:
            coef.append(a)
    mse = raw[w * (N + p.ncoef):w * (N + p.ncoef) + N]
    info = raw[-4:]
    return sig.copy(), coef, mse.copy(), dict(serial_symbols=int(info[0]), parallel_symbols=int(info[1]), R=int(info[2]), seconds=float(info[3]))


# ---- synthetic signals for the shape rows
def pam_table(M):
    t = np.arange(-(M - 1), M, 2).astype(np.float64)
    return t / np.sqrt(np.mean(t ** 2))


def qam_table(M):
    side = int(np.sqrt(M))
    lv = np.arange(-(side - 1), side, 2)
    t = (lv[None, :] + 1j * lv[:, None]).reshape(-1).astype(np.complex128)
    return t / np.sqrt(np.mean(np.abs(t) ** 2))


def signal(n, SpS, M, seed, cx=False, nsym=None):
    """n samples (n need not be a multiple of SpS) of a mildly distorted PAM / QAM signal and its symbols."""
    rng = np.random.default_rng(seed)
    nsym = nsym if nsym is not None else (n + SpS - 1) // SpS
    table = qam_table(M) if cx else pam_table(M)
    tx = table[rng.integers(0, M, size=max(nsym, (n + SpS - 1) // SpS))]
    x = np.repeat(tx, SpS)[:n].copy()
    x = x + 0.25 * np.roll(x, 1) - 0.1 * np.roll(x, -1)
    if cx:
        x = x * np.exp(0.2j) + 0.03 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    else:
        x = x + 0.06 * x ** 2 + 0.03 * rng.normal(size=n)
    return x * 0.8, tx[:nsym]


# shape rows: (id, kind, n, parameters).  Chunks of the serial kernel hold 64 symbols, tiles of the frozen kernel 256.
ROWS = [
    # coefficient counts 63, 64, 65, 128 and one above 1024: a slot empty, full, nearly empty
    ("ffe_63", "ffe", 150, dict(nTaps=63, nTrain=100)),
    ("ffe_64", "ffe", 150, dict(nTaps=64, nTrain=100)),
    ("ffe_65", "ffe", 150, dict(nTaps=65, nTrain=100)),
    ("dfe_64_64", "dfe", 200, dict(nTapsFF=64, nTapsFB=64, nTrain=120)),
    ("vol_1091", "volterra", 120, dict(n1Taps=11, n2Taps=9, n3Taps=10, order=3, nTrain=80, mu=5e-3)),        # 11 + 81 + 1000: 18 -> 24 slots
    # volterra geometry
    ("vol_equal_taps", "volterra", 150, dict(n1Taps=5, n2Taps=5, n3Taps=5, order=3, nTrain=100)),
    ("vol_n3_1", "volterra", 150, dict(n1Taps=7, n2Taps=3, n3Taps=1, order=3, nTrain=100)),
    ("vol_t2_ne_t3", "volterra", 150, dict(n1Taps=9, n2Taps=5, n3Taps=2, order=3, nTrain=100, SpS=2)),
    ("vol_order2_given_h3", "volterra", 150, dict(n1Taps=7, n2Taps=3, n3Taps=2, order=2, nTrain=100, given_h=True)),
    ("vol_fulltime", "volterra", 150, dict(n1Taps=7, n2Taps=3, n3Taps=2, order=3, nTrain=40, trainingMode="fulltime")),
    # feedback taps 0, 1 (64 is above)
    ("dfe_fb0", "dfe", 150, dict(nTapsFF=7, nTapsFB=0, nTrain=100)),
    ("dfe_fb1", "dfe", 150, dict(nTapsFF=7, nTapsFB=1, nTrain=100)),
    # SpS 1, 2, 3, SpS = nTaps; odd and even taps; n no multiple of SpS
    ("ffe_sps2_even", "ffe", 301, dict(nTaps=6, SpS=2, nTrain=100)),
    ("ffe_sps3", "ffe", 400, dict(nTaps=7, SpS=3, nTrain=100)),
    ("ffe_sps_is_taps", "ffe", 403, dict(nTaps=4, SpS=4, nTrain=60)),
    ("dfe_sps8", "dfe", 8 * 70 + 3, dict(nTapsFF=9, nTapsFB=3, SpS=8, nTrain=40)),
    # one tap at one sample per symbol: the reference zeroes the last sample
    ("ffe_one_tap", "ffe", 100, dict(nTaps=1, nTrain=50)),
    # N of one chunk, one chunk - 1, one chunk + 1
    ("ffe_N64", "ffe", 64, dict(nTaps=5, nTrain=64, trainingMode="fulltime")),
    ("ffe_N63", "ffe", 63, dict(nTaps=5, nTrain=20, trainingMode="fulltime")),
    ("dfe_N65", "dfe", 65, dict(nTapsFF=5, nTapsFB=3, nTrain=20)),
    # nTrain 0, 1, N - 1, N, N + 5, on a chunk border
    ("ffe_train0", "ffe", 150, dict(nTaps=5, nTrain=0)),
    ("ffe_train1", "ffe", 150, dict(nTaps=5, nTrain=1)),
    ("ffe_trainNm1", "ffe", 150, dict(nTaps=5, nTrain=149)),
    ("ffe_trainN", "ffe", 150, dict(nTaps=5, nTrain=150, preconvIters=2)),
    ("ffe_trainNp5", "ffe", 150, dict(nTaps=5, nTrain=155, nsym=160)),
    ("ffe_train128", "ffe", 200, dict(nTaps=5, nTrain=128)),
    ("dfe_train0", "dfe", 100, dict(nTapsFF=5, nTapsFB=2, nTrain=0)),
    # a frozen region of one symbol, one tile, one tile + 1; nTrain one before and one behind a frozen-tile border
    ("ffe_frozen_1", "ffe", 100, dict(nTaps=5, nTrain=99)),
    ("ffe_frozen_tile", "ffe", 306, dict(nTaps=5, nTrain=50)),
    ("ffe_frozen_tile_p1", "ffe", 307, dict(nTaps=5, nTrain=50)),
    ("vol_frozen_tile_m1", "volterra", 305, dict(n1Taps=5, n2Taps=3, n3Taps=2, order=3, nTrain=50)),
    # pre-convergence: (nTrain + 1) SpS below, equal to and above nTaps, two and four passes
    ("ffe_pre2_below", "ffe", 150, dict(nTaps=11, nTrain=3, preconvIters=2, SpS=2, mu=5e-3)),
    ("ffe_pre4_below", "ffe", 150, dict(nTaps=11, nTrain=2, preconvIters=4, mu=5e-3)),
    ("ffe_pre4_equal", "ffe", 150, dict(nTaps=8, nTrain=3, preconvIters=4, SpS=2, mu=5e-3)),
    ("ffe_pre2_above", "ffe", 200, dict(nTaps=7, nTrain=70, preconvIters=2)),
    ("ffe_pre4_fulltime", "ffe", 150, dict(nTaps=7, nTrain=70, preconvIters=4, trainingMode="fulltime")),
    ("dfe_pre2_below", "dfe", 150, dict(nTapsFF=11, nTapsFB=5, nTrain=3, preconvIters=2, SpS=2, mu=5e-3)),
    ("dfe_pre4_equal", "dfe", 150, dict(nTapsFF=8, nTapsFB=5, nTrain=3, preconvIters=4, SpS=2, mu=5e-3)),
    ("dfe_pre4_above", "dfe", 200, dict(nTapsFF=7, nTapsFB=70, nTrain=70, preconvIters=4)),
    ("vol_pre2_below", "volterra", 150, dict(n1Taps=9, n2Taps=3, n3Taps=2, order=3, nTrain=2, preconvIters=2, mu=5e-3)),
    ("vol_pre4_above", "volterra", 400, dict(n1Taps=5, n2Taps=3, n3Taps=2, order=3, nTrain=70, preconvIters=4)),
    # tables
    ("ffe_pam2", "ffe", 150, dict(nTaps=5, nTrain=60, M=2)),
    ("ffe_pam8", "ffe", 150, dict(nTaps=5, nTrain=60, M=8)),
    ("ffe_ook", "ffe", 150, dict(nTaps=5, nTrain=60, M=2, constType="ook")),
    ("ffe_qam16", "ffe", 150, dict(nTaps=5, nTrain=60, M=16, constType="qam")),
    ("dfe_qam64", "dfe", 150, dict(nTapsFF=5, nTapsFB=3, nTrain=60, M=64, constType="qam", SpS=2)),
    ("ffe_psk8_f32", "ffe", 150, dict(nTaps=5, nTrain=60, M=8, constType="psk", prec=np.complex64)),
    ("vol_prec32", "volterra", 150, dict(n1Taps=7, n2Taps=3, n3Taps=2, order=3, nTrain=100)),             # prec left at float32
]
ROW_IDS = [r[0] for r in ROWS]


def row(rid):
    """(kind, sigIn, symbRef, parameter object) of a shape row."""
    _, kind, n, prm = next(r for r in ROWS if r[0] == rid)
    prm = dict(prm)
    cx = prm.get("constType", "pam") in ("qam", "psk")
    M, SpS = prm.setdefault("M", 4), prm.get("SpS", 1)
    nsym = prm.pop("nsym", None)
    x, tx = signal(n, SpS, M if prm.get("constType") != "psk" else 4, sum(map(ord, rid)), cx=cx, nsym=nsym)
    prm.setdefault("mu", 1e-2)
    if kind == "volterra" and rid != "vol_prec32":
        prm.setdefault("prec", np.float64)
    if prm.pop("given_h", False):
        rng = np.random.default_rng(7)
        n1, n2, n3 = prm["n1Taps"], prm["n2Taps"], prm["n3Taps"]
        h1 = 0.05 * rng.normal(size=n1)
        h1[n1 // 2] += 1.0
        prm["h"] = [h1, 0.05 * rng.normal(size=(n2, n2)), 0.05 * rng.normal(size=(n3, n3, n3))]       # not symmetric, h3 not zero
    return kind, x, tx, Param(**prm)
