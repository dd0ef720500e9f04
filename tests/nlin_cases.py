"""Shared by the perturbation-model tests: the fixtures tests/golden/nlin/*.npz (tools/gen_golden_nlin.py), the conditions every
fixture must meet, the parameter objects, the bounds, and the files the emulator (tests/emu/emu_nlin.cpp) reads and writes.

The bounds (all relative to the largest magnitude of what is compared against):
    complex128 in, prec complex128: every output against the reference's      1e-9, the standing bound of the double paths
    coefficient matrices against the reference's                               1e-9 of max |C|
    nReducedCoeffs, reductionFactor, the kept set                              equal
    anything single precision takes part in, against the reference's complex128 result:
                                                                               4 x the distance between the reference's own
                                                                               complex64 and complex128 results in the same
                                                                               fixture (the FEC engine's margin), as the
                                                                               generator recorded it per kind of output:
                                                                               dist_d64 (the larger of dx's and dy's),
                                                                               dist_phi64 (of the phases'), dist_nlin64
    every variant (complex64 input, prec complex64) against the restatement of exactly that computation
    (tests/nlin_restatement.py: ``in_single``, ``prec_single``):            1e-9; where the compared values are complex64, 2^-23:
                                                                               one single-precision unit of the largest, two
                                                                               roundings of nearly equal doubles
The reference has no fixture for a complex64 input to the calculation functions, so those calls are held to the restatement
alone; ``perturbationNLIN`` of a complex64 ``Ein`` is recorded in the fixture ``ein64`` and held to 4 x its own distance there.
Only fixtures whose reference distances are nonzero are used (all of them: check_conditions)."""
import json
import os
import subprocess

import numpy as np

import nlin_restatement as rs
from opticommpy_amd import perturbation as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nlin")
CASES = ["am_l3", "am_default", "amr_default", "nb_amr", "tiny", "noisy", "amr_all", "amr_corner", "ein64"]
TOL128 = 1e-9
MARGIN64 = 4.0
EPS32 = 2.0 ** -23
OUTPUTS = ("dx", "dy", "phx", "phy")


class Param:
    """Stand-in for the reference's parameters object: attributes only."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


_LOADED = {}


def load(name):
    """A fixture, read once and shared (nobody writes to it)."""
    if name not in _LOADED:
        z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
        g = {k: z[k] for k in z.files}
        g["cfg"] = json.loads(str(g["cfg"]))
        g["C_ispm"] = complex(g["C_ispm"])
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _LOADED[name] = g
    return _LOADED[name]


def param(g, prec=np.complex128, **kw):
    k = dict(g["cfg"]["param"])
    k["prec"] = prec
    k.update(kw)
    return Param(**k)


def mode(g):
    return g["cfg"]["param"]["mode"]


def coeff_tol(g):
    return g["cfg"]["param"].get("coeffTol", -20)


def rel(got, want):
    """max |got - want| over the largest magnitude of want."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128))) / np.max(np.abs(want)))


def full_matrix(g):
    """C as the calculation forms it: the sum with C_ispm in the corner."""
    C = g["C_ifwm"] + g["C_ixpm"]
    C[-1, -1] = g["C_ispm"]
    return C


def check_conditions(g):
    """What the generator promised, re-asserted on the stored arrays."""
    N = g["cfg"]["N"]
    W = g["C_ifwm"].shape[0]
    assert g["Ein"].shape == (N, 2) and g["C_ifwm"].shape == g["C_ixpm"].shape == (W, W) and W % 2 == 1
    assert W == 2 * g["cfg"]["param"].get("matrixOrder", 25) + 1
    a = np.abs(full_matrix(g)).flatten()
    assert np.sum(a == a.max()) == 1 and int(np.argmax(a)) == W * W - 1          # max |C| once, in the corner
    if mode(g) == "AMR":
        thr = a.max() * 10 ** (coeff_tol(g) / 20)
        nz = a[a > 0]
        assert thr == 0 or np.min(np.abs(nz / thr - 1)) > 1e-9                     # nothing sits on the threshold
        assert 1 <= int(g["nReducedCoeffs"]) <= W * W
    for k in ("nlin",) + OUTPUTS:
        assert g[k + "128"].shape[0] == N and g[k + "64"].shape[0] == N
        assert rel(g[k + "64"], g[k + "128"]) > 0                                  # the single-precision bounds are not empty
    assert float(g["dist_d64"]) == max(rel(g["dx64"], g["dx128"]), rel(g["dy64"], g["dy128"]))
    assert float(g["dist_phi64"]) == max(rel(g["phx64"], g["phx128"]), rel(g["phy64"], g["phy128"]))
    assert float(g["dist_nlin64"]) == rel(g["nlin64"], g["nlin128"])
    assert g["dx64"].dtype == np.complex64 and g["dx128"].dtype == np.complex128 and g["phx64"].dtype == np.float64
    assert len(np.unique(g["Ein"])) > 2
    if "nlin128_e64" in g:
        assert g["nlin128_e64"].dtype == np.complex64 and float(g["dist_e64"]) > 0


_RESTATED = {}


def restate(g, in_single=False, prec_single=False):
    """The restatement's (dx, dy, phi_x, phi_y, nlin) for the fixture's matrices, mode and inputs (rounded to complex64 with
    ``in_single``), computed once per variant and shared."""
    key = (g["cfg"]["name"], in_single, prec_single)
    if key not in _RESTATED:
        keep = off = None
        if mode(g) == "AMR":
            keep, _, _, off = rs.select(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], coeff_tol(g))
        cast = (lambda v: v.astype(np.complex64)) if in_single else (lambda v: v)
        out = rs.nlin(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], cast(g["x"]), cast(g["y"]), keep, off, in_single, prec_single)
        field = rs.perturbation_nlin(cast(g["Ein"]), g["cfg"]["param"].get("Pin", 0), g["C_ifwm"], g["C_ixpm"], g["C_ispm"], keep, off,
                                     prec_single)
        _RESTATED[key] = out + (field,)
        for v in _RESTATED[key]:
            v.setflags(write=False)
    return _RESTATED[key]


def check_calc(g, got, prec, single_in=False):
    """(dx, dy, phi_x, phi_y) of a calculation on the fixture's x, y (cast to complex64 with ``single_in``) at ``prec``: against
    the restatement of exactly that computation, and -- complex128 input -- against the reference; the figures."""
    out = {}
    p64 = np.dtype(prec) == np.complex64
    want = restate(g, single_in, p64)
    for k, v, w in zip(OUTPUTS, got, want):
        v = np.asarray(v)
        assert v.dtype == (np.dtype(prec) if k[0] == "d" else np.float64), (k, v.dtype)
        out[k + "_restated"] = rel(v, w)
        assert out[k + "_restated"] <= (EPS32 if p64 and k[0] == "d" else TOL128), (k, out)
        if not single_in:
            out[k] = rel(v, g[k + "128"])
            bound = MARGIN64 * float(g["dist_d64" if k[0] == "d" else "dist_phi64"]) if p64 else TOL128
            assert out[k] <= bound, (k, out[k], bound)
    return out


def check_nlin(g, got, prec, single_in=False):
    """perturbationNLIN's result for the fixture's Ein (cast to complex64 with ``single_in``) at ``prec``, likewise."""
    got = np.asarray(got)
    p64 = np.dtype(prec) == np.complex64
    assert got.dtype == (np.complex64 if single_in else np.complex128) and got.shape == g["Ein"].shape
    want = restate(g, single_in, p64)[4]
    out = {}
    if single_in:
        out["restated"] = rel(got, want.astype(np.complex64))
        assert out["restated"] <= EPS32, out
        if "nlin128_e64" in g and not p64:
            out["reference"] = rel(got, g["nlin128"])
            assert out["reference"] <= MARGIN64 * float(g["dist_e64"]), (out, float(g["dist_e64"]))
        return out
    out["restated"] = rel(got, want)
    # (prec = complex64: dx and dy pass through single precision, a relative 2^-24 each, before they are scaled into the field)
    assert out["restated"] <= (EPS32 if p64 else TOL128), out
    out["reference"] = rel(got, g["nlin128"])
    bound = MARGIN64 * float(g["dist_nlin64"]) if p64 else TOL128
    assert out["reference"] <= bound, (out, bound)
    return out


# ---- the emulator's files (tests/emu/emu_nlin.cpp)
def build_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_nlin") / "emu_nlin"
    subprocess.check_call(["g++", "-O2", "-mfma", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_nlin.cpp"), "-o", str(exe)])
    return str(exe)


def run_emu(exe, tmp, q):
    """A prepared call (``perturbation._prepare_calc`` / ``_prepare_nlin``: the package's own host side) with the kernels walked
    on the CPU: what ``perturbation._run`` returns."""
    plan, x, n = q["plan"], q["x"], q["n"]
    c64, p64 = x.dtype == np.complex64, q["prec"] == np.complex64
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([plan["L"], len(plan["passes"]), len(plan["coef"]), len(plan["phase_m"]), plan["dense"], q["entry"], c64, p64,
                          plan["ispm_offset"], 0, 0, 0], dtype=np.int32).tobytes())
        f.write(np.array([n], dtype=np.int64).tobytes())
        f.write(np.array([plan["ispm"].real, plan["ispm"].imag, q["peak"]], dtype=np.float64).tobytes())
        for k in ("passes", "coef", "nidx", "phase_m", "phase_c"):
            f.write(plan[k].tobytes())
        f.write(x.tobytes())
        if q["entry"] == 0:
            f.write(q["y"].tobytes())
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")])
    raw = open(tmp / "out.bin", "rb").read()
    if q["entry"] == 1:
        out = np.frombuffer(raw, dtype=x.dtype).reshape(n, 2).copy()
        return [out]
    w = q["prec"].itemsize
    assert len(raw) == 2 * n * w + 2 * n * 8
    return [np.frombuffer(raw[:n * w], dtype=q["prec"]).copy(), np.frombuffer(raw[n * w:2 * n * w], dtype=q["prec"]).copy(),
            np.frombuffer(raw[2 * n * w:2 * n * w + 8 * n], dtype=np.float64).copy(), np.frombuffer(raw[2 * n * w + 8 * n:], dtype=np.float64).copy()]


def prepare_calc(g, x, y, prec):
    if mode(g) == "AMR":
        return pt._prepare_calc(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], x, y, prec, "AMR", coeff_tol(g))
    return pt._prepare_calc(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], x, y, prec, "AM")
