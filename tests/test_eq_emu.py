"""The arithmetic of the adaptive-equalizer kernels without a GPU: tests/emu/emu_eq.cpp includes
opticommpy_amd/csrc/eq_kernels.h -- the per-symbol bodies the gfx950 kernels call -- and loops them over lanes and symbols with
g++, in the kernel's lane layout and reduction order.  Every fixture is held to the bounds of tests/test_gpu_eq.py: sigOut and H
within 1e-9 (rel-L2 and per element against max |ref|), errSq within 1e-9 of max |ref|; geometries with two and four
coefficients per lane are held to the numpy restatement at the same bounds."""
import os
import subprocess

import numpy as np
import pytest

import eq_cases as ec
import eq_restatement as er
from opticommpy_amd import equalization as oeq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_eq") / "emu_eq"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_eq.cpp"),
                           "-o", str(exe)])
    return str(exe)


def run_emu(exe, tmp, sigIn, param, symbRef):
    """Write the emulator's input as the package hands it to the library and read (sigOut, H, errSq) back."""
    q = ec.write_emu_input(tmp / "in.bin", sigIn, param, symbRef)
    p = q["params"]
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], stdout=subprocess.DEVNULL)
    raw = np.fromfile(tmp / "out.bin", dtype=np.float64)
    ns, nh = 2 * p.total * p.nModes, 2 * p.nModes ** 2 * p.nTaps
    sigOut = raw[:ns].view(np.complex128).reshape(p.total, p.nModes)
    return (sigOut.reshape(p.total) if q["input1D"] else sigOut, raw[ns:ns + nh].view(np.complex128).reshape(p.nModes ** 2, p.nTaps),
            raw[ns + nh:].reshape(p.nModes, p.total))


@pytest.mark.parametrize("name", ec.EXPECTED_CASES)
def test_emulated_kernels_match_the_reference(emu, tmp_path, name):
    g = ec.load(name)
    ec.check_conditions(g)
    sigOut, H, errSq = run_emu(emu, tmp_path, g["sigIn"], ec.param128(g), g["symbRef"])
    assert sigOut.shape == g["sigOut"].shape
    ec.compare_results(sigOut, H, errSq, g, name, static_from=ec.static_start(g))
    if name == "default_prec":            # prec left at complex64: the single-precision constellation, against the complex64 run
        sigOut = run_emu(emu, tmp_path, g["sigIn"], ec.param(g), g["symbRef"])[0]
        d = ec.rel_l2(sigOut, g["sigOut64"].astype(np.complex128))
        print(f"default_prec: distance to the complex64 run {d:.2e}, the reference's own {float(g['self_err']):.2e}")
        assert d <= 2 * float(g["self_err"]), d


@pytest.mark.parametrize("modes,taps,sps,alg", [
    (2, 33, 2, ["nlms", "dd-lms"]),          # 66 coefficients: two per lane, the second nearly empty
    (3, 23, 1, ["cma", "rde"]),              # 69: two per lane
    (4, 17, 3, ["da-rde", "static", "nlms"]),    # 68: two per lane, a static stage between two adaptive runs
    (3, 64, 2, ["nlms", "rde"]),             # 192: three of four per lane
    (4, 64, 1, ["dd-lms", "cma"]),           # 256: four per lane, all full
])
def test_emulated_lane_layouts_match_the_restatement(emu, tmp_path, modes, taps, sps, alg):
    rng = np.random.default_rng(modes * 100 + taps)
    nsym = 150
    prm = ec.Param(alg=alg, nTaps=taps, SpS=sps, M=16, mu=[4e-3] * len(alg), L=[60, 50, 30][:len(alg)] if len(alg) == 3 else [70, 60],
                   numIter=2, prec=np.complex128)
    table = oeq._tables(16, "qam", 0, np.complex128)[0]
    tx = table[rng.integers(0, 16, size=(nsym, modes))]
    x = np.repeat(tx, sps, axis=0) * 0.9 + 0.05 * (rng.normal(size=(nsym * sps, modes)) + 1j * rng.normal(size=(nsym * sps, modes)))
    x = x + 0.2 * np.roll(x, 1, axis=1)
    want = er.restate(x, prm, tx)
    assert want[3] >= 1e-9
    got = run_emu(emu, tmp_path, x, prm, tx)
    for a, b, what in zip(got, want, ("sigOut", "H", "errSq")):
        ec.compare(a, b, f"{modes} x {taps} taps {alg} {what}")
