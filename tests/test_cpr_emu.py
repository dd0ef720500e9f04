"""The arithmetic of the carrier-recovery kernels without a GPU: tests/emu/emu_cpr.cpp includes
opticommpy_amd/csrc/cpr_kernels.h -- the per-element bodies the gfx950 kernels call -- and loops them over the symbols with g++.
Every fixture is held to the bounds of tests/test_gpu_cpr.py: raw test phases within 1e-12 rad at every symbol, unwrapped phases
within 1e-9 rad, sigOut and the frequency-compensated signal within 1e-9 (rel-L2 and per element), fo within 1e-12 relative."""
import os
import subprocess

import numpy as np
import pytest

import cpr_cases as cc
from opticommpy_amd import _lib
from opticommpy_amd import cpr as ocpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPR, BPS, FOE, DEROTATE = 0, 1, 2, 3


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_cpr") / "emu_cpr"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_cpr.cpp"),
                           "-o", str(exe)])
    return str(exe)


def run_emu(exe, tmp, what, x, table, Nh=0, B=1, runFOE=0, P=4, Fs=32e9, fo=0.0):
    """Write the emulator's input as the package hands it to the library and read its output back."""
    x, n, modes = ocpr._signal(x)
    x = np.ascontiguousarray(x)
    wide = ocpr._wide(table)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([n, modes, _lib.METRICS_DTYPES[x.dtype.name], Nh, B, len(wide) // 2, runFOE, P, what], dtype=np.int64).tobytes())
        f.write(np.array([Fs, fo], dtype=np.float64).tobytes())
        f.write(wide.tobytes())
        f.write(x.tobytes())
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")])
    raw = np.fromfile(tmp / "out.bin", dtype=np.float64)
    cnt = n * modes
    if what == BPS:
        return raw.reshape(x.shape)
    if what == DEROTATE:
        return raw.view(np.complex128).reshape(x.shape)
    if what == FOE:
        return raw[:2 * cnt].view(np.complex128).reshape(x.shape), raw[2 * cnt:]
    return (raw[:2 * cnt].view(np.complex128).reshape(x.shape), raw[2 * cnt:3 * cnt].reshape(x.shape), raw[3 * cnt:4 * cnt].reshape(x.shape),
            raw[4 * cnt:])


@pytest.mark.parametrize("name", cc.EXPECTED_CASES)
def test_emulated_kernels_match_the_reference(emu, tmp_path, name):
    g = cc.load(name)
    cc.check_conditions(g)
    cfg = g["cfg"]
    table = ocpr._table(cfg["M"], cfg["constType"], cfg["param"].get("shapingFactor", 0))
    sig, phase, raw, fo = run_emu(emu, tmp_path, CPR, g["sigIn"], table, cfg["N"] // 2, cfg["B"], int(cfg["foe"]), cfg["P"], 1 / cfg["Ts"])
    cc.compare_phases(raw, g["raw"], cc.RAW_ABS, f"{name} raw")
    cc.compare_phases(phase, g["phaseEst"], cc.PHASE_ABS, f"{name} phaseEst")
    cc.compare_signal(sig, g["sigOut"], f"{name} sigOut")
    if cfg["foe"]:
        cc.compare_fo(fo, g["fo"], f"{name} fo")
        sig_foe, fo2 = run_emu(emu, tmp_path, FOE, g["sigIn"], table, P=cfg["P"], Fs=1 / cfg["Ts"])
        cc.compare_signal(sig_foe, g["sig_foe"], f"{name} fourthPowerFOE")
        assert np.array_equal(fo2, fo)
    # the search alone, on what the reference's cpr handed to its bps
    alone = run_emu(emu, tmp_path, BPS, cc.bps_input(g), table, cfg["N"] // 2, cfg["B"])
    cc.compare_phases(alone, g["raw"], cc.RAW_ABS, f"{name} bps")


def test_separable_and_full_search_decide_alike(emu, tmp_path):
    """A square-QAM table goes through the two-axis search; the same points with one of them moved by an ulp are no product of
    levels any more and go through the full search.  Both must find the fixture's decisions."""
    g = cc.load("qam64_shaped")
    cfg = g["cfg"]
    table = g["table"].astype(np.complex128)
    moved = table.copy()
    moved[5] = complex(np.nextafter(moved[5].real, 2.0), moved[5].imag)
    for t in (table, moved):
        raw = run_emu(emu, tmp_path, BPS, g["sigIn"], t, cfg["N"] // 2, cfg["B"])
        cc.compare_phases(raw, g["raw"], cc.RAW_ABS, "qam64_shaped bps")


def test_unwrap_is_numpys(emu, tmp_path):
    """np.unwrap(4 phi) / 4 over several scan blocks, on phases that wrap many times: QPSK at high SNR with a fast walk."""
    rng = np.random.default_rng(3)
    n = 5000
    table = ocpr._table(4, "qam", 0)
    walk = np.cumsum(rng.normal(size=(n, 2)) * 0.02, axis=0) + 0.004 * np.arange(n)[:, None]
    x = table.astype(np.complex128)[rng.integers(0, 4, size=(n, 2))] * np.exp(1j * walk)
    x += (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape)) * 0.02
    sig, phase, raw, _ = run_emu(emu, tmp_path, CPR, x, table, 8, 32, 0)
    want = np.unwrap(4 * raw, axis=0) / 4
    assert np.max(np.abs(np.diff(raw, axis=0))) > np.pi / 4 and np.ptp(want) > 4 * np.pi
    cc.compare_phases(phase, want, cc.PHASE_ABS, "unwrap")
    y = x * np.exp(1j * want)
    cc.compare_signal(sig, y / np.sqrt(np.mean(y * np.conj(y)).real), "apply")


def test_frequency_grid_is_numpys(emu, tmp_path):
    """fo is numpy's fftshift(Fs fftfreq(n))[ind] / P at even and odd lengths, negative and positive offsets."""
    rng = np.random.default_rng(5)
    for n, Fs, off in ((257, 1.0, -0.031), (1000, 32e9, 1.9e9), (300, 1.0, 0.124), (4000, 1e3, 120.3)):
        k = np.arange(n)
        x = np.exp(1j * (2 * np.pi * off * k / Fs + rng.choice(4, n) * np.pi / 2 + np.pi / 4)).reshape(n, 1)
        y, fo = run_emu(emu, tmp_path, FOE, x, np.ones(2), P=4, Fs=Fs)
        f = np.fft.fftshift(Fs * np.fft.fftfreq(n))
        ind = np.argmax(np.abs(np.fft.fftshift(np.fft.fft(x[:, 0] ** 4))))
        assert fo[0] == f[ind] / 4 and fo[0] != 0, (n, fo, f[ind] / 4)
        cc.compare_signal(y, x * np.exp(-1j * 2 * np.pi * fo[0] * (k / Fs))[:, None], f"derotation n = {n}")


def test_derotation_holds_at_a_million_radians(emu, tmp_path):
    """The derotation body alone, on symbols 4 000 000 ... of a signal 1.3 GHz off at 32 GBd: angles of 1e6 rad."""
    rng = np.random.default_rng(6)
    n, k0, Fs, fo = 512, 4_000_000, 32e9, 1.3e9
    x = (rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2)))
    y = run_emu(emu, tmp_path, DEROTATE, x, np.ones(2), Nh=k0, Fs=Fs, fo=fo)
    t = np.arange(k0, k0 + n) * 1 / Fs
    assert abs(2 * np.pi * fo * t[0]) > 1e6
    cc.compare_signal(y, x * np.exp(-1j * 2 * np.pi * fo * t)[:, None], "derotation at 1e6 rad")
