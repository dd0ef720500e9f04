"""The arithmetic of the synchronisation kernels without a GPU: tests/emu/emu_sync.cpp includes
opticommpy_amd/csrc/sync_kernels.h -- the per-element bodies and the decisions the gfx950 kernels call -- and loops them with g++
around a radix-2 transform of its own.  Every fixture and every shape row marked for the emulator is held to the bounds of
tests/test_gpu_sync.py: the output equal to the reference's, delay, swap, rot and conj equal, corrMatrix within 1e-9 of its
largest entry.  The received signal is decimated here with the restatement's decimate: the device's is the receiver engine's."""
import os
import subprocess
import types

import numpy as np
import pytest

import sync_cases as sc
import sync_restatement as sr
import sync_shape_cases as ss
from opticommpy_amd import _lib
from opticommpy_amd import sync as osync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMP, REAL, DELAY = 0, 1, 2


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_sync") / "emu_sync"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_sync.cpp"),
                           "-o", str(exe)])
    return str(exe)


def _run(exe, tmp, mode, modes, x, y, x_f32, y_f32):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([mode, modes, x.shape[0], y.shape[0], _lib.METRICS_DTYPES[x.dtype.name], _lib.METRICS_DTYPES[y.dtype.name],
                          int(x_f32), int(y_f32)], dtype=np.int64).tobytes())
        f.write(x.tobytes())
        f.write(y.tobytes())
    subprocess.check_call([exe, str(tmp / "in.bin"), str(tmp / "out.bin")])
    raw = open(tmp / "out.bin", "rb").read()
    rec = np.frombuffer(raw[:256], dtype=np.int64)
    corr = np.frombuffer(raw[256:768], dtype=np.float64)
    info = types.SimpleNamespace(delay=rec[:modes].copy(), swap=rec[8:8 + modes].copy(),
                                 rot=np.array([_lib.SYNC_ROT[r] for r in rec[16:16 + modes]], dtype=np.complex64),
                                 conj=rec[24:24 + modes].astype(bool), corrMatrix=corr[:modes * modes].reshape(modes, modes).copy())
    return info, raw[768:]


def run_sync(exe, tmp, rx, tx, SpS, mode):
    """symbolSync through the emulator, with the package's own argument handling."""
    rx, tx, p = osync._check(rx, tx, SpS, mode)
    rx2 = rx.reshape(len(rx), -1)
    rx_f32 = rx2.dtype == np.complex64
    if SpS > 1:
        rx2 = sr.decimate(rx2.astype(np.complex128), SpS)
    info, out = _run(exe, tmp, p.mode, p.nModes, tx, rx2, tx.dtype == np.complex64, rx_f32)
    return np.frombuffer(out, dtype=tx.dtype).reshape(tx.shape).copy(), info


@pytest.mark.parametrize("name", sc.EXPECTED_CASES)
def test_emulated_kernels_match_the_reference(emu, tmp_path, name):
    g = sc.load(name)
    sc.check_conditions(g)
    out, info = run_sync(emu, tmp_path, g["rx"], g["tx"], g["cfg"]["SpS"], g["cfg"]["mode"])
    sc.compare(out, info, g["out"], g, name)
    # finddelay on the pairs the reference's own finddelay saw in 'amp': |tx[:, swap[k]]| - mean against |rx_k| - mean
    if g["cfg"]["mode"] == "amp":
        cols = len(g["delay"])
        rx = g["rx"].reshape(len(g["rx"]), cols)
        rx = sr.decimate(rx, g["cfg"]["SpS"]) if g["cfg"]["SpS"] > 1 else rx
        tx = g["tx"].reshape(len(g["tx"]), cols)
        for k in range(cols):
            a, b = np.abs(tx[:, g["swap"][k]]), np.abs(rx[:, k])
            a, b = a - np.mean(a), b - np.mean(b)
            got, _ = _run(emu, tmp_path, DELAY, 1, a, b, False, False)
            assert got.delay[0] == g["delay"][k], (name, k)


@pytest.mark.parametrize("row", ss.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_kernels_match_the_restatement(emu, tmp_path, row):
    ss.check_conditions(row)
    rx, tx = ss.signals(row)
    out, info = run_sync(emu, tmp_path, rx, tx, row.SpS, row.mode)
    ss.compare(row, out, info, "emu")


def test_finddelay_with_complex_sequences_of_unequal_length(emu, tmp_path):
    rng = np.random.default_rng(8)
    for nx, ny, dt in ((50, 50, np.complex128), (64, 31, np.complex64), (17, 90, np.float64), (5, 1, np.float32), (1, 1, np.float64)):
        x = rng.normal(size=nx) + 1j * rng.normal(size=nx)
        y = np.resize(np.roll(x, 3), ny) * np.exp(0.7j) + 0.01 * rng.normal(size=ny)
        if np.dtype(dt).kind == "f":
            x, y = x.real, y.real
        x, y = x.astype(dt), y.astype(dt)
        got, _ = _run(emu, tmp_path, DELAY, 1, x, y, False, False)
        assert got.delay[0] == sr.finddelay(x, y), (nx, ny, dt)
