"""The arithmetic of the link-metrics kernels without a GPU: tests/emu/emu_metrics.cpp includes
opticommpy_amd/csrc/metrics_kernels.h -- the per-symbol bodies and combine steps the gfx950 kernels call -- and loops them over
the symbols with g++.  Every fixture is held to the bounds of tests/test_gpu_metrics.py: BER, SER and the demodulated bits equal
the reference's, SNR [dB], GMI, NGMI, MI and both EVMs are within 1e-9 relative."""
import os
import subprocess

import numpy as np
import pytest

import metrics_cases as mc
from opticommpy_amd import _lib
from opticommpy_amd import metrics as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANT_ALL = _lib.METRICS_BER | _lib.METRICS_GMI | _lib.METRICS_MI | _lib.METRICS_EVM
DEMOD = 32


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_metrics") / "emu_metrics"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_metrics.cpp"),
                           "-o", str(exe)])
    return str(exe)


def run_emu(exe, path, want, rx, tx, M, constType, px=None, discard=0):
    """Write the emulator's input as the package would hand it to the library (same tables, same shape rules) and parse its output."""
    if want == _lib.METRICS_EVM_BLIND:
        norm, w32 = om._evm_tables(M, constType)
        raw, pxa, Es, H = np.zeros(M, np.complex128), np.ones(M) / M, 1.0, 1.0
    else:
        raw, norm, pxa, Es, H = om._tables(M, constType, px)
        w32 = np.zeros(M, np.float32)
    rx, n, modes, transposed = om._columns(rx, "rx")
    rx = np.ascontiguousarray(rx)
    with open(path, "wb") as f:
        f.write(np.array([n, modes, _lib.METRICS_DTYPES[rx.dtype.name], transposed, int(constType in ("qam", "psk")), M, discard, want],
                         dtype=np.int64).tobytes())
        f.write(np.array([Es, H], dtype=np.float64).tobytes())
        for a in (raw, norm, pxa, w32):
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(rx.tobytes())
        if tx is not None:
            f.write(np.ascontiguousarray(tx, dtype=rx.dtype).tobytes())
    out = subprocess.check_output([exe, str(path)]).decode()
    if want == DEMOD:
        return np.array(out.split()[1:], dtype=np.int64)
    res = {}
    for line in out.splitlines():
        name, k, val = line.split()
        res.setdefault(name, []).append(float.fromhex(val))
    return {k: np.array(v) for k, v in res.items()}


def test_every_case_of_the_issue_has_a_fixture():
    assert mc.CASES == mc.EXPECTED_CASES


@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_emulated_kernels_match_the_reference(emu, tmp_path, name):
    g = mc.load(name)
    mc.check_conditions(g)
    cfg = g["cfg"]
    M, ct = cfg["M"], cfg["constType"]
    for discard, suffix in ((0, ""), (cfg["discard"], "_d")):
        got = run_emu(emu, tmp_path / "in.bin", WANT_ALL, g["rx"], g["tx"], M, ct, g["px"], discard)
        mc.compare(got, g, suffix, name)
        blind = run_emu(emu, tmp_path / "in.bin", _lib.METRICS_EVM_BLIND, g["rx"], None, M, ct, None, discard)
        mc.compare({"EVM_blind": blind["EVM"]}, g, suffix, name)
    # a selection gives the values of the full call bit for bit
    full = run_emu(emu, tmp_path / "in.bin", WANT_ALL, g["rx"], g["tx"], M, ct, g["px"])
    for want, names in ((_lib.METRICS_BER, ("BER", "SER", "SNR")), (_lib.METRICS_GMI, ("GMI", "NGMI")), (_lib.METRICS_MI, ("MI",)),
                        (_lib.METRICS_EVM, ("EVM",))):
        part = run_emu(emu, tmp_path / "in.bin", want, g["rx"], g["tx"], M, ct, g["px"])
        for k in names:
            assert np.array_equal(part[k], full[k]), (name, k)


@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_emulated_hard_decisions_are_bit_equal(emu, tmp_path, name):
    g = mc.load(name)
    symb = mc.demod_input(g)
    raw = om._tables(g["cfg"]["M"], g["cfg"]["constType"])[0]
    bits = run_emu(emu, tmp_path / "in.bin", DEMOD, symb, None, g["cfg"]["M"], g["cfg"]["constType"])
    assert len(raw) == g["cfg"]["M"] and np.array_equal(bits, g["bits"])


def test_float32_pairwise_mean_is_numpys(emu, tmp_path):
    """The blind EVM's denominator is a float32 np.mean in the reference: the emulated leaf / combine functions must give numpy's
    pairwise sum exactly, at lengths on both sides of the block and unroll boundaries.  Checked through the blind EVM of noisy
    symbols against the numpy expression: a float32 sum in another order would differ by about 1e-8, the double-precision numerator
    differs by rounding only."""
    rng = np.random.default_rng(7)
    table, w32 = om._evm_tables(64, "qam")
    for n in (130, 1000, 4096, 4097, 7992, 8193, 12345, 20001):
        symb = table[rng.integers(0, 64, n)] + 0.03 * (rng.normal(size=n) + 1j * rng.normal(size=n))
        got = run_emu(emu, tmp_path / "in.bin", _lib.METRICS_EVM_BLIND, symb, None, 64, "qam")["EVM"][0]
        s = symb / np.sqrt(np.mean(symb * np.conj(symb)).real)
        c64 = table.astype(np.complex64)
        ind = np.argmin(np.abs(s[:, None] - c64[None, :]), axis=1)
        dec = c64[ind]
        want = np.mean(np.abs(s - dec) ** 2) / np.mean(np.abs(dec) ** 2)
        assert abs(got - want) <= 1e-12 * want, (n, got, want)
