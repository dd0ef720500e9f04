"""The arithmetic of the soft-decision FEC kernels without a GPU: tests/emu/emu_fec.cpp includes
opticommpy_amd/csrc/fec_kernels.h -- the node bodies the gfx950 kernels call -- and walks them over nodes and codewords with g++
as the two engines of engine_fec.hip do (padded per-codeword messages and a loop left at convergence; messages of all codewords
with the unsat / done flags of the launches).  Every fixture is held to the bounds of tests/fec_cases.py in both precisions and
from both walks, which must agree bit for bit; so is every row of tests/fec_shape_cases.py marked for the emulator, against the
restatement."""
import os
import subprocess

import numpy as np
import pytest

import fec_cases as fc
import fec_restatement as fr
import fec_shape_cases as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_fec") / "emu_fec"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_fec.cpp"),
                           "-o", str(exe)])
    return str(exe)


def run_emu(exe, tmp, llrs, prm, engine, transposed=False):
    q = fc.write_emu_ldpc(tmp / "in.bin", llrs, prm, engine, transposed)
    subprocess.check_call([exe, "ldpc", str(tmp / "in.bin"), str(tmp / "out.bin")])
    return fc.read_emu_ldpc(tmp / "out.bin", q)


@pytest.mark.parametrize("name", fc.EXPECTED_CASES)
def test_emulated_kernels_match_the_reference(emu, tmp_path, name):
    g = fc.load(name)
    fc.check_conditions(g)
    for prec in fc.PRECS:
        got = {e: run_emu(emu, tmp_path, g["llrs"], fc.param(g, prec), e) for e in ("lds", "global")}
        fc.compare_decode(got["lds"], g, prec, f"{name} [{prec}]")
        for a, b in zip(got["lds"], got["global"]):
            assert a.tobytes() == b.tobytes(), (name, prec)              # the two walks: the same bits
        # the other orientation and a single-precision input
        bits, out, fail, last = run_emu(emu, tmp_path, np.ascontiguousarray(g["llrs"].T), fc.param(g, prec), "global", transposed=True)
        assert out.T.tobytes() == np.ascontiguousarray(got["lds"][1]).tobytes() or np.array_equal(out.T, got["lds"][1]), name
        assert np.array_equal(bits.T, got["lds"][0]) and np.array_equal(fail, got["lds"][2]) and np.array_equal(last, got["lds"][3])


@pytest.mark.parametrize("ncw", [1, 65, 300])
def test_emulated_batches_repeat_the_fixture(emu, tmp_path, ncw):
    """Fewer codewords than a workgroup has threads, and more: the global walk keeps its parity flags per codeword in the first
    case and per thread in the second."""
    g = fc.load("msa_648_mixed")
    cols = np.arange(ncw) % 4 if ncw > 1 else np.array([2])
    x = np.ascontiguousarray(g["llrs"][:, cols])
    for engine in ("lds", "global"):
        fc.compare_decode(run_emu(emu, tmp_path, x, fc.param(g), engine), g, "float64", f"x {ncw} [{engine}]", columns=cols)


def test_a_float32_input_is_clipped_then_widened(emu, tmp_path):
    g = fc.load("msa_648_clip")
    x32 = g["llrs"].astype(np.float32)
    want = fr.decode(g["indptr"], g["indices"], g["shape"], x32, "MSA", 8, np.float64)
    got = run_emu(emu, tmp_path, x32, fc.param(g, "float64"), "lds")
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dc", [3, 9, 33, 64])
def test_emulated_check_degrees_match_the_restatement(emu, tmp_path, dc):
    """One graph per form of the SPA check body (unrolled to 8, to 32, the loop) with irregular degrees up to ``dc``, and the
    variable degrees that follow; float64 at the bound of the fixtures, MSA bit-equal."""
    rng = np.random.default_rng(dc)
    m, n = 40, 160
    indptr, indices = fs.sampled_graph(rng, m, n, (dc, 2), 2, dc)
    assert np.diff(indptr)[0] == dc and np.diff(indptr).max() == dc and np.diff(indptr).min() == 2
    llrs = 2 * (1 + 0.8 * rng.normal(size=(n, 3))) / 0.64
    for alg in ("SPA", "MSA"):
        prm = fc.Param(H=fc.Csr(indptr, indices, (m, n)), alg=alg, maxIter=5, prec=np.float64)
        want = fr.decode(indptr, indices, (m, n), llrs, alg, 5, np.float64)
        for engine in ("lds", "global"):
            bits, out, fail, last = run_emu(emu, tmp_path, llrs, prm, engine)
            assert np.array_equal(bits, want[0]) and np.array_equal(fail, want[2]) and np.array_equal(last, want[3]), (dc, alg, engine)
            if alg == "MSA":
                assert np.array_equal(out, want[1]), (dc, engine)
            else:
                assert np.all(fc.rel_cols(out, want[1]) <= fc.REL), (dc, engine, fc.rel_cols(out, want[1]))


@pytest.mark.parametrize("row", fs.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_shape_row_matches_the_restatement(emu, tmp_path, row):
    """Every size, degree and edge of tests/fec_shape_cases.py from both walks, one of them in the other orientation."""
    fs.check_conditions(row)
    x = fs.signals(row)
    lds = run_emu(emu, tmp_path, x, fs.param(row), "lds")
    fs.compare(row, lds, "emulated, lds")
    bits, out, fail, last = run_emu(emu, tmp_path, np.ascontiguousarray(x.T), fs.param(row), "global", transposed=True)
    for a, b in zip((bits.T, out.T, fail, last), lds):
        assert a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), row.id


@pytest.mark.parametrize("row", fs.EMU_LLR_ROWS, ids=lambda r: r.id)
def test_emulated_llr_shape_row_matches_the_restatement(emu, tmp_path, row):
    fs.check_llr_conditions(row)
    g = fs.llr_signals(row)
    q = fc.write_emu_llr(tmp_path / "in.bin", g)
    subprocess.check_call([emu, "llr", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    assert got.shape == (row.n * q["b"],)
    fs.compare_llr(row, got, "emulated")


@pytest.mark.parametrize("name", fc.LLR_CASES)
def test_emulated_llr_matches_the_reference(emu, tmp_path, name):
    g = fc.load_llr(name)
    q = fc.write_emu_llr(tmp_path / "in.bin", g)
    subprocess.check_call([emu, "llr", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    assert got.shape == (len(g["rxSymb"]) * q["b"],)
    fc.compare_llr(got, g, name)
