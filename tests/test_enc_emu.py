"""The arithmetic of the encoder kernels without a GPU: tests/emu/emu_enc.cpp includes opticommpy_amd/csrc/enc_kernels.h -- the
per-lane bodies the gfx950 kernels call -- and walks them with g++ in the tiling of engine_enc.hip (workgroups of 256 lanes, waves
of 64 whose ballot is built lane by lane, a tile of 16 packed messages per workgroup, parities taken 256 checks at a time and a
carry per ballot scanned 64 ballots at a time).  The host side is the package's own (``fec._prepare_encode`` / ``_prepare_mod``), so a fixture goes through everything but
the launch.  Every fixture and every row of tests/enc_shape_cases.py, in both orientations, with ``np.array_equal``."""
import numpy as np
import pytest

import enc_cases as ec
import enc_shape_cases as es


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return ec.build_emu(tmp_path_factory)


@pytest.mark.parametrize("name", sorted(ec.EXPECTED_CASES))
def test_emulated_encoder_matches_the_reference(emu, tmp_path, name):
    g = ec.load(name)
    ec.check_conditions(g)
    p = ec.param(g)
    got = ec.run_emu_encode(emu, tmp_path, g["bits"], p)
    assert got.dtype == np.uint8 and np.array_equal(got, g["codewords"])
    # the same object again (G or P1 / P2 are set now, H is Hm), and the other orientation
    assert np.array_equal(ec.run_emu_encode(emu, tmp_path, g["bits"], p, transposed=True), g["codewords"])
    assert np.array_equal(ec.run_emu_encode(emu, tmp_path, g["bits"], ec.param(g), transposed=True), g["codewords"])
    # more codewords than a tile holds: the fixture's columns repeated
    cols = np.arange(2 * es.TILE + 3) % g["bits"].shape[1]
    got = ec.run_emu_encode(emu, tmp_path, np.ascontiguousarray(g["bits"][:, cols]), p)
    assert np.array_equal(got, g["codewords"][:, cols])


def test_emulated_encoder_with_P1_and_P2_given(emu, tmp_path):
    g = ec.load("p_648_r34")
    p = ec.Param(mode="IEEE_802.11nD2", n=648, P1=ec.unpacked(g, "P1"), P2=ec.unpacked(g, "P2"))
    assert np.array_equal(ec.run_emu_encode(emu, tmp_path, g["bits"], p), g["codewords"])


@pytest.mark.parametrize("row", es.ENC_ROWS, ids=lambda r: r.id)
def test_emulated_shape_row_matches_the_restatement(emu, tmp_path, row):
    prm, bits, want = es.make(row)
    es.check_conditions(row, prm, bits, want)
    for transposed in (False, True):
        got = ec.run_emu_encode(emu, tmp_path, bits, prm, transposed)
        assert got.shape == want.shape and np.array_equal(got, want), (row.id, transposed)


@pytest.mark.parametrize("name", ec.MOD_CASES)
def test_emulated_mapper_matches_the_reference(emu, tmp_path, name):
    g = ec.load_mod(name)
    got = ec.run_emu_modulate(emu, tmp_path, g["bits"], g["cfg"]["M"], g["cfg"]["constType"])
    assert np.array_equal(got, g["symbols"].astype(np.complex128))


@pytest.mark.parametrize("row", es.MOD_ROWS, ids=lambda r: r.id)
def test_emulated_mapper_shape_row_matches_the_restatement(emu, tmp_path, row):
    bits, want = es.mod_make(row)
    got = ec.run_emu_modulate(emu, tmp_path, bits, row.M, row.constType)
    assert got.shape == (row.nsymb,) and np.array_equal(got, want)
