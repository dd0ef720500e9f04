"""The arithmetic of the OFDM kernels without a GPU: tests/emu/emu_ofdm.cpp includes opticommpy_amd/csrc/ofdm_kernels.h -- the bodies
the gfx950 kernels call -- and walks them with g++ in the launch geometry of engine_ofdm.hip (lanes as fibers that meet at the
barriers of the register-and-LDS transform; a plain DFT where rocFFT stands).  The host side is the package's own
(``ofdm._prepare_mod`` / ``_prepare_demod``), so a fixture goes through everything but the launch, at the bounds of
tests/ofdm_cases.py."""
import numpy as np
import pytest

import ofdm_cases as oc
import ofdm_restatement as rs
import ofdm_shape_cases as sc


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return oc.build_emu(tmp_path_factory)


@pytest.mark.parametrize("route", ["auto", "rocfft"])
@pytest.mark.parametrize("name", oc.CASES)
def test_emulated_modulator_matches_the_reference(emu, tmp_path, name, route):
    g = oc.load(name)
    oc.check_conditions(g)
    for in_dtype in (np.complex128, np.complex64):
        x = g["symb"].astype(in_dtype)
        got = oc.run_emu_mod(emu, tmp_path, x, oc.param(g), np.complex64, route)
        oc.check_mod(g, got, np.complex64)
        wide = oc.run_emu_mod(emu, tmp_path, x, oc.param(g), np.complex128, route)
        oc.check_mod(g, wide, np.complex128)
        assert np.array_equal(wide.astype(np.complex64), got)


@pytest.mark.parametrize("route", ["auto", "rocfft"])
@pytest.mark.parametrize("name", oc.CASES)
def test_emulated_demodulator_matches_the_reference(emu, tmp_path, name, route):
    g = oc.load(name)
    for dtype in (np.complex128, np.complex64):
        got, H = oc.run_emu_demod(emu, tmp_path, g["rx"].astype(dtype), oc.param(g), route)
        oc.check_demod(g, got, H, dtype)


@pytest.mark.parametrize("row", sc.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_shape_row_matches_the_restatement(emu, tmp_path, row):
    c = sc.make(row)
    got = oc.run_emu_mod(emu, tmp_path, c.symb, c.param, np.complex128)
    sc.check_mod(c, got, np.complex128)
    got, H = oc.run_emu_demod(emu, tmp_path, c.rx, c.param)
    sc.check_demod(c, got, H, np.complex128)
