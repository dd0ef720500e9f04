"""The arithmetic of the perturbation-model kernels without a GPU: tests/emu/emu_nlin.cpp includes
opticommpy_amd/csrc/nlin_kernels.h -- the bodies the gfx950 kernels call -- and walks them with g++ in the launch geometry and the
launch sequence of engine_nlin.hip (lanes as fibers that meet at the barriers between the lines of the main kernel; the power
sums in the engine's order).  The host side is the package's own (``perturbation._prepare_calc`` / ``_prepare_nlin``), so a
fixture goes through everything but the launch, at the bounds of tests/nlin_cases.py."""
import numpy as np
import pytest

import nlin_cases as nc
import nlin_shape_cases as sc
from opticommpy_amd import perturbation as pt


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return nc.build_emu(tmp_path_factory)


@pytest.mark.parametrize("name", nc.CASES)
def test_emulated_calculation_matches_the_reference(emu, tmp_path, name):
    g = nc.load(name)
    nc.check_conditions(g)
    for prec in (np.complex128, np.complex64):
        nc.check_calc(g, nc.run_emu(emu, tmp_path, nc.prepare_calc(g, g["x"], g["y"], prec)), prec)
        x, y = g["x"].astype(np.complex64), g["y"].astype(np.complex64)
        nc.check_calc(g, nc.run_emu(emu, tmp_path, nc.prepare_calc(g, x, y, prec)), prec, single_in=True)


@pytest.mark.parametrize("name", nc.CASES)
def test_emulated_field_matches_the_reference(emu, tmp_path, name):
    g = nc.load(name)
    for prec in (np.complex128, np.complex64):
        q = pt._prepare_nlin(g["Ein"], nc.param(g, prec))
        nc.check_nlin(g, nc.run_emu(emu, tmp_path, q)[0], prec)
        q = pt._prepare_nlin(g["Ein"].astype(np.complex64), nc.param(g, prec))
        nc.check_nlin(g, nc.run_emu(emu, tmp_path, q)[0], prec, single_in=True)


@pytest.mark.parametrize("row", sc.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_shape_row_matches_the_restatement(emu, tmp_path, row):
    c = sc.make(row)
    for prec in (np.complex128, np.complex64):
        sc.check_calc(c, nc.run_emu(emu, tmp_path, sc.prepare_calc(c, prec)), prec)
        sc.check_nlin(c, nc.run_emu(emu, tmp_path, pt._prepare_nlin(c.Ein, sc.param(c, prec)))[0], prec)
