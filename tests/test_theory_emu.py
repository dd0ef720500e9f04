"""The kernels of engine_theory.hip on the host: tests/emu/emu_theory.cpp walks the bodies of theory_kernels.h in the kernels' tile
and lane layout (g++, a stand-alone program run as a subprocess), against the fixtures and the shape rows of tests/theory_cases.py.
Bounds as on the GPU: 1e-12 against the long-double restatement, 2e-7 against the reference at tol = 1e-9, calcMI at 1e-9 relative.
The same program is built and run once with the address and undefined-behaviour sanitizers."""
import numpy as np
import pytest

import theory_cases as tc
import theory_restatement as rs


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return tc.build_emu(tmp_path_factory.mktemp("emu_theory") / "emu_theory")


@pytest.fixture(scope="module")
def rows():
    return tc.load("shape_rows")


@pytest.mark.parametrize("name", list(tc.MI_CASES))
def test_fixtures(exe, tmp_path, name):
    g = tc.load(name)
    c = g["cfg"]
    got = tc.emu_theory(exe, tmp_path, g["table"], g["px"], float(g["sigma"]))[0]
    assert abs(got - float(g["restatement"])) <= tc.RS_TOL
    if c["tol"] is not None:
        assert np.all(np.abs(got - g["ref"]) <= tc.REF_TOL)
    else:
        k_all, k_groups = c["symmetry"].index(False), c["symmetry"].index(True)
        assert abs(got - g["ref"][k_all]) <= 2 * g["distance"][k_all] and abs(got - g["ref"][k_groups]) > tc.QUIRK


@pytest.mark.parametrize("name", [r["name"] for r in tc.SHAPE_ROWS if r["name"] not in tc.EMU_SUBSET])
def test_shape_rows(exe, tmp_path, rows, name):
    table, px, sigma = tc.row_input(tc.ROW[name])
    got = tc.emu_theory(exe, tmp_path, table, px, sigma)
    assert got.shape == rows[name].shape and np.max(np.abs(got - rows[name])) <= tc.RS_TOL
    if name == "M1":
        assert got[0] == 0.0
    if name == "snr_m40":
        assert 0 < got[0] < 1e-3
    if name == "snr_p60":
        assert abs(got[0] - rs.entropy(px)) <= tc.RS_TOL
    if name == "grid21":
        assert np.all(np.diff(got) >= 0)
    if name == "nS65":                                  # a value does not depend on which other deviations come with it
        one = tc.emu_theory(exe, tmp_path, table, px, sigma[40:41])
        assert one[0] == got[40]


@pytest.mark.parametrize("name", list(tc.EMU_SUBSET))
def test_large_rows_at_chosen_points(exe, tmp_path, name):
    """All points of these tables take the host minutes; their first, last and a middle one are held to the restatement's."""
    table, px, sigma = tc.row_input(tc.ROW[name])
    pts = tc.EMU_SUBSET[name]
    got = tc.emu_theory(exe, tmp_path, table, px, sigma, points=pts)[0]
    want = rs.point_terms(table, px, sigma[0], pts)
    assert np.max(np.abs(got - want.astype(np.float64))) <= tc.RS_TOL / len(table)      # each point's share of the bound


@pytest.mark.parametrize("name", list(tc.CALC_CASES))
def test_calc_mi_fixtures(exe, tmp_path, name):
    g = tc.load(name)
    got = tc.emu_calc_mi(exe, tmp_path, g["rx"], g["tx"], float(g["sigma2"]), g["table"], g["px"])
    assert abs(got - float(g["restatement"])) <= tc.CALC_TOL * abs(float(g["restatement"]))
    if g["cfg"]["dtype"] != "complex64":                 # (the reference takes single-precision distances of single-precision data)
        assert abs(got - g["mi"][0]) <= tc.CALC_TOL * abs(g["mi"][0])


@pytest.mark.parametrize("n", tc.CALC_ROWS)
def test_calc_mi_rows(exe, tmp_path, n):
    rx, tx, s2, table, px = tc.calc_input(n)
    want = float(rs.calc_mi(rx, tx, s2, table, px))
    got = tc.emu_calc_mi(exe, tmp_path, rx, tx, s2, table, px)
    assert abs(got - want) <= tc.CALC_TOL * abs(want)


def test_under_the_sanitizers(tmp_path):
    exe = tc.build_emu(tmp_path / "emu_theory_san", flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    g = tc.load("qam16_mb_10dB")
    got = tc.emu_theory(exe, tmp_path, g["table"], g["px"], float(g["sigma"]))[0]
    assert abs(got - float(g["restatement"])) <= tc.RS_TOL
    table, px, sigma = tc.row_input(tc.ROW["M3"])
    assert tc.emu_theory(exe, tmp_path, table, px, sigma, points=(2,)).shape == (1, 1)
    rx, tx, s2, table, px = tc.calc_input(257)
    want = float(rs.calc_mi(rx, tx, s2, table, px))
    assert abs(tc.emu_calc_mi(exe, tmp_path, rx, tx, s2, table, px) - want) <= tc.CALC_TOL * abs(want)
