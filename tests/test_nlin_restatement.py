"""The numpy restatement of the perturbation model (tests/nlin_restatement.py) against every reference-generated fixture, in both
modes: it is what the GPU shape rows and the emulator are held to, so it is held to the reference first."""
import numpy as np
import pytest

import nlin_cases as nc
import nlin_restatement as rs


@pytest.mark.parametrize("name", nc.CASES)
def test_fixture_meets_its_conditions(name):
    nc.check_conditions(nc.load(name))


@pytest.mark.parametrize("name", nc.CASES)
def test_restatement_matches_the_reference_in_double(name):
    g = nc.load(name)
    got = nc.restate(g)
    for k, v in zip(nc.OUTPUTS, got):
        d = nc.rel(v, g[k + "128"])
        assert d <= nc.TOL128, (k, d)
    assert nc.rel(got[4], g["nlin128"]) <= nc.TOL128


@pytest.mark.parametrize("name", nc.CASES)
def test_restatement_at_single_precision_stays_within_the_reference_margin(name):
    g = nc.load(name)
    got = nc.restate(g, False, True)
    assert got[0].dtype == np.complex64
    for k, v in zip(nc.OUTPUTS, got):
        d = nc.rel(v, g[k + "128"])
        assert d <= nc.MARGIN64 * float(g["dist_d64" if k[0] == "d" else "dist_phi64"]), (k, d)
    assert nc.rel(got[4], g["nlin128"]) <= nc.MARGIN64 * float(g["dist_nlin64"])


@pytest.mark.parametrize("name", [n for n in nc.CASES if nc.mode(nc.load(n)) == "AMR"])
def test_selection_matches_the_reference(name):
    g = nc.load(name)
    keep, n, factor, off = rs.select(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], nc.coeff_tol(g))
    L = (keep.shape[0] - 1) // 2
    assert n == int(g["nReducedCoeffs"]) == int(keep.sum()) and factor == float(g["reductionFactor"])
    assert off == L                                                     # the corner: the symbol L places after the current one


def test_everything_kept_gives_the_full_model_but_other_phases():
    g = nc.load("amr_all")
    full = rs.nlin(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], g["x"], g["y"])
    assert nc.rel(full[0], g["dx128"]) <= nc.TOL128 and nc.rel(full[1], g["dy128"]) <= nc.TOL128
    assert nc.rel(full[2], g["phx128"]) > 1e-3                          # 'AM' takes the symbol L places before
