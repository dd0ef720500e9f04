"""The long-double restatement of the theoretical-MI rule (tests/theory_restatement.py) against the fixtures, the rule against half
its step, the factorised forms the sweep uses against the general one, and the host functions of opticommpy_amd.theory against the
reference's recorded values.  No GPU and no library."""
import json
import os

import numpy as np
import pytest

import opticommpy_amd as oa
import theory_cases as tc
import theory_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [n for n, c in tc.MI_CASES.items() if c["M"] <= 16]


@pytest.fixture(scope="module")
def restated():
    """The rule on every theoryMI fixture, once."""
    out = {}
    for name in tc.MI_CASES:
        g = tc.load(name)
        out[name] = rs.rule_mi(g["table"], g["px"], float(g["sigma"]))
    return out


@pytest.mark.parametrize("name", list(tc.MI_CASES))
def test_restatement_against_the_fixtures(restated, name):
    g = tc.load(name)
    c = g["cfg"]
    assert abs(float(restated[name]) - float(g["restatement"])) <= 1e-15
    assert float(g["sigma"]) == float(rs.sigma_of(c["SNR"]))
    dist = np.abs(g["ref"] - float(restated[name]))
    assert np.allclose(dist, g["distance"], rtol=0, atol=1e-15)
    if c["tol"] is not None:
        assert np.all(dist <= tc.REF_FIX), dist
    else:                                       # 64-QAM: all points within the quirk's size, the |x| groups well beyond it
        assert dist[c["symmetry"].index(False)] < tc.QUIRK < dist[c["symmetry"].index(True)], dist


@pytest.mark.parametrize("name", SMALL)
def test_rule_against_half_its_step(restated, name):
    g = tc.load(name)
    fine = rs.rule_mi(g["table"], g["px"], float(g["sigma"]), h=rs.H_STEP / 2)
    assert abs(float(restated[name] - fine)) <= tc.RULE_BOUND


def test_the_sweeps_factorised_forms_are_the_rule(restated):
    g = tc.load("qam16_10dB")
    lv = np.unique(g["table"].real)
    sep = rs.rule_mi_separable(lv, np.unique(g["table"].imag), float(g["sigma"]))
    assert abs(float(sep - restated["qam16_10dB"])) <= 1e-15
    g = tc.load("pam4_10dB")
    assert abs(float(rs.rule_mi_real(g["table"], None, float(g["sigma"])) - restated["pam4_10dB"])) <= 1e-15


def test_one_point_per_orbit_is_the_rule(restated):
    """What the sweep does for PSK: the grid's symmetries map the table onto itself, the rule's value is the same for every point
    of an orbit, and both steps come from one pass over the finer grid."""
    g = tc.load("psk8_8dB")
    orbits = rs.d4_orbits(g["table"])
    assert sorted(m for _, m in orbits) == [4, 4]
    coarse, fine = rs.point_terms_pair(g["table"], g["px"], float(g["sigma"]), [i for i, _ in orbits])
    mult = np.array([m for _, m in orbits]).astype(rs.LD)
    H = rs.LD(rs.entropy(g["px"]))
    assert abs(float(H - np.sum(mult * coarse) - restated["psk8_8dB"])) <= 1e-15
    assert abs(float(H - np.sum(mult * fine) - rs.rule_mi(g["table"], g["px"], float(g["sigma"]), h=rs.H_STEP / 2))) <= 1e-15
    assert sorted(m for _, m in rs.d4_orbits(np.array([1.0, -1.0]))) == [2]                  # 2-PSK: the reflections only
    assert sorted(m for _, m in rs.d4_orbits(tc.load("qam16_10dB")["table"])) == [4, 4, 8]
    with pytest.raises(AssertionError):
        rs.d4_orbits(tc.scattered(5, 1))


def test_recorded_sweep_is_within_the_bound():
    with open(os.path.join(ROOT, "profiles", "theory_quadrature.json")) as f:
        q = json.load(f)
    assert (q["h"], q["T"], q["bound"]) == (rs.H_STEP, rs.T_MAX, tc.RULE_BOUND) == (oa.theory.RULE_STEP, oa.theory.RULE_RANGE, oa.theory.RULE_BOUND)
    assert 0 < q["worst"]["err"] <= tc.RULE_BOUND
    every = (2, 4, 8, 16, 64, 256, 1024)
    assert {(c["M"], c["constType"]) for c in q["cases"]} == ({(M, "qam") for M in (4, 16, 64, 256, 1024)} | {(M, "pam") for M in every}
                                                              | {(M, "psk") for M in every})
    assert q["snr_dB"] == [float(v) for v in np.arange(-10.0, 40.01, 2.5)] and "not_swept" not in q
    assert {c["M"]: c["points"] for c in q["cases"] if c["constType"] == "psk"} == {2: 1, 4: 1, 8: 2, 16: 3, 64: 9, 256: 33, 1024: 129}
    assert all(c["worst"] <= tc.RULE_BOUND for c in q["cases"])


@pytest.mark.parametrize("name", ["M1", "M2", "M3", "nS2", "px_six_decades", "snr_m40", "snr_p60"])
def test_shape_row_values_are_the_restatements(name):
    table, px, sigma = tc.row_input(tc.ROW[name])
    want = tc.load("shape_rows")[name]
    got = np.array([float(rs.rule_mi(table, px, s)) for s in sigma])
    assert np.max(np.abs(got - want)) <= 1e-15
    if name == "M1":
        assert got[0] == 0.0
    if name == "snr_m40":
        assert 0 < got[0] < 1e-3
    if name == "snr_p60":
        assert abs(got[0] - rs.entropy(px)) <= 1e-15


@pytest.mark.parametrize("name", list(tc.CALC_CASES))
def test_calc_mi_restatement_against_the_reference(name):
    g = tc.load(name)
    got = float(rs.calc_mi(g["rx"], g["tx"], float(g["sigma2"]), g["table"], g["px"]))
    assert g["mi"].shape == (1,) and got == float(g["restatement"])
    # the reference takes single-precision distances of single-precision data; in double it is within rounding of the restatement
    assert abs(got - g["mi"][0]) <= (1e-5 if g["cfg"]["dtype"] == "complex64" else 1e-12) * abs(got)
    assert float(g["sigma2"]) == float(np.var(g["rx"] - g["tx"])) and g["rx"].shape == (tc.CALC_N,)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    return float(np.max(np.abs(got - want) / np.abs(want)))


def test_host_functions_against_the_reference():
    import types
    g = tc.load("gn_model")
    p = types.SimpleNamespace(Ltotal=700, Lspan=50, alpha=0.2, D=16, gamma=1.3, Fc=193.1e12)
    Ptx = np.arange(-10, 1.5, 0.5)
    assert np.array_equal(Ptx, g["Ptx"])
    OSNR, P_nli, P_ase = oa.GNmodel_OSNR(32e9, 80, 37.5e9, Ptx, p, 12.5e9)
    assert max(rel(OSNR, g["OSNR"]), rel(P_nli, g["P_nli"]), rel(P_ase, g["P_ase"])) <= tc.HOST_TOL
    assert rel(oa.GNmodel_OSNR(32e9, 80, 37.5e9, Ptx)[0], g["OSNR_default"]) <= tc.HOST_TOL
    lin = oa.calcLinOSNR(14, -4, 0.2, 50, 35, 6, 193.1e12, 12.5e9)
    assert lin.shape == (15,) and rel(lin, g["lin"]) <= tc.HOST_TOL
    assert rel(oa.GN_Model_NyquistWDM(32e9, 80, 37.5e9, 0.2, 1.3, 50, 14, -2.0, 16, 12.5e9, 193.1e12), g["gn_one"]) <= tc.HOST_TOL
    assert rel(oa.ASE_NyquistWDM(0.2, 50, 14, 4.5, 12.5e9, 193.1e12), g["ase_one"]) <= tc.HOST_TOL
    ce = oa.condEntropy(0.3, -0.2, g["table16"].astype(np.complex64), np.ones(16) / 16, 5, 0.25)
    assert rel(ce, g["cond_entropy"]) <= tc.HOST_TOL
    # the restatement's own host functions, the same way
    assert rel(rs.lin_osnr(14, -4, 0.2, 50, 35, 6, 193.1e12, 12.5e9), g["lin"]) <= tc.HOST_TOL
    assert rel(rs.gn_model(32e9, 80, 37.5e9, 0.2, 1.3, 50, 14, -2.0, 16, 12.5e9, 193.1e12), g["gn_one"]) <= tc.HOST_TOL
    assert rel(rs.ase(0.2, 50, 14, 4.5, 12.5e9, 193.1e12), g["ase_one"]) <= tc.HOST_TOL
    assert rel(rs.cond_entropy(0.3, -0.2, g["table16"].astype(np.complex64), np.ones(16) / 16, 5, 0.25), g["cond_entropy"]) <= tc.HOST_TOL
