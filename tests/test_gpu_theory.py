"""theoryMI, constellationMI and calcMI on the GPU against the fixtures tests/golden/theory/*.npz (the reference's values and the
long-double restatement of the rule) and the shape rows of tests/theory_cases.py.  Bounds as stated there."""
import types

import numpy as np
import pytest

import opticommpy_amd as oa
import theory_cases as tc
import theory_restatement as rs
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    return tc.load("shape_rows")


@pytest.mark.parametrize("name", list(tc.MI_CASES))
def test_theory_mi_fixtures(name):
    g = tc.load(name)
    c = g["cfg"]
    px = None if c["px"] is None else g["px"]
    got = oa.theoryMI(c["M"], c["constType"], c["SNR"], pX=px)
    print(f"{name}: device {got:.15f} restatement {float(g['restatement']):.15f} ref {g['ref']}")
    assert type(got) is float and abs(got - float(g["restatement"])) <= tc.RS_TOL
    if c["tol"] is not None:
        assert np.all(np.abs(got - g["ref"]) <= tc.REF_TOL)
    else:
        k_all, k_groups = c["symmetry"].index(False), c["symmetry"].index(True)
        assert abs(got - g["ref"][k_all]) <= 2 * g["distance"][k_all] and abs(got - g["ref"][k_groups]) > tc.QUIRK
    # symmetry and tol change nothing, a repeated call gives the same bits, and so does the table handed to constellationMI
    assert oa.theoryMI(c["M"], c["constType"], c["SNR"], pX=px, symmetry=False, tol=1e-9) == got
    assert oa.constellationMI(g["table"], c["SNR"], pX=px) == got


@pytest.mark.parametrize("name", [r["name"] for r in tc.SHAPE_ROWS])
def test_shape_rows(rows, name):
    table, px, sigma = tc.row_input(tc.ROW[name])
    snr = np.array(tc.ROW[name]["SNR"])
    got = oa.constellationMI(table, snr, pX=px)
    err = float(np.max(np.abs(got - rows[name])))
    print(f"{name}: largest distance to the restatement {err:.2e}")
    assert isinstance(got, np.ndarray) and got.shape == rows[name].shape and got.dtype == np.float64 and err <= tc.RS_TOL
    assert np.array_equal(oa.constellationMI(table, snr, pX=px), got)            # repeats bit for bit
    if name == "M1":
        assert got[0] == 0.0
    if name == "snr_m40":
        assert 0 < got[0] < 1e-3
    if name == "snr_p60":
        assert abs(got[0] - rs.entropy(px)) <= tc.RS_TOL
    if name == "grid21":
        assert np.all(np.diff(got) >= 0)
    if name in ("nS2", "nS65", "grid21"):                                       # an array SNR equals the scalar calls bit for bit
        for k in (0, len(snr) // 2, len(snr) - 1):
            assert oa.constellationMI(table, float(snr[k]), pX=px) == got[k]


def test_real_table_is_the_complex_one():
    g = tc.load("pam4_10dB")
    assert oa.constellationMI(g["table"].real.copy(), 10.0) == oa.constellationMI(g["table"], 10.0)


@pytest.mark.parametrize("name", list(tc.CALC_CASES))
def test_calc_mi_fixtures(name):
    g = tc.load(name)
    rx0, tx0 = g["rx"].copy(), g["tx"].copy()
    got = oa.calcMI(rx0, tx0, float(g["sigma2"]), g["table"], g["px"])
    print(f"{name}: device {got[0]:.15f} restatement {float(g['restatement']):.15f} ref {g['mi'][0]:.15f}")
    assert isinstance(got, np.ndarray) and got.shape == (1,) and got.dtype == np.float64
    assert abs(got[0] - float(g["restatement"])) <= tc.CALC_TOL * abs(float(g["restatement"]))
    if g["cfg"]["dtype"] != "complex64":                 # (the reference takes single-precision distances of single-precision data)
        assert abs(got[0] - g["mi"][0]) <= tc.CALC_TOL * abs(g["mi"][0])
    rx, tx = oa.to_device(rx0), oa.to_device(tx0)
    before = device.transfer_counts()
    on_dev = oa.calcMI(rx, tx, float(g["sigma2"]), g["table"], g["px"])
    assert device.transfer_counts() == before and np.array_equal(on_dev, got)
    assert np.array_equal(rx.get(), g["rx"]) and np.array_equal(tx.get(), g["tx"]) and np.array_equal(rx0, g["rx"]) and np.array_equal(tx0, g["tx"])


@pytest.mark.parametrize("n", tc.CALC_ROWS)
def test_calc_mi_rows(n):
    rx, tx, s2, table, px = tc.calc_input(n)
    want = float(rs.calc_mi(rx, tx, s2, table, px))
    got = oa.calcMI(rx, tx, s2, table, px)
    assert abs(got[0] - want) <= tc.CALC_TOL * abs(want), (n, got[0], want)
    assert np.array_equal(oa.calcMI(rx, tx, s2, table, px), got)


def test_monte_carlo_mi_is_calc_mi_on_the_normalised_arrays():
    g = tc.load("calc_qam16")
    rx, tx = g["rx"], g["tx"]
    mc = oa.monteCarloMI(rx, tx, 16, "qam")[0]
    rxn = np.mean(tx / rx) * rx
    rxn, txn = rxn / np.sqrt(np.mean(np.abs(rxn) ** 2)), tx / np.sqrt(np.mean(np.abs(tx) ** 2))
    const = oa.grayMapping(16, "qam")
    px = np.ones(16) / 16
    table = const / np.sqrt(np.sum(np.abs(const) ** 2 * px))
    direct = oa.calcMI(rxn, txn, np.var(rxn - txn), table, px)[0]
    assert abs(mc - direct) <= tc.CALC_TOL * abs(direct), (mc, direct)


def test_chain_monte_carlo_against_theory():
    """2^16 16-QAM symbols through awgn at 12 dB: the estimate's standard deviation is about 1.5 / sqrt(n) = 0.006 bit."""
    n = 1 << 16
    rng = np.random.default_rng(2024)
    const = oa.grayMapping(16, "qam").astype(np.complex128)
    tx = const[rng.integers(0, 16, size=n)] / np.sqrt(np.mean(np.abs(const) ** 2))
    rx = oa.awgn(tx, types.SimpleNamespace(snr=12.0, seed=11))
    mc = oa.monteCarloMI(rx, tx, 16, "qam")[0]
    th = oa.theoryMI(16, "qam", 12.0)
    print(f"chain: monteCarloMI {mc:.6f} theoryMI {th:.6f}")
    assert abs(mc - th) <= 0.05
