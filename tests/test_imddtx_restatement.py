"""tests/imddtx_restatement.py is held to the reference's fixtures first: 1e-12 of the largest sample for every field, bit for bit
for upsample.  Only then do the shape rows of the emulator and GPU tests lean on it."""
import numpy as np
import pytest

import imddtx_cases as ic
import imddtx_restatement as ir


def test_the_fixtures_are_the_expected_files_and_show_what_they_must():
    ic.check_files()
    ic.check_conditions()


@pytest.mark.parametrize("case", ic.PAM_CASES)
def test_pam_path_matches_the_reference(case):
    g = ic.load("pam_" + case)
    d = g["cfg"]["param"]
    got = ic.pam_restated(g["symbTx"], g["pulse"], d)
    err = ic.rel_peak(got, g["sigTxo"])
    print(f"pam_{case}: {err:.2e}")
    assert err <= ic.BOUND
    N = (d["nBits"] // int(np.log2(d.get("M", 4)))) * d.get("SpS", 16)
    assert g["sigTxo"].shape == ((N,) if d.get("nPolModes", 1) == 1 else (N, d["nPolModes"]))


@pytest.mark.parametrize("case", ic.MOD_CASES)
def test_modulators_match_the_reference(case):
    g = ic.load("mod_" + case)
    err = ic.rel_peak(ic.mod_restated(g), g["out"])
    print(f"mod_{case}: {err:.2e}")
    assert err <= ic.BOUND


@pytest.mark.parametrize("case", ic.AWGN_CASES)
def test_awgn_matches_the_reference(case):
    g = ic.load("awgn_" + case)
    got = ic.awgn_restated(g)
    assert got.dtype == g["out"].dtype
    err = ic.rel_peak(got, g["out"])
    print(f"awgn_{case}: {err:.2e}")
    assert err <= ic.BOUND


def test_upsample_and_the_cell():
    g = ic.load("sources")
    for name, factor in g["cfg"]["rows"]["upsample"].items():
        got = ir.upsample(g[name + "_in"], factor)
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    c = ic.load("cell_ook")
    k = c["cfg"]["param"]
    assert np.array_equal(ir.upsample(c["symbTx"], k["SpS"]), c["symbolsUp"])
    assert c["sigTx"].dtype == np.complex128 and c["sigTxo"].dtype == np.complex128
    sig = ir.narrow(ir.shaped(c["symbTx"].real, c["pulse"], k["SpS"]))
    assert ic.rel_peak(sig, c["sigTx"].real) <= ic.BOUND
    Ai = np.sqrt(1e-3 * 10 ** (k["Pi_dBm"] / 10))
    assert ic.rel_peak(ir.narrow(ir.mzm(Ai, c["sigTx"], k["Vpi"], k["Vb"], 60)), c["sigTxo"]) <= ic.BOUND
