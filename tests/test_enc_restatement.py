"""tests/enc_restatement.py against every encoder fixture (tests/golden/enc): the restatement the shape tests hold the kernels to
returns the reference's codewords and symbols, bit for bit."""
import numpy as np
import pytest

import enc_cases as ec
import enc_restatement as er


@pytest.mark.parametrize("name", sorted(ec.EXPECTED_CASES))
def test_restated_encoders_match_the_reference(name):
    g = ec.load(name)
    ec.check_conditions(g)
    c, bits = g["cfg"], g["bits"]
    k = bits.shape[0]
    if c["branch"] == "G":
        got = er.encode_generator(ec.unpacked(g, "G"), bits, True, c["n"])
        assert np.array_equal(er.encode_generator(ec.unpacked(g, "G"), bits, False, c["n"]), got)   # G = [I | P]: either way
    elif c["branch"] == "P1P2":
        got = er.encode_triang(ec.unpacked(g, "P1"), ec.unpacked(g, "P2"), bits)
    else:
        got = er.encode_dvbs2(ec.H_of(g).toarray()[:, :k], bits)
    assert got.dtype == np.uint8 and np.array_equal(got, g["codewords"])


@pytest.mark.parametrize("name", ec.MOD_CASES)
def test_restated_mapper_matches_the_reference(name):
    g = ec.load_mod(name)
    ec.check_mod_conditions(g)
    got = er.modulate(g["bits"], g["cfg"]["M"], g["cfg"]["constType"])
    assert got.dtype == g["symbols"].dtype and np.array_equal(got, g["symbols"])


def test_restated_tables_are_the_mapping_of_the_package():
    import opticommpy_amd as oa
    for M, ct in ((2, "psk"), (4, "qam"), (16, "qam"), (64, "qam"), (256, "qam"), (1024, "qam"), (8, "psk"), (4, "pam"), (8, "pam")):
        assert np.array_equal(er.gray_table(M, ct), oa.grayMapping(M, ct)), (M, ct)
