"""tests/fec_restatement.py pinned to the reference's recorded results (tests/golden/fec, tools/gen_golden_fec.py): min-sum
bit-equal in both precisions, sum-product -- the same ordered product as the reference's -- at the bounds of tests/fec_cases.py,
the edge maps equal to those the reference builds, calcLLR at its bound.  The GPU tests then use the restatement for graphs too
large to store."""
import numpy as np
import pytest

import fec_cases as fc
import fec_restatement as fr


def test_the_fixture_set_is_complete():
    assert fc.CASES == fc.EXPECTED_CASES
    for name in fc.EXPECTED_CASES:
        fc.check_conditions(fc.load(name))
    fc.check_set()
    precs = [fc.load(n)["cfg"]["prec"] for n in fc.EXPECTED_CASES]
    assert precs.count("float32") == 1
    for name in fc.LLR_CASES:
        g = fc.load_llr(name)
        assert np.any(np.isinf(g["llr"])) == name.endswith("underflow") and not np.any(np.isnan(g["llr"]))
    assert not np.allclose(fc.load_llr("qam64_shaped")["px"], 1 / 64)


@pytest.mark.parametrize("name", fc.EXPECTED_CASES)
def test_restatement_matches_the_reference(name):
    g = fc.load(name)
    for prec in fc.PRECS:
        got = fr.decode(g["indptr"], g["indices"], g["shape"], g["llrs"], g["cfg"]["alg"], g["cfg"]["maxIter"], prec)
        fc.compare_decode(got, g, prec, f"{name} [{prec}]")


@pytest.mark.parametrize("name", fc.EDGE_CASES)
def test_restatement_matches_the_reference_on_a_check_of_degree_one(name):
    """The m = 12, n = 24 graph with a check of degree 1 and a variable of degree 0.  Min-sum sends +-inf from that check and gets
    inf - inf = NaN back, whose sign the reference takes as negative (fec.py:609, 622: ``1 if val >= 0 else -1``): with NaN taken
    as positive the posterior of that variable is -inf instead of +inf from the second iteration on, and codewords 0 and 2 of the
    min-sum fixture never converge."""
    g = fc.load(name)
    dc, dv = np.diff(g["indptr"]), np.bincount(g["indices"], minlength=int(g["shape"][1]))
    assert tuple(g["shape"]) == (12, 24) and np.sum(dc == 1) == 1 and np.sum(dv == 0) == 1 and g["llrs"].shape == (24, 4)
    assert g["cfg"]["maxIter"] == 6 and np.any((g["fail64"] == 0) & (g["iter64"] > 0)) and 0 < g["fail64"].sum() < 4
    assert np.array_equal(g["fail32"], g["fail64"]) and np.array_equal(g["iter32"], g["iter64"])
    assert np.array_equal(np.isnan(g["out32"]), np.isnan(g["out64"]))
    assert np.array_equal(g["bits32"][~np.isnan(g["out64"])], g["bits64"][~np.isnan(g["out64"])])
    inf = g["cfg"]["alg"] == "MSA"
    assert np.any(np.isinf(g["out64"])) == inf and np.any(np.isinf(g["out32"])) == inf
    for prec in fc.PRECS:
        with np.errstate(invalid="ignore"):
            got = fr.decode(g["indptr"], g["indices"], g["shape"], g["llrs"], g["cfg"]["alg"], 6, prec)
        fc.compare_decode(got, g, prec, f"{name} [{prec}]", nan=inf)


@pytest.mark.parametrize("key", fc.GRAPHS)
def test_restated_edge_maps_are_the_references(key):
    z = fc.load_graph(key)
    co, vo, ve = fr.edge_maps(z["indptr"], z["indices"], int(z["shape"][1]))
    assert np.array_equal(co, z["check_offsets"]) and np.array_equal(vo, z["var_offsets"]) and np.array_equal(ve, z["var_edge_indices"])


@pytest.mark.parametrize("name", fc.LLR_CASES)
def test_restated_llr_matches_the_reference(name):
    g = fc.load_llr(name)
    fc.compare_llr(fr.calc_llr(g["rxSymb"], g["sigma2"], g["constSymb"], g["bitMap"], g["px"]), g, name)
