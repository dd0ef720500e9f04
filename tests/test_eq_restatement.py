"""The numpy restatement of the adaptive equalizer (tests/eq_restatement.py) against every fixture of the reference, at the
bounds of the GPU test: sigOut and H within 1e-9 (rel-L2 and per element against max |ref|), errSq within 1e-9 of max |ref|.
`default_prec` holds two runs of the reference on one complex64 input: the one with prec = complex128 is matched with
prec = complex128 at those bounds, the one with prec left at complex64 -- whose constellation is rounded to single precision,
3e-8 away from the other's -- with prec left alone, within twice the reference's own distance between the two."""
import numpy as np
import pytest

import eq_cases as ec
import eq_restatement as er


@pytest.mark.parametrize("name", ec.EXPECTED_CASES)
def test_restatement_matches_the_reference(name):
    g = ec.load(name)
    ec.check_conditions(g)
    x0, r0 = g["sigIn"].copy(), g["symbRef"].copy()
    sigOut, H, errSq, gap = er.restate(g["sigIn"], ec.param128(g), g["symbRef"])
    assert np.array_equal(g["sigIn"], x0) and np.array_equal(g["symbRef"], r0)
    assert sigOut.shape == g["sigOut"].shape
    ec.compare_results(sigOut, H, errSq, g, name, static_from=ec.static_start(g))
    if any(a in ec.DECIDING for a in g["cfg"]["alg"]):
        print(f"{name}: smallest decision gap over all updates {gap:.2e}")
        assert gap >= 1e-7            # every pass of stage 0 counted, not only the stored one: no decision hangs on a rounding


def test_default_prec_restatement_is_as_far_from_the_single_precision_run_as_the_reference_itself():
    g = ec.load("default_prec")
    sigOut, H, errSq, _ = er.restate(g["sigIn"], ec.param(g), g["symbRef"])
    d = ec.rel_l2(sigOut, g["sigOut64"].astype(np.complex128))
    print(f"default_prec: distance to the complex64 run {d:.2e}, the reference's own {float(g['self_err']):.2e}")
    assert d <= 2 * float(g["self_err"])
