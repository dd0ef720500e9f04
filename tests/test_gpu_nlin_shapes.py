"""The perturbation-model kernels on the GPU at every shape of tests/nlin_shape_cases.py, held to the numpy restatement in both
precisions; and that the rows cover what that module's list claims."""
import numpy as np
import pytest

import nlin_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import _lib


@pytest.mark.gpu
@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_restatement(row):
    c = sc.make(row)
    Ci, Cx, Cs = c.mats
    for prec in (np.complex128, np.complex64):
        if row.mode == "AMR":
            got = oa.calcNLINperturbationSimplified(Ci, Cx, Cs, c.x, c.y, row.tol, prec)
            assert got[4] == c.plan["nReducedCoeffs"] == int(c.plan["keep"].sum())
        else:
            got = oa.calcNLINperturbation(Ci, Cx, Cs, c.x, c.y, prec)
        sc.check_calc(c, got[:4], prec)
        sc.check_nlin(c, oa.perturbationNLIN(c.Ein, sc.param(c, prec)), prec)


def test_rows_cover_what_the_list_claims():
    T, R = sc.T, sc.OUT
    by = {r.id: r for r in sc.ROWS}
    assert len(by) == len(sc.ROWS)
    shapes = {(r.N, r.L) for r in sc.ROWS}
    assert {1, 2, T - 1, T, T + 1, 2 * T + 1} <= {r.N for r in sc.ROWS}
    for f in (lambda L: L, lambda L: 2 * L, lambda L: 2 * L + 1):                   # the window wider than the signal
        assert any(N == f(L) for N, L in shapes)
    assert sum(r.N % R != 0 for r in sc.ROWS) >= 4
    assert {1, 2, 3, 4, 6, 7, _lib.NLIN_MAX_ORDER} <= {r.L for r in sc.ROWS} and (300, 128) in shapes
    assert {(2 * r.L + 1) % R for r in sc.ROWS} == {1, 3}                           # both remainders of the walk over n
    dense = [r for r in sc.ROWS if r.mode == "AM"]
    splits = {_lib.nlin_split(r.N, 2 * r.L + 3) for r in dense}
    assert {1, 2, 5, 15, _lib.NLIN_MAX_SPLIT} <= splits
    per_share = {(2 * r.L + 3) / _lib.nlin_split(r.N, 2 * r.L + 3) for r in dense}
    assert 1 in per_share and any(1 < v < 2 for v in per_share) and any(v >= 2 for v in per_share)   # one, one or two, more
    plans = {r.id: sc.make(r).plan for r in sc.ROWS if r.mode == "AMR"}
    empty = plans["amr_empty_groups"]
    assert 0 < len({int(m) for k, m, _, _ in empty["passes"] if k == 0}) < 2 * empty["L"] + 1
    assert len(plans["amr_single"]["coef"]) == 1 and plans["amr_single"]["nReducedCoeffs"] == 1
    every = plans["amr_everything"]
    assert every["nReducedCoeffs"] == (2 * every["L"] + 1) ** 2 - 1                 # all but the centre, which is zero
    assert any(r.mode == "AMR" and r.N == 1 for r in sc.ROWS)
    assert set(sc.EMU_ROWS) >= {r for r in sc.ROWS if r.N <= 2 * T + 3}
