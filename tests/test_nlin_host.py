"""The host side of the perturbation model without a device: the coefficient matrices against the reference's, every ValueError
before anything runs, the 'AMR' selection and its grouping per m, plan caching, and that the input is never written."""
import ast
import os

import numpy as np
import pytest

import nlin_cases as nc
import nlin_restatement as rs
import opticommpy_amd as oa
from opticommpy_amd import _lib
from opticommpy_amd import perturbation as pt


@pytest.mark.parametrize("name", nc.CASES)
def test_coefficient_matrices_match_the_reference(name):
    g = nc.load(name)
    p = nc.param(g)
    p.Fc = 193.1e12                                 # perturbationNLIN's default, under which the fixtures were made
    C, Ci, Cx, Cs = pt.calcPertCoeffMatrix(p)
    ref = nc.full_matrix(g)
    ref[-1, -1] = g["C_ifwm"][-1, -1]
    W = ref.shape[0]
    ref[W // 2, W // 2] = g["C_ispm"]               # calcPertCoeffMatrix's own C carries C_ispm at the centre
    top = np.max(np.abs(nc.full_matrix(g)))
    for got, want in ((C, ref), (Ci, g["C_ifwm"]), (Cx, g["C_ixpm"]), (np.array([Cs]), np.array([g["C_ispm"]]))):
        assert got.shape == want.shape and np.max(np.abs(got - want)) / top <= nc.TOL128
    assert isinstance(Cs, complex) and Ci.flags.writeable


def test_exp1_on_both_axes():
    # E1(1) and E1(10) (Abramowitz & Stegun, table 5.1); E1(-j a) = -Ci(a) + j (pi / 2 - Si(a)) with Si(1), Ci(1), Si(10), Ci(10)
    got = pt.exp1(np.array([1.0, 10.0, -1j, -10j, 1j, 0.0]))
    want = [0.21938393439552029, 4.156968929685324e-06, -0.33740392290096813 + 1j * (np.pi / 2 - 0.94608307036718301),
            0.045456433004455373 + 1j * (np.pi / 2 - 1.6583475942188740)]
    for a, b in zip(got[:4], want):
        assert abs(a - b) <= 1e-14 * max(1.0, abs(b)), (a, b)
    assert got[4] == np.conj(got[2]) and np.isinf(got[5])
    # the two evaluations meet at |z| = 4
    lo, hi = pt.exp1(np.array([-4j])), pt.exp1(np.array([-4j * (1 + 1e-15)]))
    assert abs(lo[0] - hi[0]) <= 1e-14


def test_the_product_path_imports_no_scipy():
    src = open(os.path.join(nc.ROOT, "opticommpy_amd", "perturbation.py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.module:
            names.add(node.module.split(".")[0])
    assert "scipy" not in names and "numpy" in names


def test_the_four_functions_are_exported():
    for k in ("calcPertCoeffMatrix", "calcNLINperturbation", "calcNLINperturbationSimplified", "perturbationNLIN"):
        assert getattr(oa, k) is getattr(pt, k) and k in oa.__all__


def _mats(L=2):
    _, Ci, Cx, Cs = pt.calcPertCoeffMatrix(nc.Param(matrixOrder=L))
    return Ci, Cx, Cs


def test_errors_are_raised_before_anything_runs(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", no_library)
    E = np.ones((8, 2), dtype=complex)
    x = np.ones(8, dtype=complex)
    Ci, Cx, Cs = _mats()
    bad_params = [dict(powerWeighted=True), dict(matrixOrder=0), dict(matrixOrder=-3), dict(matrixOrder=129), dict(matrixOrder=2.5),
                  dict(mode="AMX"), dict(mode="am"), dict(prec=np.float64), dict(prec=np.complex256 if hasattr(np, "complex256") else "c32"),
                  dict(mode="AMR", coeffTol=0.0), dict(mode="AMR", coeffTol=float("nan"))]
    for kw in bad_params:
        prm = nc.Param(**kw)
        with pytest.raises(ValueError):
            oa.perturbationNLIN(E.copy(), prm)
        assert vars(prm) == kw                      # a call that raises writes no default into param
    for bad in (np.ones(8, dtype=complex), np.ones((8, 3), dtype=complex), np.ones((2, 8), dtype=complex), np.ones((0, 2), dtype=complex),
                np.ones((4, 2, 1), dtype=complex)):
        with pytest.raises(ValueError):
            oa.perturbationNLIN(bad, nc.Param())
    for kw in (dict(powerWeighted=True), dict(matrixOrder=0), dict(matrixOrder=129)):
        with pytest.raises(ValueError):
            oa.calcPertCoeffMatrix(nc.Param(**kw))
    with pytest.raises(ValueError):
        oa.calcNLINperturbation(Ci, Cx, Cs, x, x[:-1])
    with pytest.raises(ValueError):
        oa.calcNLINperturbation(Ci, Cx, Cs, x.reshape(4, 2), x.reshape(4, 2))
    with pytest.raises(ValueError):
        oa.calcNLINperturbation(Ci, Cx, Cs, x[:0], x[:0])
    with pytest.raises(ValueError):
        oa.calcNLINperturbation(Ci, Cx, Cs, x, x, prec=np.float32)
    with pytest.raises(ValueError):
        oa.calcNLINperturbationSimplified(Ci, Cx, Cs, x, x, coeffTol=-20, prec=np.int32)
    with pytest.raises(ValueError):
        oa.calcNLINperturbationSimplified(Ci, Cx, Cs, x, x, coeffTol=1.0)
    nan, inf = Ci.copy(), Cx.copy()
    nan[0, 0], inf[1, 1] = np.nan, np.inf
    for A, B, s in ((nan, Cx, Cs), (Ci, inf, Cs), (Ci, Cx, np.inf), (Ci[:, :-1], Cx[:, :-1], Cs), (Ci[:-1, :-1], Cx[:-1, :-1], Cs),
                    (Ci, Cx[:3, :3], Cs), (Ci[2:3, 2:3], Cx[2:3, 2:3], Cs), (Ci.flatten(), Cx.flatten(), Cs),
                    (np.zeros((259, 259)), np.zeros((259, 259)), Cs)):
        with pytest.raises(ValueError):
            oa.calcNLINperturbation(A, B, s, x, x)


def test_preparation_leaves_the_input_alone_and_writes_the_defaults():
    g = nc.load("am_l3")
    E = g["Ein"].copy()
    p = nc.Param(matrixOrder=3)
    q = pt._prepare_nlin(E, p)
    assert np.array_equal(E, g["Ein"]) and q["x"].dtype == np.complex128 and q["n"] == len(E) and q["entry"] == _lib.NLIN_FIELD
    assert (p.D, p.alpha, p.lspan, p.length, p.pulseWidth, p.gamma, p.Fc, p.powerWeighted, p.Rs, p.powerWeightN, p.matrixOrder) == \
        (17, 0.2, 50, 800, 0.5, 1.3, 193.1e12, False, 32e9, 10, 3)
    assert q["peak"] == 0.5e-3 and q["prec"] == np.complex128
    q = pt._prepare_nlin(E.astype(np.complex64), nc.Param(matrixOrder=3, Pin=3, prec=np.complex64))
    assert q["x"].dtype == np.complex64 and q["prec"] == np.complex64 and abs(q["peak"] - 0.5e-3 * 10 ** 0.3) < 1e-18


@pytest.mark.parametrize("name", nc.CASES)
def test_plan_reproduces_the_kept_coefficients(name):
    """Scattering the passes back gives C_ifwm (and the centre column and row of C_ixpm) on the kept set and nothing elsewhere."""
    g = nc.load(name)
    amr = nc.mode(g) == "AMR"
    plan = pt._coeff_plan(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], nc.mode(g), nc.coeff_tol(g) if amr else None)
    L = plan["L"]
    W = 2 * L + 1
    if amr:
        keep, n, factor, off = rs.select(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], nc.coeff_tol(g))
        assert plan["nReducedCoeffs"] == n == int(g["nReducedCoeffs"]) and plan["reductionFactor"] == factor == float(g["reductionFactor"])
        assert np.array_equal(plan["keep"], keep) and plan["ispm_offset"] == off == L and not plan["dense"]
    else:
        keep = np.ones((W, W), dtype=bool)
        assert plan["ispm_offset"] == -L and plan["dense"] and len(plan["passes"]) == W + 2
    ifwm, col = np.zeros((W, W), dtype=complex), {1: np.zeros(W, dtype=complex), 2: np.zeros(W, dtype=complex)}
    seen = set()
    for kind, m, first, count in plan["passes"]:
        assert count >= 1 and (kind, m) not in seen and (kind == 0 or m == 0)
        seen.add((kind, m))
        n = plan["nidx"][first:first + count]
        assert np.all(np.diff(n) > 0) and n[0] >= -L and n[-1] <= L                   # by rising n, each once
        if plan["dense"]:
            assert np.array_equal(n, np.arange(-L, L + 1))
        if kind == 0:
            ifwm[L - n, L + m] = plan["coef"][first:first + count]
        else:
            col[kind][L - n] = plan["coef"][first:first + count]
    assert np.array_equal(ifwm, np.where(keep, g["C_ifwm"], 0))
    want_col = np.where(keep[:, L], g["C_ixpm"][:, L], 0)
    assert np.array_equal(col[1], want_col) and np.array_equal(col[2], want_col)
    row = np.zeros(W, dtype=complex)
    row[plan["phase_m"] + L] = plan["phase_c"]
    assert np.array_equal(row, np.where(keep[L], g["C_ixpm"][L], 0)) and len(set(plan["phase_m"].tolist())) == len(plan["phase_m"])
    assert plan["ispm"] == g["C_ispm"]
    if amr:                                           # no pass without a coefficient, no zero coefficient carried along
        assert np.all(plan["coef"] != 0) and np.all(plan["phase_c"] != 0)


def test_amr_plans_leave_out_empty_groups_and_can_hold_one_coefficient():
    g = nc.load("amr_default")
    plan = pt._coeff_plan(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], "AMR", -20)
    ms = {int(m) for kind, m, _, _ in plan["passes"] if kind == 0}
    assert 0 < len(ms) < 2 * plan["L"] + 1                                           # some m have no coefficient left
    g = nc.load("amr_corner")
    plan = pt._coeff_plan(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], "AMR", -0.1)
    L = plan["L"]
    assert plan["nReducedCoeffs"] == 1 and plan["passes"].tolist() == [[0, L, 0, 1]] and plan["nidx"].tolist() == [-L]
    assert plan["coef"][0] == g["C_ifwm"][2 * L, 2 * L] and len(plan["phase_m"]) == 0


def test_plans_and_matrices_are_cached_by_content():
    pt.release_plans()
    assert pt.plan_cache_info() == []
    Ci, Cx, Cs = _mats(3)
    a = pt._coeff_plan(Ci, Cx, Cs, "AM", None)
    b = pt._coeff_plan(Ci.copy(), Cx.copy(), complex(Cs), "AM", None)               # other arrays, the same content
    assert a is b and len(pt.plan_cache_info()) == 1
    c = pt._coeff_plan(Ci, Cx, Cs, "AMR", -20)
    d = pt._coeff_plan(Ci, Cx, Cs, "AMR", -30)
    assert len({a["key"], c["key"], d["key"]}) == 3 and len(pt.plan_cache_info()) == 3
    Ci2 = Ci.copy()
    Ci2[0, 0] *= 1 + 1e-15
    assert pt._coeff_plan(Ci2, Cx, Cs, "AM", None)["key"] not in (a["key"], c["key"], d["key"])
    for k in range(12):                                                              # the cache is bounded
        pt._coeff_plan(Ci * (k + 2), Cx, Cs, "AM", None)
    assert len(pt.plan_cache_info()) <= 8
    assert not a["coef"].flags.writeable
    # the matrices: one computation per parameter set, fresh arrays per call
    p = nc.Param(matrixOrder=3)
    first = pt._coeff_matrices(p)
    assert pt._coeff_matrices(nc.Param(matrixOrder=3, D=17.0)) is first and pt._coeff_matrices(nc.Param(matrixOrder=3, D=16)) is not first
    m1, m2 = pt.calcPertCoeffMatrix(p), pt.calcPertCoeffMatrix(p)
    assert m1[1] is not m2[1] and np.array_equal(m1[1], m2[1])
    m1[1][0, 0] = 0
    assert pt.calcPertCoeffMatrix(p)[1][0, 0] != 0
    pt.release_plans()


def test_launch_geometry_is_the_kernels():
    src = open(os.path.join(nc.ROOT, "opticommpy_amd", "csrc", "nlin_kernels.h")).read()
    for name, value in (("kMaxL", _lib.NLIN_MAX_ORDER), ("kOut", _lib.NLIN_OUT), ("kMaxSplit", _lib.NLIN_MAX_SPLIT),
                        ("kTargetGroups", _lib.NLIN_TARGET_GROUPS)):
        assert f"{name} = {value}" in src, name
    assert "kLanes = 64" in src and _lib.NLIN_TILE == 64 * _lib.NLIN_OUT and pt.MAX_ORDER == _lib.NLIN_MAX_ORDER
    assert [_lib.nlin_split(n, 5) for n in (1, 128 * 256, 128 * 256 + 1, 1024 * 256 + 1, 2048 * 256 + 1)] == [5, 5, 5, 2, 1]
    assert _lib.nlin_split(300, 259) == 16 and _lib.nlin_split(300, 0) == 0
