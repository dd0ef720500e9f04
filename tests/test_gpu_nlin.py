"""The perturbation model on the GPU against every reference-generated fixture: the three entry points on numpy arrays and on
DeviceArrays, complex128 and complex64 inputs, both values of prec, at the bounds of tests/nlin_cases.py; a second call bit-equal
to the first; inputs unchanged; and modulateGray -> pnorm -> perturbationNLIN kept on the device."""
import numpy as np
import pytest

import nlin_cases as nc
import opticommpy_amd as oa
from opticommpy_amd import device as dev

pytestmark = pytest.mark.gpu
PRECS = (np.complex128, np.complex64)


def _calc(g, x, y, prec):
    """The fixture's calculation: (dx, dy, phi_x, phi_y) and, 'AMR', the two counts."""
    if nc.mode(g) == "AMR":
        out = oa.calcNLINperturbationSimplified(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], x, y, nc.coeff_tol(g), prec)
        assert out[4] == int(g["nReducedCoeffs"]) and out[5] == float(g["reductionFactor"])
        return out[:4]
    return oa.calcNLINperturbation(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], x, y, prec)


@pytest.mark.parametrize("single_in", [False, True], ids=["c128", "c64"])
@pytest.mark.parametrize("name", nc.CASES)
def test_calculation_matches_the_reference(name, single_in):
    g = nc.load(name)
    nc.check_conditions(g)
    dtype = np.complex64 if single_in else np.complex128
    x, y = g["x"].astype(dtype), g["y"].astype(dtype)
    for prec in PRECS:
        got = _calc(g, x, y, prec)
        assert all(isinstance(v, np.ndarray) for v in got)
        nc.check_calc(g, got, prec, single_in)
        again = _calc(g, x, y, prec)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))               # fixed order: bit for bit
        xd, yd = oa.to_device(x), oa.to_device(y)
        before = dev.transfer_counts()
        on_dev = _calc(g, xd, yd, prec)
        assert dev.transfer_counts() == before                                      # nothing but a status leaves the GPU
        assert all(dev.is_device(v) for v in on_dev)
        assert all(np.array_equal(a, b.get()) for a, b in zip(got, on_dev))
        assert np.array_equal(xd.get(), x) and np.array_equal(yd.get(), y)
    assert np.array_equal(x, g["x"].astype(dtype)) and np.array_equal(y, g["y"].astype(dtype))


@pytest.mark.parametrize("single_in", [False, True], ids=["c128", "c64"])
@pytest.mark.parametrize("name", nc.CASES)
def test_field_matches_the_reference(name, single_in):
    g = nc.load(name)
    E = g["Ein"].astype(np.complex64 if single_in else np.complex128)
    keep = E.copy()
    for prec in PRECS:
        got = oa.perturbationNLIN(E, nc.param(g, prec))
        assert isinstance(got, np.ndarray) and np.array_equal(E, keep)             # unlike the reference: Ein is never written
        nc.check_nlin(g, got, prec, single_in)
        assert np.array_equal(got, oa.perturbationNLIN(E, nc.param(g, prec)))
        Ed = oa.to_device(E)
        before = dev.transfer_counts()
        on_dev = oa.perturbationNLIN(Ed, nc.param(g, prec))
        assert dev.transfer_counts() == before and dev.is_device(on_dev) and on_dev.dtype == E.dtype and on_dev.shape == E.shape
        assert np.array_equal(on_dev.get(), got) and np.array_equal(Ed.get(), keep)


def test_everything_kept_is_the_full_model_with_other_phases():
    g = nc.load("amr_all")
    full = oa.calcNLINperturbation(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], g["x"], g["y"], np.complex128)
    kept = oa.calcNLINperturbationSimplified(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], g["x"], g["y"], -400, np.complex128)
    assert nc.rel(full[0], kept[0]) <= nc.TOL128 and nc.rel(full[1], kept[1]) <= nc.TOL128
    assert nc.rel(full[2], kept[2]) > 1e-3


def test_device_arrays_of_another_kind_are_refused():
    g = nc.load("am_l3")
    with pytest.raises(TypeError):
        oa.perturbationNLIN(oa.to_device(g["Ein"].real.copy()), nc.param(g))
    with pytest.raises(ValueError):
        oa.calcNLINperturbation(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], oa.to_device(g["x"]), g["y"])
    with pytest.raises(TypeError):
        oa.calcNLINperturbation(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], oa.to_device(g["x"]), oa.to_device(g["y"].astype(np.complex64)))


def test_the_library_checks_the_tables_itself():
    """A plan whose entries point outside the window never reaches a kernel."""
    import ctypes as C
    from opticommpy_amd import _lib, perturbation as pt
    g = nc.load("am_l3")
    q = pt._prepare_calc(g["C_ifwm"], g["C_ixpm"], g["C_ispm"], g["x"], g["y"], np.complex128, "AMR", -20)
    plan = q["plan"]
    lib = _lib.load()
    n = q["n"]
    outs = [np.empty(n, dtype=np.complex128), np.empty(n, dtype=np.complex128), np.empty(n), np.empty(n)]

    def call(passes=plan["passes"], nidx=plan["nidx"], phase_m=plan["phase_m"], **kw):
        p = pt._params(q)
        p.plan_key = 0
        for k, v in kw.items():
            setattr(p, k, v)
        passes, nidx, phase_m = (np.ascontiguousarray(a, dtype=np.int32) for a in (passes, nidx, phase_m))
        ip = C.POINTER(C.c_int32)
        return lib.ssf_pert_nlin(0, C.byref(p), passes.ctypes.data_as(ip), plan["coef"].ctypes.data_as(C.c_void_p), nidx.ctypes.data_as(ip),
                                 phase_m.ctypes.data_as(ip), plan["phase_c"].ctypes.data_as(C.c_void_p), q["x"].ctypes.data_as(C.c_void_p),
                                 q["y"].ctypes.data_as(C.c_void_p), *[o.ctypes.data_as(C.c_void_p) for o in outs])
    assert call() == 0
    L = plan["L"]
    bad = plan["passes"].copy()
    bad[0, 1] = L + 1
    assert call(passes=bad) == -1
    bad = plan["passes"].copy()
    bad[-1, 3] += 1
    assert call(passes=bad) == -1
    bad = plan["nidx"].copy()
    bad[0] = -L - 1
    assert call(nidx=bad) == -1
    bad = plan["phase_m"].copy()
    bad[0] = L + 1
    assert call(phase_m=bad) == -1
    # more coefficients in a pass than its slice of LDS holds (an n repeated), and a pass whose n do not rise
    W = 2 * L + 1
    coef = np.ones(W + 1, dtype=np.complex128)
    ip = C.POINTER(C.c_int32)

    def one_pass(n_list):
        p = pt._params(q)
        p.plan_key, p.npass, p.ncoef, p.nphase = 0, 1, len(n_list), 0
        passes = np.array([[0, 1, 0, len(n_list)]], dtype=np.int32)
        nidx = np.array(n_list, dtype=np.int32)
        return lib.ssf_pert_nlin(0, C.byref(p), passes.ctypes.data_as(ip), coef.ctypes.data_as(C.c_void_p), nidx.ctypes.data_as(ip), None, None,
                                 q["x"].ctypes.data_as(C.c_void_p), q["y"].ctypes.data_as(C.c_void_p), *[o.ctypes.data_as(C.c_void_p) for o in outs])
    assert one_pass(list(range(-L, L + 1))) == 0
    assert one_pass(list(range(-L, L + 1)) + [L]) == -1
    assert one_pass([0] * (W + 1)) == -1 and one_pass([1, 0]) == -1 and one_pass([0, 0]) == -1
    assert call(L=0) == -1 and call(L=129) == -1 and call(n=0) == -1 and call(ispm_offset=L + 1) == -1 and call(dense=1) == -1
    assert call(prec=7) == -1 and call(entry=2) == -1


def test_modulated_symbols_stay_on_the_device():
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, 4 * 600 * 2).astype(np.uint8)
    p = nc.Param(matrixOrder=5, Pin=2, mode="AMR", coeffTol=-25)
    symb = oa.pnorm(oa.modulateGray(bits, 16, "qam")).reshape(600, 2)
    want = oa.perturbationNLIN(symb, nc.Param(**vars(p)))
    bd = oa.to_device(bits)
    before = dev.transfer_counts()
    sd = oa.pnorm(oa.modulateGray(bd, 16, "qam")).reshape(600, 2)
    got = oa.perturbationNLIN(sd, nc.Param(**vars(p)))
    assert dev.transfer_counts() == before and dev.is_device(got) and got.shape == (600, 2) and got.dtype == np.complex128
    assert np.array_equal(got.get(), want) and np.max(np.abs(want)) > 0
