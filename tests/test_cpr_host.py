"""Host side of the carrier phase recovery (opticommpy_amd/cpr.py) without a GPU: what is out of scope is refused before the
library is even loaded, the constellation handed to the library equals the reference's bit for bit, and the shape rules hold."""
import numpy as np
import pytest

import cpr_cases as cc
import opticommpy_amd as oa
from opticommpy_amd import _lib
from opticommpy_amd import cpr as ocpr


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the checks under test come before it."""
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


X = (np.arange(64).reshape(32, 2) + 1j).astype(np.complex128)


def test_every_case_of_the_issue_has_a_fixture():
    assert cc.CASES == cc.EXPECTED_CASES
    for name in cc.CASES:
        cc.check_conditions(cc.load(name))


def test_public_names():
    assert oa.bpsGPU is oa.bps and callable(oa.cpr) and callable(oa.fourthPowerFOE)
    assert ocpr.cpr is not None and oa.cpr.bps is oa.bps
    for name in ("cpr", "bps", "bpsGPU", "fourthPowerFOE"):
        assert name in oa.__all__


@pytest.mark.parametrize("alg", ["ddpll", "viterbi"])
def test_serial_and_other_estimators_are_named_in_the_refusal(no_library, alg):
    with pytest.raises(ValueError, match="ddpll.*viterbi"):
        oa.cpr(X, cc.Param(alg=alg, M=16))


@pytest.mark.parametrize("kw", [
    dict(alg="pll"),
    dict(constType="pam"), dict(constType="apsk"),
    dict(M=3), dict(M=1), dict(M=2048), dict(M=12), dict(M=16.5),
    dict(M=2), dict(M=8), dict(M=32), dict(M=128), dict(M=512),            # non-square QAM
    dict(B=0), dict(B=-3), dict(B=1025),
    dict(N=2048), dict(N=-1),
])
def test_out_of_scope_parameters_raise_before_the_library_loads(no_library, kw):
    with pytest.raises(ValueError):
        oa.cpr(X, cc.Param(**dict(dict(M=16), **kw)))


def test_limits_that_must_work_are_inside_the_scope():
    assert ocpr.MAX_B >= 128 and ocpr.MAX_HALF_WINDOW >= 1023 // 2 and 2 * ocpr.MAX_HALF_WINDOW + 1 >= 1023 and ocpr.MAX_M >= 1024
    ocpr._check_search(1023 // 2, 128)
    assert ocpr._check_constellation(1024, "qam") == 1024 and ocpr._check_constellation(8, "psk") == 8
    assert ocpr._check_constellation(2, "psk") == 2


def test_signals_out_of_scope_raise_before_the_library_loads(no_library):
    table = ocpr._table(16, "qam", 0)
    for bad in (X[:1], X[:1, 0], np.zeros((0, 2), complex), np.zeros((4, 65), complex), np.zeros((4, 2, 2), complex), np.complex128(1)):
        with pytest.raises(ValueError):
            oa.cpr(bad, cc.Param(M=16))
        with pytest.raises(ValueError):
            oa.bps(bad, 3, table, 8)
        with pytest.raises(ValueError):
            oa.fourthPowerFOE(bad, 32e9)
    with pytest.raises(ValueError):
        oa.bps(X, 1024, table, 8)
    with pytest.raises(ValueError):
        oa.bps(X, 3, table, 0)
    with pytest.raises(ValueError):
        oa.bps(X, 3, table[:1], 8)
    with pytest.raises(ValueError):
        oa.fourthPowerFOE(X, 32e9, 0)
    with pytest.raises(ValueError):
        oa.fourthPowerFOE(X, 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32])
def test_device_arrays_of_another_dtype_raise_type_error(no_library, dtype):
    d = object.__new__(oa.DeviceArray)                      # (no GPU needed: the check is on the type)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (32, 2), np.dtype(dtype), 0, None, d
    with pytest.raises(TypeError, match="complex128 or complex64"):
        oa.cpr(d, cc.Param(M=16))
    with pytest.raises(TypeError):
        oa.bps(d, 3, ocpr._table(16, "qam", 0), 8)
    with pytest.raises(TypeError):
        oa.fourthPowerFOE(d, 32e9)


@pytest.mark.parametrize("name", cc.EXPECTED_CASES)
def test_table_is_the_references_bit_for_bit(name):
    g = cc.load(name)
    prm = g["cfg"]["param"]
    table = ocpr._table(prm["M"], prm.get("constType", "qam"), prm.get("shapingFactor", 0))
    assert table.dtype == np.complex64 == g["table"].dtype
    assert table.tobytes() == g["table"].tobytes()
    wide = ocpr._wide(table)
    assert wide.dtype == np.float64 and np.array_equal(wide.view(np.complex128), g["table"].astype(np.complex128))


def test_table_is_rebuilt_for_every_call():
    a = ocpr._table(16, "qam", 0)
    a[0] = 0
    assert ocpr._table(16, "qam", 0)[0] != 0


def test_shape_rules():
    x, n, modes = ocpr._signal(np.ones(10, np.complex64))
    assert (n, modes) == (10, 1) and x.dtype == np.complex64 and x.ndim == 1
    x, n, modes = ocpr._signal(np.ones((3, 8)))                       # no 'transposed' rule: 3 symbols of 8 modes
    assert (n, modes) == (3, 8) and x.dtype == np.complex128
    x, n, modes = ocpr._signal(np.ones((10, 1), np.complex128))
    assert (n, modes) == (10, 1) and x.ndim == 2
    x, n, modes = ocpr._signal([[1, 2], [3, 4]])
    assert (n, modes) == (2, 2) and x.dtype == np.complex128


def test_struct_layout_matches_the_header(tmp_path):
    """ssf_cpr_params as gcc lays it out against the ctypes mirror."""
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines = ['printf("size %zu\\n", sizeof(ssf_cpr_params));']
    for f, _ in _lib.CprParams._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(ssf_cpr_params, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    (tmp_path / "layout.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.CprParams)
    for f, _ in _lib.CprParams._fields_:
        assert int(got[f]) == getattr(_lib.CprParams, f).offset, f


def test_library_refuses_bad_arguments_without_a_device():
    """The C ABI's own checks come before any allocation or launch: they answer on a box without a GPU."""
    import ctypes as C
    lib = _lib.load()
    tab = ocpr._wide(ocpr._table(16, "qam", 0))
    tp = tab.ctypes.data_as(C.POINTER(C.c_double))
    x = np.ascontiguousarray(X)
    out = np.empty_like(x)
    ph = np.empty(x.shape)
    fo = np.zeros(2)
    xp, op, pp, fp = (a.ctypes.data_as(C.c_void_p) for a in (x, out, ph, fo))
    good = dict(n=32, nModes=2, M=16, dtype=0, B=64, Nh=17, runFOE=1, P=4, Fs=32e9)
    for bad in (dict(n=1), dict(nModes=0), dict(nModes=65), dict(M=1), dict(M=1025), dict(dtype=2), dict(B=0), dict(B=1025), dict(Nh=-1),
                dict(Nh=1024), dict(P=0), dict(Fs=0.0)):
        p = _lib.CprParams(**dict(good, **bad))
        assert lib.ssf_cpr(0, C.byref(p), tp, xp, op, None, None) == -1, bad
    assert lib.ssf_cpr(0, None, tp, xp, op, None, None) == -1
    assert lib.ssf_bps(0, 32, 2, 0, 1024, 64, 16, tp, xp, pp) == -1
    assert lib.ssf_bps(0, 32, 2, 0, 17, 64, 16, tp, xp, None) == -1
    assert lib.ssf_foe(0, 32, 2, 0, 0, 32e9, xp, op, fo.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert lib.ssf_foe(0, 1, 2, 0, 4, 32e9, xp, op, fo.ctypes.data_as(C.POINTER(C.c_double))) == -1
    assert b"ssf_foe" in lib.ssf_last_error(None)
