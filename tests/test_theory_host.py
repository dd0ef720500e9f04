"""Host side of the theoretical MI (no GPU): every refusal of opticommpy_amd.theory comes before the library is loaded, the table
handed down is the reference's bit for bit, result types, public names, the ctypes prototypes against include/ssf.h and the C ABI's
rejection of bad arguments before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import opticommpy_amd as oa
import theory_cases as tc
from opticommpy_amd import _lib
from opticommpy_amd import theory as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("theoryMI", "constellationMI", "calcMI", "condEntropy", "GN_Model_NyquistWDM", "ASE_NyquistWDM", "GNmodel_OSNR", "calcLinOSNR")


def test_public_names():
    from opticommpy_amd.metrics import GNmodel_OSNR, calcLinOSNR, calcMI, theoryMI
    assert theoryMI is oa.theoryMI and calcMI is oa.calcMI and GNmodel_OSNR is oa.GNmodel_OSNR and calcLinOSNR is oa.calcLinOSNR
    for name in NAMES:
        assert callable(getattr(oa, name)) and name in oa.__all__ and name in oa.metrics.__all__ and name in th.__all__
    for words in ("4.70459", "4.68143", "symmetry", "1e-10"):          # the deviations are stated, with their numbers
        assert words in th.__doc__


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def test_every_refusal_comes_before_the_library(no_library):
    bad = [lambda: oa.theoryMI(16, "apsk", 10), lambda: oa.theoryMI(32, "qam", 10), lambda: oa.theoryMI(2048, "qam", 10),
           lambda: oa.theoryMI(12, "psk", 10), lambda: oa.theoryMI(16, "qam", 10, lim=5), lambda: oa.theoryMI(16, "qam", 10, lim=-np.inf),
           lambda: oa.theoryMI(16, "qam", 10, tol=1e-11), lambda: oa.theoryMI(16, "qam", 10, tol=0), lambda: oa.theoryMI(16, "qam", 10, tol=np.nan),
           lambda: oa.theoryMI(16, "qam", 10, pX=np.ones(8) / 8), lambda: oa.theoryMI(4, "qam", 10, pX=[0.5, 0.5, 0.0, 0.0]),
           lambda: oa.theoryMI(4, "qam", 10, pX=[0.5, 0.5, np.nan, 0.1]), lambda: oa.theoryMI(4, "qam", 10, pX=[0.5, 0.7, -0.2, 0.1]),
           lambda: oa.theoryMI(4, "qam", 10, pX=[0.5, 0.5, np.inf, 0.1]),
           lambda: oa.theoryMI(16, "qam", np.zeros(4097)), lambda: oa.theoryMI(16, "qam", np.zeros((2, 2))), lambda: oa.theoryMI(16, "qam", []),
           lambda: oa.theoryMI(16, "qam", np.nan), lambda: oa.theoryMI(16, "qam", 1e5),
           lambda: oa.constellationMI([], 10), lambda: oa.constellationMI(np.ones(1025), 10), lambda: oa.constellationMI(np.ones((2, 2)), 10),
           lambda: oa.constellationMI([1.0, np.inf], 10), lambda: oa.constellationMI([1.0, -1.0], 10, pX=[1.0]),
           lambda: oa.calcMI(np.ones(4), np.ones(4), 0.0, [1.0, -1.0], [0.5, 0.5]), lambda: oa.calcMI(np.ones(4), np.ones(4), -1.0, [1.0, -1.0], [0.5, 0.5]),
           lambda: oa.calcMI(np.ones(4), np.ones(4), 0.1, [1.0, -1.0], [1.0]), lambda: oa.calcMI(np.ones(4), np.ones(5), 0.1, [1.0, -1.0], [0.5, 0.5]),
           lambda: oa.calcMI(np.ones((4, 1)), np.ones((4, 1)), 0.1, [1.0, -1.0], [0.5, 0.5]), lambda: oa.calcMI([], [], 0.1, [1.0, -1.0], [0.5, 0.5]),
           lambda: oa.calcMI(np.ones(4), np.ones(4), 0.1, np.ones(1025), np.ones(1025) / 1025)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")
    with pytest.raises(AssertionError, match="the library was loaded"):    # a good call does reach it
        oa.theoryMI(16, "qam", 10, tol=1e-10, symmetry=False)


@pytest.fixture
def captured(monkeypatch):
    seen = []

    def fake(table, pX, sigma):
        seen.append((table, pX, sigma))
        return np.arange(sigma.shape[0], dtype=np.float64)
    monkeypatch.setattr(th, "_integrate", fake)
    return seen


@pytest.mark.parametrize("name", list(tc.MI_CASES))
def test_what_is_handed_down_equals_the_references(captured, name):
    g = tc.load(name)
    c = g["cfg"]
    oa.theoryMI(c["M"], c["constType"], c["SNR"], pX=None if c["px"] is None else g["px"])
    table, pX, sigma = captured[0]
    assert table.dtype == np.complex128 and table.flags.c_contiguous and np.array_equal(table, g["table"])
    assert np.array_equal(table, table.astype(np.complex64).astype(np.complex128))      # single precision through the normalisation
    assert pX.dtype == np.float64 and np.array_equal(pX, g["px"])
    assert sigma.shape == (1,) and sigma[0] == float(g["sigma"])


def test_result_types(captured):
    assert type(oa.theoryMI(16, "qam", 10)) is float and type(oa.theoryMI(16, "qam", np.float32(10))) is float
    r = oa.theoryMI(16, "qam", np.arange(-2, 35, 1))
    assert isinstance(r, np.ndarray) and r.shape == (37,) and r.dtype == np.float64
    assert oa.theoryMI(16, "qam", [10.0]).shape == (1,)
    assert type(oa.constellationMI([1.0, -1.0], 3)) is float and oa.constellationMI([1 + 1j, -1j], [3, 4]).shape == (2,)
    table, pX, sigma = captured[-1]
    assert np.array_equal(table, np.array([1 + 1j, -1j])) and np.array_equal(pX, [0.5, 0.5])      # used as given
    assert np.array_equal(sigma, np.sqrt((1 / 2) * 1 / (10 ** (np.array([3.0, 4.0]) / 10))))
    oa.theoryMI(4, "qam", 5, symmetry=True)
    oa.theoryMI(4, "qam", 5, symmetry=False, tol=0.5)
    assert all(np.array_equal(a, b) for a, b in zip(captured[-1], captured[-2]))                   # symmetry and tol change nothing


_CTYPES = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "const double *": C.POINTER(C.c_double),
           "double *": C.POINTER(C.c_double), "const void *": C.c_void_p}


@pytest.mark.parametrize("name", ["ssf_theory_mi", "ssf_calc_mi"])
def test_prototypes_match_the_header(name):
    header = " ".join(open(os.path.join(ROOT, "include", "ssf.h")).read().split())
    m = re.search(rf"\bint {name}\(([^)]*)\);", header)
    assert m, name
    want = []
    for arg in m.group(1).split(","):
        ctype = re.sub(r"\s*\w+$", "", arg.strip())            # drop the parameter's name
        want.append(_CTYPES[ctype.strip()])
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int and args == want


def test_the_rule_is_the_same_everywhere():
    """The kernel header, the module and the restatement name one step and one range."""
    import theory_restatement as rs
    src = open(os.path.join(ROOT, "opticommpy_amd", "csrc", "theory_kernels.h")).read()
    m = re.search(r"constexpr double kStep = ([0-9.]+), kTmax = ([0-9.]+);", src)
    assert (float(m.group(1)), float(m.group(2))) == (th.RULE_STEP, th.RULE_RANGE) == (rs.H_STEP, rs.T_MAX)
    assert int(re.search(r"constexpr int kK = (\d+)", src).group(1)) == round(rs.T_MAX / rs.H_STEP)
    assert th.RULE_BOUND == tc.RULE_BOUND and (th.MAX_POINTS, th.MAX_SNRS) == (1024, 4096)


def test_abi_rejects_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    d = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    tab, px, sg, out = np.array([1.0, 0.0, -1.0, 0.0]), np.array([0.5, 0.5]), np.array([0.3]), np.zeros(1)
    ok = dict(M=2, nS=1, tab=d(tab), px=d(px), sg=d(sg), out=d(out))
    keep = []

    def arr(a):
        keep.append(np.ascontiguousarray(a, dtype=np.float64))
        return keep[-1].ctypes.data_as(C.POINTER(C.c_double))
    for bad in (dict(M=0), dict(M=1025), dict(nS=0), dict(nS=4097), dict(tab=None), dict(px=None), dict(sg=None), dict(out=None),
                dict(px=arr([0.5, 0.0])), dict(px=arr([0.5, np.nan])), dict(px=arr([-0.5, 1.5])), dict(sg=arr([0.0])), dict(sg=arr([np.inf])),
                dict(sg=arr([-1.0])), dict(tab=arr([1.0, np.nan, 0.0, 0.0]))):
        a = dict(ok, **bad)
        assert lib.ssf_theory_mi(0, a["M"], a["nS"], a["tab"], a["px"], a["sg"], a["out"]) == -1, bad
    assert b"ssf_theory_mi" in lib.ssf_last_error(None)
    x = np.ones(8, dtype=np.complex128)
    xp = x.ctypes.data_as(C.c_void_p)
    okc = dict(n=8, dtype=0, M=2, s2=0.1, tab=d(tab), px=d(px), rx=xp, tx=xp, out=d(out))
    for bad in (dict(n=0), dict(dtype=4), dict(dtype=-1), dict(M=0), dict(M=1025), dict(s2=0.0), dict(s2=-1.0), dict(s2=np.nan), dict(tab=None),
                dict(px=None), dict(rx=None), dict(tx=None), dict(out=None), dict(px=arr([1.0, 0.0]))):
        a = dict(okc, **bad)
        assert lib.ssf_calc_mi(0, a["n"], a["dtype"], a["M"], a["s2"], a["tab"], a["px"], a["rx"], a["tx"], a["out"]) == -1, bad
    assert b"ssf_calc_mi" in lib.ssf_last_error(None)


@pytest.mark.skipif(oa.checkGPU(), reason="needs a box WITHOUT a GPU")
def test_no_cpu_fallback_when_no_gpu():
    x = np.ones(16, dtype=np.complex128)
    for call in (lambda: oa.theoryMI(4, "qam", 5.0), lambda: oa.constellationMI([1.0, -1.0], 5.0),
                 lambda: oa.calcMI(x, x, 0.1, [1.0, -1.0], [0.5, 0.5])):
        with pytest.raises(RuntimeError):
            call()


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libssf_hip.so")
    with pytest.raises(RuntimeError, match="HIP extension not built"):
        oa.theoryMI(4, "qam", 5.0)
    with pytest.raises(RuntimeError, match="HIP extension not built"):
        oa.calcMI(np.ones(4), np.ones(4), 0.1, [1.0, -1.0], [0.5, 0.5])
