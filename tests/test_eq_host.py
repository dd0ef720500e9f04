"""Host side of the adaptive equalizer (opticommpy_amd/equalization.py) without a GPU: what is out of scope is refused before the
library is even loaded, the quantities handed to the library equal the reference's, and the shape rules hold."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eq_cases as ec
import opticommpy_amd as oa
from opticommpy_amd import _lib
from opticommpy_amd import equalization as oeq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the checks under test come before it."""
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


X = (np.arange(128).reshape(64, 2) * 0.01 + 1j).astype(np.complex128)       # 64 samples, 2 modes: 32 symbols at 2 SpS
REF = np.ones((32, 2), dtype=np.complex128)


def test_every_case_of_the_issue_has_a_fixture():
    assert ec.CASES == ec.EXPECTED_CASES
    for name in ec.CASES:
        g = ec.load(name)
        ec.check_conditions(g)
        assert g["cfg"]["total"] <= 1500 and os.path.getsize(os.path.join(ec.GOLDEN, f"eq_{name}.npz")) <= 282045


def test_public_name():
    assert oa.mimoAdaptEqualizer is oeq.mimoAdaptEqualizer and "mimoAdaptEqualizer" in oa.__all__


@pytest.mark.parametrize("kw", [
    dict(alg=["rls"]), dict(alg=["dd-rls"]), dict(alg=["nlms", "rls"], mu=[1e-3, 1e-3], L=[10, 10]), dict(alg=["lms"]), dict(alg=[]),
    dict(alg="rls"),
    dict(runWL=True), dict(storeCoeff=True),
    dict(nTaps=0), dict(nTaps=65), dict(nTaps=7.5), dict(SpS=0), dict(SpS=9),
    dict(constType="pam"), dict(M=8), dict(M=3), dict(M=2048),
    dict(alg=["nlms", "dd-lms"]), dict(alg=["nlms"], mu=[1e-3, 1e-3]), dict(alg=["nlms"], L=[10, 10]),      # one entry per stage
    dict(L=[0]), dict(L=[-1]), dict(L=[33]), dict(alg=["nlms", "cma"], mu=[1e-3, 1e-3], L=[20, 13]),
    dict(numIter=0), dict(numIter=1.5),
    dict(nTaps=65), dict(prec=np.float32),
    dict(H=np.zeros((4, 14), complex)), dict(H=np.zeros((2, 15), complex)),
])
def test_out_of_scope_parameters_raise_before_the_library_loads(no_library, kw):
    with pytest.raises(ValueError):
        oa.mimoAdaptEqualizer(X, ec.Param(**kw), REF)


def test_signals_out_of_scope_raise_before_the_library_loads(no_library):
    for bad in (np.zeros((64, 5), complex), np.zeros((3, 4), complex), np.zeros((2, 2, 2), complex), np.complex128(1),
                np.zeros((14, 2), complex), np.zeros(14, complex), np.zeros((0, 2), complex)):
        with pytest.raises(ValueError):
            oa.mimoAdaptEqualizer(bad, ec.Param(alg=["cma"]))
    for alg in ("nlms", "da-rde"):                           # a data-aided stage needs symbRef, long and wide enough
        for ref in (None, [], REF[:31], REF[:, :1], np.ones((32, 3), complex)):
            with pytest.raises(ValueError):
                oa.mimoAdaptEqualizer(X, ec.Param(alg=[alg]), ref)
        with pytest.raises(ValueError):
            oa.mimoAdaptEqualizer(X, ec.Param(alg=["cma", alg], mu=[1e-3, 1e-3], L=[10, 22]), REF[:31])
    oeq._prepare(X, ec.Param(alg=["cma", "nlms"], mu=[1e-3, 1e-3], L=[10, 21]), REF[:31])
    oeq._prepare(X, ec.Param(alg=["cma", "rde", "dd-lms", "static"], mu=[1e-3] * 4, L=[8] * 4))      # no symbRef needed


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32])
def test_device_arrays_of_another_dtype_raise_type_error(no_library, dtype):
    d = object.__new__(oa.DeviceArray)                      # (no GPU needed: the check is on the type)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (64, 2), np.dtype(dtype), 0, None, d
    with pytest.raises(TypeError, match="complex128 or complex64"):
        oa.mimoAdaptEqualizer(d, ec.Param(alg=["cma"]))


def test_defaults_are_the_references():
    with pytest.raises(ValueError):                          # the default 'nlms' needs symbRef
        oeq._prepare(X, None, None)
    q = oeq._prepare(X, None, REF)
    p = q["params"]
    assert (p.nTaps, p.SpS, p.numIter, p.M, p.nStages, p.nModes, p.n, p.total) == (15, 2, 1, 4, 1, 2, 64, 32)
    assert q["alg"] == ["nlms"] and q["L"] == [32] and q["mu"] == [float(np.float32(1e-3))] and not q["returnResults"]
    assert q["stages"][0].alg == _lib.EQ_ALGS["nlms"] and q["stages"][0].L == 32
    assert np.array_equal(q["H"], ec.spike(2, 15)) and q["H"].dtype == np.complex128
    # a string, a scalar step size and a scalar length are one stage
    q = oeq._prepare(X, ec.Param(alg="cma", mu=2e-3, L=20))
    assert q["alg"] == ["cma"] and q["L"] == [20] and q["mu"] == [float(np.float32(2e-3))]


def test_step_size_is_rounded_to_single_precision():
    for mu in (1e-3, 5e-3, 2e-3, 0.1, 1 / 3):
        q = oeq._prepare(X, ec.Param(alg=["cma", "rde"], mu=[mu, mu / 7], L=[10, 10]))
        assert q["stages"][0].mu == float(np.float32(mu)) and q["stages"][1].mu == float(np.float32(mu / 7))
        assert q["stages"][0].mu != mu


@pytest.mark.parametrize("name", ec.EXPECTED_CASES)
def test_tables_are_the_references(name):
    g = ec.load(name)
    prm = g["cfg"]["param"]
    wanted = [(np.dtype(g["cfg"]["prec"] or "complex64"), g["table"], g["Rcma"], g["Rrde"])]
    if name == "default_prec":
        wanted.append((np.dtype("complex128"), g["table128"], g["Rcma128"], g["Rrde128"]))
    for prec, table, Rcma, Rrde in wanted:
        c, R, radii = oeq._tables(prm["M"], prm.get("constType", "qam"), 0, prec)
        assert c.dtype == prec == table.dtype and c.tobytes() == table.tobytes()
        assert R == float(np.asarray(Rcma).real) and np.asarray(Rcma).imag == 0
        assert radii.dtype == np.float64 and np.array_equal(radii, np.asarray(Rrde).real.astype(np.float64)) and np.all(np.asarray(Rrde).imag == 0)
        q = oeq._prepare(g["sigIn"], ec.param(g, prec=prec.type), g["symbRef"])
        assert np.array_equal(q["table"].view(np.complex128), table.astype(np.complex128)) and q["params"].Rcma == R
        assert np.array_equal(q["radii"], radii) and q["params"].nRadii == len(radii) and q["params"].M == prm["M"]


@pytest.mark.parametrize("n,nTaps,SpS,want", [
    (3000, 4, 3, 1001), (3000, 15, 2, 1500), (3000, 15, 1, 3000), (3000, 16, 1, 3001), (3000, 16, 2, 1501), (3001, 16, 2, 1501),
    (3000, 15, 3, 1000), (3001, 15, 3, 1001), (3002, 15, 3, 1001), (3000, 1, 1, 3000), (3000, 2, 3, 1001), (64, 64, 2, 33),
])
def test_total_number_of_symbols(n, nTaps, SpS, want):
    assert oeq.total_symbols(n, nTaps, SpS) == want
    padded = n + 2 * (nTaps // 2)
    assert (want - 1) * SpS + nTaps <= padded < want * SpS + nTaps          # the last window fits, one more would not
    assert oeq._prepare(np.ones((n, 1), complex), ec.Param(alg=["cma"], nTaps=nTaps, SpS=SpS))["total"] == want


def test_shape_rules_and_initial_coefficients():
    q = oeq._prepare(np.ones(64, np.complex64), ec.Param(alg=["cma"]))
    assert q["input1D"] and q["x"].shape == (64, 1) and q["x"].dtype == np.complex64 and q["params"].dtype == 1
    q = oeq._prepare(np.ones((64, 1)), ec.Param(alg=["cma"]))
    assert not q["input1D"] and q["x"].dtype == np.complex128 and q["params"].dtype == 0
    q = oeq._prepare(X, ec.Param(alg=["nlms"]), REF[:, 0].astype(np.complex64).repeat(2).reshape(32, 2))
    assert q["params"].ref_dtype == 1 and q["params"].nref == 32
    H = np.arange(60).reshape(4, 15) * (1 + 2j)
    keep = H.copy()
    q = oeq._prepare(X, ec.Param(alg=["cma"], H=H))
    assert np.array_equal(q["H"], H) and q["H"] is not H and np.array_equal(H, keep)
    for modes, taps in ((1, 1), (3, 4), (4, 64)):
        q = oeq._prepare(np.ones((70, modes), complex), ec.Param(alg=["cma"], nTaps=taps))
        assert np.array_equal(q["H"], ec.spike(modes, taps))


def test_struct_layout_matches_the_header(tmp_path):
    """ssf_eq_params and ssf_eq_stage as gcc lays them out against the ctypes mirrors."""
    structs = {"ssf_eq_params": _lib.EqParams, "ssf_eq_stage": _lib.EqStage}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    (tmp_path / "layout.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    header = open(os.path.join(ROOT, "include", "ssf.h")).read()
    for name, value in _lib.EQ_ALGS.items():
        assert re.search(rf"SSF_EQ_{name.replace('-', '').upper()} = {value}\b", header), name


def test_chunk_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "opticommpy_amd", "csrc", "eq_kernels.h")).read()
    assert int(re.search(r"constexpr int kChunk = (\d+);", src).group(1)) == _lib.EQ_CHUNK
    wave, pre = (int(re.search(rf"constexpr int {k} = (\d+);", src).group(1)) for k in ("kWave", "kPre"))
    assert wave * pre == _lib.EQ_STAGE_ELEMS
    for modes in (1, 2, 3, 4):                               # every geometry the shape tests use stages whole chunks
        for taps in (1, 2, 15, 16, 17, 64):
            for sps in (1, 2, 3):
                c = _lib.eq_chunk(modes, taps, sps)
                assert c == _lib.EQ_CHUNK and ((c - 1) * sps + taps) * modes <= _lib.EQ_STAGE_ELEMS
    for modes, taps, sps in ((4, 64, 8), (4, 64, 4), (3, 64, 8), (1, 64, 8), (4, 1, 8)):
        c = _lib.eq_chunk(modes, taps, sps)
        assert 1 <= c <= _lib.EQ_CHUNK and ((c - 1) * sps + taps) * modes <= _lib.EQ_STAGE_ELEMS
        assert c == _lib.EQ_CHUNK or (c * sps + taps) * modes > _lib.EQ_STAGE_ELEMS


def test_library_refuses_bad_arguments_without_a_device():
    """The C ABI's own checks come before any allocation or launch: they answer on a box without a GPU."""
    lib = _lib.load()
    q = oeq._prepare(X, ec.Param(alg=["nlms", "dd-lms"], mu=[1e-3, 1e-3], L=[16, 16], M=16), REF)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))         # noqa: E731
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                    # noqa: E731
    out, H = np.empty((32, 2), complex), q["H"]
    x, ref = np.ascontiguousarray(q["x"]), np.ascontiguousarray(q["ref"])

    def call(params=None, stages=q["stages"], refp=vp(ref), **bad):
        p = _lib.EqParams.from_buffer_copy(q["params"])
        for k, v in bad.items():
            setattr(p, k, v)
        return lib.ssf_mimo_eq(0, C.byref(p) if params is None else params, stages, dp(q["table"]), dp(q["radii"]), vp(H), vp(x), refp,
                               vp(out), None)

    for bad in (dict(nModes=0), dict(nModes=5), dict(nTaps=0), dict(nTaps=65), dict(SpS=0), dict(SpS=9), dict(n=14), dict(dtype=2),
                dict(total=31), dict(total=33), dict(M=1), dict(M=1025), dict(nRadii=0), dict(nRadii=1025), dict(numIter=0),
                dict(nStages=0), dict(nref=31), dict(ref_dtype=3), dict(Rcma=float("nan"))):
        assert call(**bad) == -1, bad
    assert b"ssf_mimo_eq" in lib.ssf_last_error(None)
    assert call(refp=None) == -1                                   # a data-aided stage without ref
    for L, alg in ((0, 0), (17, 0), (16, 6), (16, -1)):
        st = (_lib.EqStage * 2)(_lib.EqStage(L=L, alg=alg, mu=1e-3), _lib.EqStage(L=16, alg=4, mu=1e-3))
        assert call(stages=st) == -1, (L, alg)
    assert lib.ssf_mimo_eq(0, None, q["stages"], dp(q["table"]), dp(q["radii"]), vp(H), vp(x), vp(ref), vp(out), None) == -1
    assert lib.ssf_mimo_eq(0, C.byref(q["params"]), q["stages"], dp(q["table"]), dp(q["radii"]), None, vp(x), vp(ref), vp(out), None) == -1
    assert np.array_equal(H, ec.spike(2, 15))
