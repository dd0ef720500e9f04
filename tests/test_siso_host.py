"""Host side of ffe / dfe / volterra / anorm without a GPU: exports, the reference's defaults, every refusal (all raised before
the library is touched), the layout of ssf_siso_params against its ctypes mirror, the division of a call's symbols between the
two kernels, and the C entry's own argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import opticommpy_amd as oa
import siso_cases as sc
from opticommpy_amd import _lib, equalization, metrics, sisoeq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.linspace(-1.0, 1.0, 40)
T = np.tile(sc.pam_table(4), 10)
XC, TC = X * (1 + 0.5j), np.tile(sc.qam_table(4), 10)


def test_exports():
    for name in ("ffe", "dfe", "volterra"):
        assert getattr(oa, name) is getattr(sisoeq, name) is getattr(equalization, name)
        assert name in oa.__all__ and name in equalization.__all__ and name in sisoeq.__all__
    assert oa.anorm is metrics.anorm and "anorm" in oa.__all__ and "anorm" in metrics.__all__
    assert "mimoAdaptEqualizer" in equalization.__all__ and isinstance(sisoeq.last_call, dict)
    from opticommpy_amd.equalization import dfe, ffe, volterra  # noqa: F401


def test_defaults_are_the_references():
    q = sisoeq._prepare("ffe", X, T, None)
    p = q["params"]
    assert (p.nTaps, p.SpS, p.nTrain, p.M, p.preconvIters, p.mode, p.mu, p.prec32, p.ncoef) == (5, 1, 1000, 4, 1, 0, 1e-4, 0, 5)
    assert np.array_equal(q["parts"][0], [0, 0, 1, 0, 0]) and q["N"] == 40
    assert sisoeq._prepare("ffe", X.astype(np.float32), T, None)["params"].prec32 == 1          # prec follows the input's dtype
    q = sisoeq._prepare("dfe", X, T, None)
    p = q["params"]
    assert (p.nTaps, p.nFB, p.SpS, p.nTrain, p.mu, p.ncoef, p.prec32) == (5, 5, 1, 1000, 1e-4, 10, 0)
    assert np.array_equal(q["parts"][0], [0, 0, 1, 0, 0]) and not np.any(q["parts"][1])
    q = sisoeq._prepare("volterra", X, T, None)
    p = q["params"]
    assert (p.nTaps, p.n2, p.n3, p.order, p.mu, p.prec32, p.ncoef) == (5, 3, 2, 2, 1e-3, 1, 5 + 9)   # prec defaults to float32
    assert [a.shape for a in q["parts"]] == [(5,), (3, 3), (2, 2, 2)] and q["parts"][0][2] == 1
    assert sisoeq._prepare("volterra", X, T, sc.Param(order=3))["params"].ncoef == 5 + 9 + 8
    # the table: grayMapping in prec, then power-normalised in prec
    t32, t64 = sisoeq._table(4, "pam", np.float32), sisoeq._table(4, "pam", np.float64)
    assert t32.dtype == np.float32 and t64.dtype == np.float64 and np.allclose(t64, np.array([-3, -1, 3, 1]) / np.sqrt(5))
    assert np.allclose(sisoeq._table(2, "ook", np.float64), [0.0, np.sqrt(2.0)], rtol=1e-15, atol=0)
    assert sisoeq._table(16, "qam", np.complex64).dtype == np.complex64


def test_the_callers_coefficients_are_copied():
    f = np.array([0.1, 0.8, 0.1, 0.0, 0.0])
    q = sisoeq._prepare("ffe", X, T, sc.Param(f=f))
    q["parts"][0][0] = 7.0
    assert f[0] == 0.1


REFUSALS = [
    ("ffe", XC, TC, dict(constType="pam"), ValueError),                    # a real table with complex data
    ("ffe", XC, TC, dict(constType="ook"), ValueError),
    ("ffe", X, T, dict(constType="qam"), ValueError),                      # a complex table with real data
    ("dfe", X, T, dict(constType="psk"), ValueError),
    ("ffe", X, T, dict(constType="apsk"), ValueError),
    ("volterra", XC, TC, dict(constType="qam", prec=np.complex64), TypeError),
    ("volterra", X, T, dict(prec=np.complex64), TypeError),
    ("ffe", X, T, dict(prec=np.float16), ValueError),
    ("ffe", X, T, dict(prec=np.int32), ValueError),
    ("ffe", XC, TC, dict(constType="qam", prec=np.float64), TypeError),    # a real prec with complex data
    ("dfe", X, T, dict(prec=np.complex128), TypeError),
    ("ffe", X, TC, dict(), TypeError),                                     # real data against complex symbols
    ("ffe", X, T, dict(SpS=0), ValueError),
    ("ffe", X, T, dict(SpS=6), ValueError),                                # SpS > nTaps: the reference indexes out of range
    ("ffe", X, T, dict(SpS=9, nTaps=11), ValueError),                      # above the kernels' 8
    ("dfe", X, T, dict(SpS=6), ValueError),
    ("volterra", X, T, dict(n1Taps=3, n2Taps=5), ValueError),
    ("volterra", X, T, dict(n1Taps=3, n3Taps=5), ValueError),
    ("volterra", X, T, dict(order=1), ValueError),
    ("volterra", X, T, dict(order=4), ValueError),
    ("ffe", X, T, dict(preconvIters=0), ValueError),
    ("ffe", X, T, dict(nTrain=-1), ValueError),
    ("ffe", X, T[:10], dict(nTrain=20), ValueError),                       # fewer symbols than min(nTrain, N)
    ("ffe", X, T[:30], dict(nTrain=1000), ValueError),
    ("ffe", np.zeros(0), T, dict(), ValueError),
    ("ffe", X[:1], T, dict(SpS=2, nTaps=3), ValueError),                   # not one whole symbol
    ("ffe", X, T, dict(trainingMode="blind"), ValueError),
    ("ffe", X, T, dict(f=np.zeros(4)), ValueError),                        # initial coefficients of the wrong shape
    ("dfe", X, T, dict(b=np.zeros(6)), ValueError),
    ("dfe", X, T, dict(f=np.zeros((5, 1))), ValueError),
    ("volterra", X, T, dict(h=[np.zeros(5), np.zeros((3, 3))]), ValueError),
    ("volterra", X, T, dict(h=[np.zeros(5), np.zeros((3, 2)), np.zeros((2, 2, 2))]), ValueError),
    ("volterra", X, T, dict(h=[np.zeros(5), np.zeros((3, 3)), np.zeros((2, 2))]), ValueError),
    ("ffe", X, T, dict(f=np.zeros(5, dtype=complex)), TypeError),
    ("ffe", X, T, dict(nTaps=257), ValueError),                            # the caps
    ("dfe", X, T, dict(nTapsFB=257), ValueError),
    ("volterra", X, T, dict(n1Taps=40, n2Taps=39), ValueError),            # 40 + 1521 + ... > 1536
    ("volterra", X, T, dict(n1Taps=12, n2Taps=2, n3Taps=12, order=3), ValueError),      # 12 + 4 + 1728
    ("ffe", X, T, dict(M=2048), ValueError),                               # above the table the kernels stage
    ("ffe", X, T, dict(M=6), ValueError),
    ("ffe", X.reshape(4, 10), T, dict(), ValueError),
    ("ffe", X, T, dict(mu=np.inf), ValueError),
]


@pytest.mark.parametrize("kind,x,t,prm,exc", REFUSALS, ids=[f"{i}-{r[0]}-{'-'.join(r[3]) or 'shape'}" for i, r in enumerate(REFUSALS)])
def test_refusals_come_before_the_library(monkeypatch, kind, x, t, prm, exc):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_library)
    with pytest.raises(exc):
        getattr(oa, kind)(x, t, sc.Param(**prm))


def test_the_caps_admit_the_notebooks_settings():
    x, t = np.tile(X, 10), np.tile(T, 10)
    assert sisoeq._prepare("ffe", x, t, sc.Param(nTaps=70, SpS=2))["params"].ncoef == 70
    assert sisoeq._prepare("dfe", x, t, sc.Param(nTapsFF=70, nTapsFB=15, SpS=2))["params"].ncoef == 85
    q = sisoeq._prepare("volterra", x, t, sc.Param(n1Taps=70, n2Taps=20, n3Taps=10, order=3, SpS=2))
    assert q["params"].ncoef == 1470 <= sisoeq.MAX_COEFFS and _lib.siso_slots(1470) == 24
    assert sisoeq._prepare("ffe", x, t, sc.Param(nTaps=9, SpS=8))["params"].SpS == 8
    assert [_lib.siso_slots(c) for c in (1, 63, 64, 65, 128, 129, 512, 513, 1024, 1025, 1536)] == [1, 1, 1, 2, 2, 4, 8, 16, 16, 24, 24]


def test_expected_split():
    def split(kind, n, **kw):
        return sisoeq.expected_split(sisoeq._prepare(kind, np.tile(X, 20)[:n], np.tile(T, 20), sc.Param(**kw)))
    assert split("ffe", 600, nTrain=100) == (100, 500)
    assert split("ffe", 600, nTrain=100, trainingMode="fulltime") == (600, 0)
    assert split("dfe", 600, nTrain=100) == (600, 0)                       # the feedback needs every decision
    assert split("volterra", 600, nTrain=0) == (0, 600)
    assert split("ffe", 600, nTrain=600) == (600, 0) and split("ffe", 600, nTrain=700, preconvIters=3) == (600, 0)
    assert split("ffe", 600, nTrain=100, preconvIters=3) == (2 * 101 + 100, 500)
    assert split("ffe", 600, nTrain=2, preconvIters=3, nTaps=9, SpS=2) == (2 * 3 + 5, 295)      # the carried window: ceil(9 / 2) symbols
    q = sisoeq._prepare("ffe", np.tile(X, 20)[:600], np.tile(T, 20), sc.Param(nTrain=100))
    assert sisoeq.expected_split(q, frozen=False) == (600, 0)


def expected_split(kind, x, ref, prm):
    return sisoeq.expected_split(sisoeq._prepare(kind, x, ref, prm))


def test_fixtures_cover_both_kernels():
    """Among the fixtures are calls that the serial kernel walks alone, and calls whose tail the frozen kernel takes."""
    seen = set()
    for name in sc.EXPECTED_CASES:
        g = sc.load(name)
        x, r = sc.inputs(g)
        s, p = expected_split(g["cfg"]["kind"], x, r, sc.param(g))
        seen.add((g["cfg"]["kind"], p > 0))
    assert seen == {("ffe", True), ("ffe", False), ("dfe", False), ("volterra", True), ("volterra", False)}


def test_rows_reach_every_path():
    """The rows' expected splits: a serial walk alone, a frozen kernel alone, both; one tile, one tile + 1, a tile - 1; several passes."""
    splits = {}
    for rid in sc.ROW_IDS:
        kind, x, tx, prm = sc.row(rid)
        splits[rid] = expected_split(kind, x, tx, prm)
    assert splits["ffe_train0"] == (0, 150) and splits["dfe_train0"] == (100, 0)
    assert splits["ffe_frozen_1"] == (99, 1) and splits["ffe_frozen_tile"] == (50, 256) and splits["ffe_frozen_tile_p1"] == (50, 257)
    assert splits["vol_frozen_tile_m1"] == (50, 255)
    assert splits["ffe_trainN"] == (150, 0) and splits["ffe_trainNp5"] == (150, 0)
    assert splits["ffe_pre4_below"] == (3 * 3 + 11, 139)           # after a restart the first nTaps / SpS windows stay serial
    assert splits["ffe_pre2_above"] == (71 + 70, 130)
    assert splits["ffe_pre4_fulltime"] == (3 * 71 + 150, 0)


def test_struct_layout_matches_the_header(tmp_path):
    """ssf_siso_params as gcc lays it out against the ctypes mirror."""
    cls, cname = _lib.SisoParams, "ssf_siso_params"
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    hdr = open(os.path.join(ROOT, "include", "ssf.h")).read()
    for name, code in list(_lib.SISO_KINDS.items()) + [(m.replace("-", "_"), v) for m, v in _lib.SISO_MODES.items()]:
        assert f"SSF_SISO_{name.upper()} = {code}" in hdr


def test_the_entry_point_checks_its_arguments_without_a_device():
    lib = _lib.load()
    q = sisoeq._prepare("volterra", X, T, sc.Param(order=3))
    coef = np.concatenate([a.reshape(-1) for a in q["parts"]])
    out, mse = np.empty(40), np.empty(40)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                            # noqa: E731
    tab = q["table"].ctypes.data_as(C.POINTER(C.c_double))

    def call(**change):
        p = _lib.SisoParams()
        C.pointer(p)[0] = q["params"]
        for k, v in change.items():
            setattr(p, k, v)
        return lib.ssf_siso_eq(0, C.byref(p), tab, vp(coef), vp(X), vp(T), vp(out), vp(mse))
    for change in (dict(kind=7), dict(n=0), dict(dtype=9), dict(mode=2), dict(nTaps=0), dict(nTaps=257), dict(SpS=0), dict(SpS=9), dict(SpS=6),
                   dict(M=1), dict(M=2000), dict(preconvIters=0), dict(nTrain=-1), dict(order=4), dict(n2=6), dict(n3=0), dict(ncoef=21),
                   dict(dtype=0), dict(ref_dtype=0), dict(nref=10, nTrain=20), dict(mu=float("nan"))):
        assert call(**change) == -1, change
        assert b"ssf_siso_eq" in lib.ssf_last_error(None)
    assert lib.ssf_siso_eq(0, None, tab, vp(coef), vp(X), vp(T), vp(out), vp(mse)) == -1
    p = q["params"]
    assert lib.ssf_siso_eq(0, C.byref(p), tab, None, vp(X), vp(T), vp(out), vp(mse)) == -1
    assert lib.ssf_siso_eq(0, C.byref(p), tab, vp(coef), None, vp(T), vp(out), vp(mse)) == -1
    assert lib.ssf_siso_eq(0, C.byref(p), tab, vp(coef), vp(X), None, vp(out), vp(mse)) == -1
    assert lib.ssf_siso_eq(0, C.byref(p), tab, vp(coef), vp(X), vp(T), vp(out), None) == -1
    d = _lib.SisoParams()
    C.pointer(d)[0] = q["params"]
    d.kind, d.nTaps, d.nFB, d.ncoef = _lib.SISO_KINDS["dfe"], 5, 300, 305
    assert lib.ssf_siso_eq(0, C.byref(d), tab, vp(coef), vp(X), vp(T), vp(out), vp(mse)) == -1
    d.kind, d.nTaps, d.n2, d.n3, d.order, d.ncoef = _lib.SISO_KINDS["volterra"], 40, 39, 1, 2, 40 + 39 * 39
    assert lib.ssf_siso_eq(0, C.byref(d), tab, vp(coef), vp(X), vp(T), vp(out), vp(mse)) == -1   # above 1536 coefficients
    a = _lib.SisoParams(n=0, kind=_lib.SISO_KINDS["anorm"], dtype=2)
    assert lib.ssf_siso_eq(0, C.byref(a), None, None, vp(X), None, vp(out), None) == -1


def test_restatement_is_self_consistent_in_double_and_extended_precision():
    """The restatement in double agrees with its extended-precision self far inside the test bound: the bound of 1e-9 measures the
    kernels, not the definition."""
    import siso_restatement as sr
    kind, x, tx, prm = sc.row("vol_t2_ne_t3")
    a, b = sr.restate(kind, x, tx, prm), sr.restate(kind, x, tx, prm, ext=np.float64)
    assert sc.rel_l2(b["sigOut"], a["sigOut"]) <= 1e-12 and sc.rel_l2(b["coef"][1], a["coef"][1]) <= 1e-12
