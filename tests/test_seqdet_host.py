"""Host side of mlse / detector / autocorr / levinson / estimateWhiteningFilter without a GPU: exports and module aliases, every
refusal with its message (all raised before the library is touched), inputs left unwritten, levinson against the fixtures, the
layout of ssf_mlse_params against its ctypes mirror, and the C entries' own argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import opticommpy_amd as oa
import seqdet_cases as sc
import seqdet_restatement as rs
from opticommpy_amd import _lib, core, modulation, seqdet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y = np.linspace(-1.0, 1.0, 40)
H = np.array([1.0, 0.5])
PAM4 = sc.pam_table(4)


class FakeDevice(oa.DeviceArray):
    """A DeviceArray that owns no memory: the refusals come before any pointer is read."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.device, self._ptr, self._owner = tuple(shape), np.dtype(dtype), 0, C.c_void_p(), self


def test_exports_and_aliases():
    for name in ("mlse", "detector", "autocorr", "levinson", "estimateWhiteningFilter"):
        assert getattr(oa, name) is getattr(seqdet, name) and name in oa.__all__ and name in seqdet.__all__
    assert modulation.mlse is seqdet.mlse and modulation.detector is seqdet.detector
    assert modulation.grayMapping is oa.grayMapping and modulation.modulateGray is oa.modulateGray and modulation.demodulateGray is oa.demodulateGray
    assert set(modulation.__all__) == {"mlse", "detector", "grayMapping", "modulateGray", "demodulateGray"}
    for name in ("estimateWhiteningFilter", "autocorr", "levinson"):
        assert getattr(core, name) is getattr(seqdet, name)
    assert isinstance(seqdet.last_call, dict)
    from opticommpy_amd.core import estimateWhiteningFilter  # noqa: F401
    from opticommpy_amd.modulation import detector, mlse  # noqa: F401


MLSE_REFUSALS = [
    (Y, H, np.zeros(0), ValueError, "0 points"),
    (Y, H, sc.pam_table(65), ValueError, "65 points"),
    (Y, np.ones(6) * .1, sc.pam_table(5), ValueError, "5 ** 5 = 3125 states"),
    (Y, np.ones(12) * .1, sc.pam_table(2), ValueError, "12 taps"),
    (Y, np.zeros(0), PAM4, ValueError, "h is empty"),
    (np.zeros((40, 65)), H, PAM4, ValueError, "65 columns"),
    (np.zeros(0), H, PAM4, ValueError, "y is empty"),
    (np.zeros((0, 2)), H, PAM4, ValueError, "y is empty"),
    (np.zeros((2, 2, 2)), H, PAM4, ValueError, "1-D or (n, nModes)"),
    (Y, H.reshape(1, 2), PAM4, ValueError, "h must be one-dimensional"),
    (Y, H, PAM4.reshape(2, 2), ValueError, "constSymb must be one-dimensional"),
    (Y, H * (1 + 0.1j), PAM4, ValueError, "y is real but h has imaginary parts"),
    (Y, H, sc.qam_table(4), ValueError, "y is real but constSymb has imaginary parts"),
    (Y.astype(np.int64), H, PAM4, TypeError, "float dtype expected"),
    (FakeDevice((40,), np.float32), H, PAM4, TypeError, "needs float64 or complex128"),
    (FakeDevice((40,), np.complex64), H, PAM4, TypeError, "needs float64 or complex128"),
    (FakeDevice((1 << 22, 1), np.float64), np.ones(11) * .1, sc.pam_table(2), ValueError, f"survivor memory of {1 << 32} bytes is above 2 ** 31 bytes"),
]


@pytest.mark.parametrize("i", range(len(MLSE_REFUSALS)))
def test_mlse_refuses_before_anything_runs(i, monkeypatch):
    y, h, c, exc, text = MLSE_REFUSALS[i]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(exc) as e:
        oa.mlse(y, h, c)
    assert text in str(e.value)


def test_mlse_host_quantities():
    q = seqdet._prepare_mlse(Y.astype(np.float32), H.astype(np.complex128), PAM4.astype(np.complex64))   # zero imaginary parts are narrowed
    assert (q["M"], q["taps"], q["states"], q["cols"], q["N"], q["cx"], q["out_dtype"]) == (4, 2, 4, 1, 40, False, np.float32)
    assert q["h"].dtype == np.float64 and q["h"].shape == (4,) and q["c"].shape == (8,)
    q = seqdet._prepare_mlse(np.zeros((7, 3), dtype=np.complex64), [1.0], [1, -1])
    assert (q["states"], q["cols"], q["cx"], q["out_dtype"]) == (1, 3, True, np.complex64)
    assert seqdet._prepare_mlse(Y, np.ones(6) * .1, PAM4)["states"] == 1024                              # the cap itself
    assert seqdet.survivor_bytes(5, 1, 1) == 32 and seqdet.survivor_bytes(5, 2, 9) == 2 * 64 and seqdet.survivor_bytes(1 << 21, 1, 1024) == 1 << 31
    assert seqdet._prepare_mlse(FakeDevice((1 << 21,), np.float64), np.ones(11) * .1, sc.pam_table(2))["survivor_bytes"] == 1 << 31   # the cap itself


DET_REFUSALS = [
    (Y, 1.0, PAM4, None, "map", ValueError, "rule must be 'MAP' or 'ML'"),
    (Y, 1.0, PAM4, [.5, .5], "MAP", ValueError, "px has 2 entries for 4"),
    (Y, 0.0, PAM4, None, "MAP", ValueError, "must be positive"),
    (Y, -1.0, PAM4, None, "MAP", ValueError, "must be positive"),
    (Y, float("nan"), PAM4, None, "MAP", ValueError, "must be positive"),
    (Y, 1.0, sc.pam_table(65), None, "ML", ValueError, "65 points"),
    (Y, 1.0, np.zeros(0), None, "ML", ValueError, "0 points"),
    (np.zeros(0), 1.0, PAM4, None, "ML", ValueError, "r is empty"),
    (np.zeros((2, 2, 2)), 1.0, PAM4, None, "ML", ValueError, "1-D or (n, nModes)"),
    (Y.astype(np.int32), 1.0, PAM4, None, "ML", TypeError, "float dtype expected"),
    (FakeDevice((40,), np.float32), 1.0, PAM4, None, "ML", TypeError, "needs float64 or complex128"),
    (FakeDevice((40,), np.float64), 1.0, sc.qam_table(4), None, "ML", TypeError, "hand r over as complex128"),
]


@pytest.mark.parametrize("i", range(len(DET_REFUSALS)))
def test_detector_refuses_before_anything_runs(i, monkeypatch):
    r, s2, c, px, rule, exc, text = DET_REFUSALS[i]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(exc) as e:
        oa.detector(r, s2, c, px=px, rule=rule)
    assert text in str(e.value)


def test_detector_host_quantities():
    q = seqdet._prepare_detector(Y, 0.0, PAM4, [.1, .2, .3, .4], "ML")                 # 'ML': σ2 and px are not looked at
    assert not np.any(q["logpx"]) and q["rule"] == 0 and not q["cx"]
    q = seqdet._prepare_detector(Y, 0.5, PAM4, [.5, .5, 0, 0], "MAP")
    assert np.array_equal(q["logpx"], [np.log(.5), np.log(.5), -np.inf, -np.inf]) and q["sigma2"] == 0.5 and q["rule"] == 1
    assert np.array_equal(seqdet._prepare_detector(Y, 0.5, PAM4, None, "MAP")["logpx"], np.log(1 / 4 * np.ones(4)))
    q = seqdet._prepare_detector(Y, 0.5, sc.qam_table(4), None, "MAP")                 # a real numpy r against a complex table
    assert q["widen"] and q["cx"] and q["out_dtype"] == np.float64


AC_REFUSALS = [
    (Y * 1j, 2, ValueError, "real data"), (FakeDevice((40,), np.complex128), 2, ValueError, "real data"), (Y, 0, ValueError, "between 1 and 256"),
    (np.zeros(300), 257, ValueError, "between 1 and 256"), (Y, 41, ValueError, "exceeds the 40 samples"), (Y, 2.5, ValueError, "integer"),
    (Y.reshape(2, 20), 2, ValueError, "one-dimensional"), (FakeDevice((40,), np.float32), 2, TypeError, "needs float64"),
]


@pytest.mark.parametrize("i", range(len(AC_REFUSALS)))
@pytest.mark.parametrize("fn", ["autocorr", "estimateWhiteningFilter"])
def test_autocorr_refuses_before_anything_runs(i, fn, monkeypatch):
    x, nTaps, exc, text = AC_REFUSALS[i]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(exc) as e:
        getattr(oa, fn)(x, nTaps)
    assert text in str(e.value)


def test_inputs_are_left_unwritten():
    y, h, c = Y.copy(), H.copy(), PAM4.copy()
    seqdet._prepare_mlse(y, h, c)
    px = np.array([.1, .2, .3, .4])
    seqdet._prepare_detector(y, 1.0, c, px, "MAP")
    r = np.array([1.0, 0.5, 0.2])
    oa.levinson(r, 3)
    assert np.array_equal(y, Y) and np.array_equal(h, H) and np.array_equal(c, PAM4) and np.array_equal(px, [.1, .2, .3, .4])
    assert np.array_equal(r, [1.0, 0.5, 0.2])


@pytest.mark.parametrize("name", sc.WHITE_CASES)
def test_levinson_matches_the_reference(name):
    """The host half of estimateWhiteningFilter: the fixture's r gives the fixture's w, bit for bit (the same operations in the
    same order), and agrees with the extended-precision restatement."""
    g = sc.load(name)
    sc.check_conditions(g)
    nTaps = g["cfg"]["nTaps"]
    w = oa.levinson(g["r"], nTaps)
    assert w.dtype == np.float64 and np.array_equal(w, g["w"])
    want, ks = rs.levinson(g["r"], nTaps)
    assert np.max(np.abs(w - want)) <= 1e-12 * np.max(np.abs(want)) and (len(ks) == 0 or np.max(np.abs(ks)) < 0.95)
    assert oa.levinson(g["r"], 1).tolist() == [1.0]
    with pytest.raises(ValueError):
        oa.levinson(g["r"], nTaps + 1)


def test_restatement_autocorr_matches_the_reference():
    for name in sc.WHITE_CASES:
        g = sc.load(name)
        assert np.max(np.abs(rs.autocorr(g["x"], g["cfg"]["nTaps"]) - g["r"])) <= 1e-12 * g["r"][0]


def test_struct_layout_matches_the_header(tmp_path):
    """ssf_mlse_params as gcc lays it out against the ctypes mirror; the constants of _lib against seqdet_kernels.h."""
    cls, cname = _lib.MlseParams, "ssf_mlse_params"
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
    assert "SSF_DET_ML = 0, SSF_DET_MAP = 1" in hdr and _lib.SEQDET_RULES == {"ML": 0, "MAP": 1}
    k = open(os.path.join(ROOT, "opticommpy_amd", "csrc", "seqdet_kernels.h")).read()
    for text in (f"kMaxM = {_lib.SEQDET_MAX_M}, kMaxStates = {_lib.SEQDET_MAX_STATES}, kMaxTaps = {_lib.SEQDET_MAX_TAPS}, kMaxCols = {_lib.SEQDET_MAX_COLS}",
                 f"kSurvChunk = {_lib.SEQDET_SURV_CHUNK};", f"kStageChunk = {_lib.SEQDET_STAGE_CHUNK};", f"kDetBlock = {_lib.SEQDET_DET_BLOCK};",
                 f"kAcMaxTaps = {_lib.SEQDET_AC_MAX_TAPS}, kAcTile = {_lib.SEQDET_AC_TILE}"):
        assert text in k, text


def test_the_entry_points_check_their_arguments_without_a_device():
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                            # noqa: E731
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                 # noqa: E731
    h, c = np.array([1.0, 0, 0.5, 0]), np.ascontiguousarray(PAM4.astype(np.complex128)).view(np.float64)
    out, fin = np.empty(40), np.empty(1)

    def mlse(**change):
        p = _lib.MlseParams(n=40, cols=1, dtype=2, M=4, taps=2)
        for k, v in change.items():
            setattr(p, k, v)
        return lib.ssf_mlse(0, C.byref(p), dp(h), dp(c), vp(Y), vp(out), dp(fin))
    for change in (dict(M=0), dict(M=65), dict(taps=0), dict(taps=12), dict(M=5, taps=6), dict(M=2, taps=11, n=1 << 22), dict(cols=0), dict(cols=65),
                   dict(n=0), dict(n=1 << 40)):
        assert mlse(**change) == -1, change
        assert b"ssf_mlse" in lib.ssf_last_error(None)
    assert mlse(M=2, taps=11, n=1 << 22) == -1 and str(1 << 32).encode() in lib.ssf_last_error(None)      # the message names the figure
    assert mlse(dtype=1) == -6 and mlse(dtype=3) == -6 and mlse(dtype=9) == -6
    p = _lib.MlseParams(n=40, cols=1, dtype=2, M=4, taps=2)
    args = [C.byref(p), dp(h), dp(c), vp(Y), vp(out), dp(fin)]
    for i in range(len(args)):
        assert lib.ssf_mlse(0, *[None if j == i else a for j, a in enumerate(args)]) == -1, i

    dec, ind, lp = np.empty(40), np.empty(40, dtype=np.int64), np.zeros(4)

    def det(n=40, dtype=2, M=4, rule=1, s2=1.0, tab=dp(c), logpx=dp(lp), r=vp(Y), d=vp(dec), i=vp(ind)):
        return lib.ssf_detector(0, n, dtype, M, rule, s2, tab, logpx, r, d, i)
    for kw in (dict(n=0), dict(M=0), dict(M=65), dict(rule=2), dict(s2=0.0), dict(s2=float("nan")), dict(tab=None), dict(logpx=None), dict(r=None),
               dict(d=None), dict(i=None)):
        assert det(**kw) == -1, kw
        assert b"ssf_detector" in lib.ssf_last_error(None)
    assert det(dtype=1) == -6 and det(dtype=7) == -6 and det(rule=0, logpx=None, s2=0.0) != -1

    r = np.empty(4)
    assert lib.ssf_autocorr(0, 40, 0, vp(Y), dp(r)) == -1 and lib.ssf_autocorr(0, 40, 257, vp(Y), dp(r)) == -1
    assert lib.ssf_autocorr(0, 3, 4, vp(Y), dp(r)) == -1 and b"ssf_autocorr" in lib.ssf_last_error(None)
    assert lib.ssf_autocorr(0, 40, 4, None, dp(r)) == -1 and lib.ssf_autocorr(0, 40, 4, vp(Y), None) == -1
