"""The host side of the OFDM functions without a GPU and without the library: every ValueError is raised before the library is
touched, the carrier plan's tables say what the reference's index arithmetic says, the plan cache evicts and releases, and the ABI
names its new symbols."""
import os
import re

import numpy as np
import pytest

import ofdm_cases as oc
import ofdm_restatement as rs
import opticommpy_amd as oa
from opticommpy_amd import _lib, ofdm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test."""
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", boom)


def P(**kw):
    return oc.Param(**kw)


X = np.ones(512, dtype=np.complex128)
BAD_BOTH = [
    (dict(Nfft=16, pilotCarriers=[3]), "Np = 1"),
    (dict(Nfft=16, pilotCarriers=[3, 3, 5]), "twice"),
    (dict(Nfft=16, pilotCarriers=[3, 16]), "leaves the carriers"),
    (dict(Nfft=16, nullCarriers=[-1]), "leaves the carriers"),
    (dict(Nfft=16, hermitSymmetry=True, pilotCarriers=[0, 7]), "leaves the carriers"),          # Ns = 7
    (dict(Nfft=16, pilotCarriers=[3, 5], nullCarriers=[5]), "pilot and as null"),
    (dict(Nfft=16, pilotCarriers=[0, 1], nullCarriers=list(range(2, 16))), "Ni = "),
    (dict(Nfft=4, hermitSymmetry=True, nullCarriers=[0]), "Ni = "),
    (dict(Nfft=15, hermitSymmetry=True), "odd"),
    (dict(Nfft=16, G=-1), "G = -1"),
    (dict(Nfft=16, G=17), "G = 17"),
    (dict(Nfft=3), "Nfft = 3"),
    (dict(Nfft=16, pilotCarriers=[1.5, 3]), "integers"),
]


@pytest.mark.parametrize("kw,match", BAD_BOTH, ids=[m for _, m in BAD_BOTH])
def test_bad_parameters_raise_before_the_library(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        oa.modulateOFDM(X, P(**kw))
    with pytest.raises(ValueError, match=match):
        oa.demodulateOFDM(X, P(**kw))


def test_modulator_only_errors(no_library):
    with pytest.raises(ValueError, match=r"Number of symbols \(100\) is not divisible"):
        oa.modulateOFDM(np.ones(100, dtype=complex), P(Nfft=16))
    with pytest.raises(ValueError, match="SpS = 0"):
        oa.modulateOFDM(X, P(Nfft=16, SpS=0))
    with pytest.raises(ValueError, match=r"Nfft \(SpS - 1\) = 15 is odd"):
        oa.modulateOFDM(X, P(Nfft=15, SpS=2))
    with pytest.raises(ValueError, match="dtype = float64"):
        oa.modulateOFDM(X, P(Nfft=16), dtype=np.float64)


def test_demodulator_only_errors(no_library):
    with pytest.raises(ValueError, match=r"Number of received symbols \(512\) is not divisible by Nfft \+ G \(20\)"):
        oa.demodulateOFDM(X, P(Nfft=16, G=4))


@pytest.mark.parametrize("f", [oa.modulateOFDM, oa.demodulateOFDM])
def test_bad_arrays_raise_before_the_library(no_library, f):
    with pytest.raises(ValueError, match=r"shape \(4, 128\)"):
        f(X.reshape(4, 128), P(Nfft=16, G=0))
    with pytest.raises(ValueError, match="dtype float64"):
        f(np.ones(512), P(Nfft=16, G=0))
    with pytest.raises(ValueError, match="dtype int64"):
        f(np.ones(512, dtype=np.int64), P(Nfft=16, G=0))


def test_a_device_array_of_another_type_gets_the_type_error_of_device_arg(no_library):
    d = object.__new__(oa.DeviceArray)                      # (no GPU needed: the check is on the type)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (512,), np.dtype(np.float64), 0, None, d
    for f in (oa.modulateOFDM, oa.demodulateOFDM):
        with pytest.raises(TypeError, match="complex128"):
            f(d, P(Nfft=16, G=0))


def test_defaults_are_the_reference_code_s():
    q = ofdm._prepare_mod(np.ones(1024, dtype=complex), None)
    assert q["plan"]["Nfft"] == 512 and q["G"] == 4 and q["plan"]["SpS"] == 2 and q["pilot"] == 0.25 + 0.25j
    assert q["plan"]["Np"] == 0 and q["plan"]["Ni"] == 512 and q["nframes"] == 2 and q["dtype"] == np.complex64
    assert ofdm._prepare_demod(np.ones(516, dtype=np.complex64), None)["x"].dtype == np.complex64


def test_the_plan_s_tables_are_the_reference_s_index_arithmetic():
    rng = np.random.default_rng(5)
    for trial in range(40):
        hermit = bool(trial % 3 == 0)
        Nfft = int(rng.choice([4, 6, 12, 16, 30, 64, 255])) if not hermit else int(rng.choice([8, 12, 16, 30, 64]))
        SpS = int(rng.choice([1, 2, 3, 4])) if Nfft % 2 == 0 else int(rng.choice([1, 3]))
        Ns = Nfft // 2 - 1 if hermit else Nfft
        k = int(rng.integers(0, Ns))                                    # carriers taken away, at least one left
        taken = rng.permutation(Ns)[:k]
        npil = int(rng.integers(0, k + 1))
        npil = 0 if npil == 1 else npil
        pilots, nulls = taken[:npil], taken[npil:]
        ofdm.release_plans()
        plan = ofdm._carrier_plan(Nfft, SpS, hermit, pilots.astype(np.int64), nulls.astype(np.int64))
        data = np.setdiff1d(np.arange(Ns), np.union1d(pilots, nulls))
        assert np.array_equal(plan["data"], data) and plan["Ni"] == len(data) and plan["Ns"] == Ns
        assert np.array_equal(plan["pilots"], np.sort(pilots))
        # the modulator's map, applied to a frame of distinct values, is the reference's padded and shifted frame
        symb = rng.normal(size=len(data)) + 1j * rng.normal(size=len(data))
        pilot = 0.3 - 0.2j
        V = np.zeros(Ns, dtype=complex)
        V[data], V[pilots] = symb, pilot
        if hermit:
            V = oa.hermit(V)
        pad = (Nfft * (SpS - 1)) // 2
        want = np.fft.fftshift(oa.zeroPad(V, pad))
        code = plan["src_map"]
        src = np.where(code & 3 == _lib.OFDM_SRC_DATA, symb[np.minimum(code >> 3, len(data) - 1)],
                       np.where(code & 3 == _lib.OFDM_SRC_PILOT, pilot, 0))
        src = np.where(code & _lib.OFDM_SRC_CONJ, np.conj(src), src)
        assert np.array_equal(src, want), (Nfft, SpS, hermit)
        # the demodulator's: bin k of fft(frame) -> carrier
        S = np.fft.fftshift(np.arange(Nfft))
        S = S[1:1 + Ns] if hermit else S
        back = np.full(Nfft, -1)
        back[S] = np.arange(Ns)
        assert np.array_equal(plan["bin_carrier"], back)
        if npil:
            xs = np.sort(pilots)
            hi = plan["hi"]
            assert hi.min() >= 1 and hi.max() <= npil - 1
            y = rng.normal(size=npil)
            got = (y[hi] - y[hi - 1]) / (xs[hi] - xs[hi - 1]) * (np.arange(Ns) - xs[hi - 1]) + y[hi - 1]
            assert np.allclose(got, rs.line_through(pilots, y[np.argsort(np.argsort(pilots))], np.arange(Ns, dtype=float)), atol=1e-12)


def test_plan_cache_evicts_and_releases():
    ofdm.release_plans()
    assert ofdm.plan_cache_info() == []
    e = np.array([], dtype=np.int64)
    first = ofdm._carrier_plan(16, 2, False, e, e)
    assert ofdm._carrier_plan(16, 2, False, e, e) is first and len(ofdm.plan_cache_info()) == 1
    assert ofdm._carrier_plan(16, None, False, e, e) is not first        # the demodulator's plan has no SpS
    for n in range(ofdm._PLAN_CAP):
        ofdm._carrier_plan(32 + 2 * n, 2, False, e, e)
    keys = ofdm.plan_cache_info()
    assert len(keys) == ofdm._PLAN_CAP and (16, 2, False, (), ()) not in keys
    again = ofdm._carrier_plan(16, 2, False, e, e)
    assert again is not first and again["key"] != first["key"]          # a plan's number never comes back
    ofdm.release_plans()
    assert ofdm.plan_cache_info() == []


def test_host_helpers():
    V = np.array([1 + 2j, 3 - 1j, 0.5j])
    h = oa.hermit(V)
    assert h.shape == (8,) and h[0] == 0 and h[4] == 0 and np.array_equal(h[1:4], V) and np.array_equal(h[5:], np.conj(V[::-1]))
    assert np.max(np.abs(np.fft.ifft(h).imag)) < 1e-15
    assert np.array_equal(oa.zeroPad(np.array([1, 2]), 2), [0, 0, 1, 2, 0, 0])
    assert oa.calcSymbolRate(16, 100e9, 512, 8, 4, False) == 100e9 / (504 / 516 * 4)
    assert oa.calcSymbolRate(16, 100e9, 512, 8, 4, True) == 100e9 / (247 / 516 * 4)


def test_the_names_are_exported_and_the_abi_has_the_symbols():
    for n in ("modulateOFDM", "demodulateOFDM", "hermit", "zeroPad", "calcSymbolRate"):
        assert n in oa.__all__ and callable(getattr(oa, n))
    header = open(os.path.join(ROOT, "include", "ssf.h")).read()
    for sym in ("ssf_ofdm_modulate", "ssf_ofdm_demodulate"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SYMBOLS
    assert "ssf_ofdm_params" in header
    assert [_lib.ofdm_frames_per_workgroup(L) for L in (16, 32, 256, 4096, 8192)] == [256, 128, 16, 1, 1]
    assert _lib.ofdm_lds_length(16) and _lib.ofdm_lds_length(8192) and not _lib.ofdm_lds_length(8) and not _lib.ofdm_lds_length(500)


def test_struct_layout_matches_the_header(tmp_path):
    import ctypes as C
    import subprocess
    lines = ['printf("size %zu\\n", sizeof(ssf_ofdm_params));']
    for f, _ in _lib.OfdmParams._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(ssf_ofdm_params, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    (tmp_path / "layout.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(_lib.OfdmParams)
    for f, _ in _lib.OfdmParams._fields_:
        assert int(got[f]) == getattr(_lib.OfdmParams, f).offset, f
