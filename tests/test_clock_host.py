"""Host side of the sampling clock (opticommpy_amd/clock.py) without a GPU: what is out of scope is refused before the library is
even loaded, defaults are written back as the reference writes them, output lengths, quantizer tables and the order of the random
draws are the reference's, and the parameter structs are packed as include/ssf.h lays them out."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import clock_cases as cc
import clock_restatement as rs
import opticommpy_amd as oa
from opticommpy_amd import _lib, clock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the checks under test come before it."""
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def fake_device(shape, dtype):
    d = object.__new__(oa.DeviceArray)                      # (no GPU needed: the checks are on type and shape)
    d.shape, d.dtype, d.device, d._ptr, d._owner = tuple(shape), np.dtype(dtype), 0, None, d
    return d


X = (np.arange(64).reshape(32, 2) + 1j).astype(np.complex128)


def test_public_names():
    for name in clock.__all__:
        assert getattr(oa, name) is getattr(clock, name) and name in oa.__all__
    assert set(clock.__all__) == {"clockSamplingInterp", "quantizer", "resample", "adc", "dac", "gardnerClockRecovery", "calcClockDrift",
                                  "gardnerTED", "gardnerTEDnyquist", "interpolator"}


def test_the_package_does_not_import_scipy():
    code = "import sys; import opticommpy_amd; assert 'scipy' not in sys.modules, 'scipy was imported'"
    subprocess.check_call([os.sys.executable, "-c", code], cwd=ROOT)


@pytest.mark.parametrize("call", [
    lambda: oa.clockSamplingInterp(X[:, 0], 1, 2),                                   # 1-D: the reference needs two dimensions
    lambda: oa.clockSamplingInterp(X, 0, 2), lambda: oa.clockSamplingInterp(X, 1, -2), lambda: oa.clockSamplingInterp(X, 1, 2, -1e-12),
    lambda: oa.clockSamplingInterp(np.zeros((0, 2)), 1, 2),
    lambda: oa.quantizer(X.real[:, 0]), lambda: oa.quantizer(X.real, 0), lambda: oa.quantizer(X.real, 2.5), lambda: oa.quantizer(X.real, 33),
    lambda: oa.quantizer(X.real, 8, -1, 1), lambda: oa.quantizer(X.real, 8, 1, 1), lambda: oa.quantizer(X.real, 8, np.inf, 0),
    lambda: oa.resample(X, cc.Param(inFs=0, outFs=1)), lambda: oa.resample(np.zeros((2, 2, 2)), cc.Param()), lambda: oa.resample(X, cc.Param(N=0, outFs=1)),
    lambda: oa.adc(X, cc.Param(nBits=0)), lambda: oa.adc(X, cc.Param(Vmax=-1, Vmin=1)), lambda: oa.adc(X, cc.Param(outFs=-1)),
    lambda: oa.adc(X, cc.Param(jitter=-1)), lambda: oa.adc(X, cc.Param(N=0)),
    lambda: oa.dac(X, cc.Param(nBits=40)), lambda: oa.dac(X, cc.Param(inFs=np.nan)),
    lambda: oa.gardnerClockRecovery(X, cc.Param(lpad=-1)), lambda: oa.gardnerClockRecovery(X, cc.Param(lpad=0.5)),
    lambda: oa.gardnerClockRecovery(X, cc.Param(kp=np.nan)), lambda: oa.gardnerClockRecovery(X[:1], cc.Param(lpad=0)),
    lambda: oa.gardnerClockRecovery(np.zeros((4, 2, 2), complex)), lambda: oa.gardnerClockRecovery(np.zeros((0, 2), complex)),
    lambda: oa.calcClockDrift(np.zeros((2, 2, 2))), lambda: oa.calcClockDrift(np.zeros((0, 2))),
])
def test_out_of_scope_arguments_raise_before_the_library_loads(no_library, call):
    with pytest.raises(ValueError):
        call()


def test_types_are_checked_before_the_library_loads(no_library):
    with pytest.raises(TypeError, match="complex128, complex64, float64, float32"):
        oa.clockSamplingInterp(fake_device((8, 2), np.int32), 1, 2)
    with pytest.raises(TypeError):
        oa.quantizer(fake_device((8, 2), np.int16))
    for fn in (oa.resample, oa.adc, oa.dac):
        for dtype in (np.complex64, np.float64, np.float32):
            with pytest.raises(TypeError, match="complex128"):
                fn(fake_device((8, 2), dtype), cc.Param())
    for x in (X.astype(np.complex64), X.real.astype(np.float32)):
        with pytest.raises(TypeError, match="double precision"):
            oa.dac(x, cc.Param())
    with pytest.raises(TypeError, match="complex128, complex64"):
        oa.gardnerClockRecovery(fake_device((8, 2), np.float64))
    with pytest.raises(TypeError, match="float64"):
        oa.calcClockDrift(fake_device((8, 2), np.float32))
    with pytest.raises(TypeError):
        oa.clockSamplingInterp(np.array([["a", "b"]]), 1, 2)


def test_defaults_are_written_back_before_anything_else(no_library):
    p = cc.Param(nBits=0)
    with pytest.raises(ValueError):
        oa.adc(X, p)
    assert vars(p) == dict(nBits=0, inFs=1, outFs=1, jitter=0, ENOB=8, Vmax=1, Vmin=-1, AAF=True, N=201)
    p = cc.Param(nBits=0)
    with pytest.raises(ValueError):
        oa.dac(X, p)
    assert vars(p) == dict(nBits=0, inFs=1, outFs=1, ENOB=8, jitter=0, Vpp=2, AIF=True, N=201)
    p = cc.Param(inFs=-1)                                            # resample and the clock recovery write nothing back
    with pytest.raises(ValueError):
        oa.resample(X, p)
    assert vars(p) == dict(inFs=-1)
    q = clock._prepare_gardner(X)
    assert (q["params"].kp, q["params"].ki, q["params"].nyquist, q["params"].lpad, q["returnTiming"]) == (1e-3, 1e-6, 1, 1, False)
    assert q["Ln"] == int((1 - 500 / 1e6) * 33) and not q["input1D"]


def test_output_length_is_numpys_arange_rule():
    for N, inFs, outFs in ((2000, 64e9, 64e9), (3001, 64e9, 64e9 * 0.5 * (1 + 105e-6)), (1500, 64e9, 128e9), (3000, 64e9, 64e9 / 3), (1, 1, 7),
                           (7, 3.0, 1.0), (1000, 1.28e11, 1.28e11 * (1 + 75e-6))):
        inTs, outTs = 1 / inFs, 1 / outFs
        assert clock.output_length(N, inTs, outTs) == len(np.arange(0, N * inTs, outTs)), (N, inFs, outFs)
    assert clock.output_length(2000, 1 / 64e9, 1 / 64e9) == 2001          # numpy's rule, not N: the quotient rounds up


def test_quantizer_table_is_numpys_arange():
    rng = np.random.default_rng(0)
    longer = 0
    for _ in range(300):
        nBits = int(rng.integers(1, 11))
        minV, maxV = sorted(rng.uniform(-2, 2, size=2))
        d = rs.quant_levels(nBits, maxV, minV)
        qmin, qdelta, levels = clock.quant_table(nBits, maxV, minV)
        assert levels == len(d) and np.array_equal(qmin + np.arange(levels) * qdelta, d)
        longer += levels == 2 ** nBits + 1
    assert longer > 0                                                # the table of one level more does occur
    assert clock.quant_table(8, 1, -1)[2] == 256 and clock.quant_table(8, np.float64(1), np.int64(-1)) == clock.quant_table(8, 1, -1)


def test_jitter_and_noise_draws_follow_the_reference_order():
    """adc on complex input: two jitter draws (the real parts' first), then the complex ENOB noise (real parts, then imaginary)."""
    N, inFs, outFs, jitter = 100, 64e9, 64e9 * 0.5 * (1 + 105e-6), 1e-12
    np.random.seed(11)
    t_re = clock.output_times(N, 1 / inFs, 1 / outFs, jitter)
    t_im = clock.output_times(N, 1 / inFs, 1 / outFs, jitter)
    noise = clock._extra_noise((len(t_re), 2), True, 2.0, 8, 6.5)
    np.random.seed(11)
    want_re, want_im = rs.jittered(N, inFs, outFs, jitter), rs.jittered(N, inFs, outFs, jitter)
    Pn = 2.0 ** 2 / (12 * (2 ** (2 * 6.5))) - 2.0 ** 2 / (12 * (2 ** (2 * 8)))
    want_noise = np.random.normal(0, np.sqrt(2 * Pn / 2), (len(t_re), 2)) + 1j * np.random.normal(0, np.sqrt(2 * Pn / 2), (len(t_re), 2))
    assert np.array_equal(t_re, want_re) and np.array_equal(t_im, want_im) and not np.array_equal(t_re, t_im)
    assert np.array_equal(noise, want_noise)
    state = np.random.get_state()[1].copy()
    assert clock.output_times(N, 1 / inFs, 1 / outFs, 0) is None and np.array_equal(np.random.get_state()[1], state)   # no jitter: no draw
    np.random.seed(12)
    real_noise = clock._extra_noise((5, 1), False, 2.0, 8, 6.5)
    np.random.seed(12)
    assert np.array_equal(real_noise, np.random.normal(0, np.sqrt(Pn), (5, 1)))


def test_interpolation_plans():
    q = clock._plan_interp(X, 2.0, 1.0, _lib.CLOCK_COMPONENTS, clip=(-1, 1), quant=clock.quant_table(8, 1, -1))
    p = q["params"]
    assert (p.n_in, p.n_out, p.ncols, p.dtype, p.form, p.clip, p.quantize, p.qlevels) == (32, 16, 2, 0, 2, 1, 1, 256)
    assert q["shape"] == (16, 2) and q["dtype"] == np.complex128
    q = clock._plan_interp(X.real.astype(np.float32), 1.0, 2.0, _lib.CLOCK_REAL, clip=(-0.1, 0.1))
    assert q["dtype"] == np.float32 and (q["params"].lo, q["params"].hi) == (float(np.float32(-0.1)), float(np.float32(0.1)))


def test_scalar_helpers_are_the_references_expressions():
    x = np.array([0.3 - 0.2j, -1.1 + 0.4j, 0.7 + 0.9j, -0.5 - 0.6j])
    assert oa.gardnerTED(x[:3]) == np.real(np.conj(x[1]) * (x[2] - x[0]))
    assert oa.gardnerTEDnyquist(x[:3]) == np.abs(x[1]) ** 2 * (np.abs(x[0]) ** 2 - np.abs(x[2]) ** 2)
    assert oa.interpolator(x, 0.0) == x[2] and oa.interpolator(x, -1.0) == pytest.approx(x[1]) and oa.interpolator(x, 1.0) == pytest.approx(x[3])
    c = rs.farrow(0.37)
    assert oa.interpolator(x, 0.37) == pytest.approx(sum(ci * xi for ci, xi in zip(c, x)), rel=1e-14)
    assert math.isclose(sum(c), 1.0, rel_tol=1e-15)


def test_struct_layouts_match_header(tmp_path):
    structs = {"ssf_clock_params": _lib.ClockParams, "ssf_gardner_params": _lib.GardnerParams}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_library_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    p = _lib.ClockParams(n_in=4, n_out=4, ncols=1, dtype=0, form=_lib.CLOCK_REAL, inTs=1.0, outTs=1.0, qlevels=1, qdelta=1.0)
    buf = (C.c_double * 16)()
    assert lib.ssf_clock_interp(0, C.byref(p), buf, None, None, buf) == -1              # a complex dtype with the real form
    p.form, p.outTs = _lib.CLOCK_COMPLEX, 0.0
    assert lib.ssf_clock_interp(0, C.byref(p), buf, None, None, buf) == -1
    assert lib.ssf_quantize(0, 4, 2, 0.0, 0.0, 4, buf, buf) == -1                       # a table without a step
    assert lib.ssf_clip(0, 4, 2, 1.0, -1.0, buf, buf) == -1 and lib.ssf_minmax(0, 0, 2, buf, buf) == -1
    g = _lib.GardnerParams(n=4, lpad=1, Ln=4, nModes=1, dtype=2, nyquist=1, kp=1e-3, ki=1e-6)
    last = (C.c_int64 * 1)()
    assert lib.ssf_gardner(0, C.byref(g), buf, buf, buf, last) == -1                    # a real dtype
    assert lib.ssf_clock_drift(0, 0, 1, 0, buf, buf) == -1 and lib.ssf_clock_scale_add(0, 0, 1.0, 1, buf, None, buf) == -1
