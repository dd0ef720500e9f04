"""The sampling-clock kernels walked on the CPU (tests/emu/emu_clock.cpp loops the bodies of opticommpy_amd/csrc/clock_kernels.h in
the launch geometry) over every fixture and every shape row, at the bounds of tests/clock_cases.py: the converters bit-equal to the
reference's recorded results, the clock recovery bit-equal to the restatement."""
import numpy as np
import pytest

import clock_cases as cc
import clock_restatement as rs
import clock_shape_cases as sc
from opticommpy_amd import _lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return cc.Emu(cc.build_emu(tmp_path_factory), tmp_path_factory.mktemp("clock_io"))


def test_constants_are_the_bindings(emu):
    k = cc.emu_constants(emu.exe)
    assert k == dict(chunk=_lib.CLOCK_CHUNK, win=_lib.CLOCK_CHUNK + 4, ring=_lib.CLOCK_RING, flush=_lib.CLOCK_FLUSH, lag=_lib.CLOCK_LAG,
                     block=_lib.CLOCK_BLOCK, max_blocks=_lib.CLOCK_MAX_BLOCKS)
    assert (k["chunk"], k["flush"]) == (sc.C, sc.F) and k["lag"] + k["flush"] + 2 <= k["ring"]


@pytest.mark.parametrize("name", cc.INTERP)
def test_interpolation_fixtures(emu, name):
    g = cc.load("interp", name)
    cc.check_conditions("interp", g)
    y = cc.run_interp(emu, g)
    assert y.dtype == g["y"].dtype and np.array_equal(y, g["y"])


@pytest.mark.parametrize("name", cc.QUANT)
def test_quantizer_fixtures(emu, name):
    g = cc.load("quant", name)
    cc.check_conditions("quant", g)
    assert np.array_equal(cc.run_quant(emu, g), g["y"])
    assert np.array_equal(cc.run_quant(emu, g, g["x"].astype(np.float32)), rs.quantizer(g["x"].astype(np.float32), g["cfg"]["nBits"],
                                                                                           g["cfg"]["maxV"], g["cfg"]["minV"]))


@pytest.mark.parametrize("name", [n for n in cc.CONV if n not in cc.FILTERS])
def test_converter_fixtures_without_filters(emu, name):
    g = cc.load("conv", name)
    cc.check_conditions("conv", g)
    cc.check_conv(name, g, cc.run_conv(emu, g))


@pytest.mark.parametrize("name", cc.GARDNER)
def test_clock_recovery_fixtures(emu, name):
    g = cc.load("gardner", name)
    cc.check_conditions("gardner", g)
    out, tv = cc.run_gardner(emu, g)
    cc.check_gardner(g, out, tv)
    drift = emu.calcClockDrift(tv)
    want = rs.clock_drift(tv)
    assert np.array_equal(drift, want, equal_nan=True)
    assert [None if np.isnan(v) else float(v) for v in emu.calcClockDrift(g["tv"])] == g["cfg"]["drift"]


@pytest.mark.parametrize("name", list(sc.GARDNER_ROWS))
def test_clock_recovery_rows(emu, name):
    r, want, tvw, info = sc.gardner_expect(name)
    full, tv, last, status, q = emu.gardner_raw(r["x"], cc.Param(returnTiming=True, **r["p"]))
    assert not np.any(status) and last.tolist() == info["last_n"]
    out = full[0:min(max(0, int(np.max(last))), q["Ln"]), :]
    assert out.shape == want.shape and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert tv.shape == tvw.shape and np.array_equal(tv.view(np.uint64), tvw.view(np.uint64))
    assert not np.any(full[out.shape[0]:])                      # nothing beyond the furthest output


def test_clock_drift_rows(emu):
    """Peaks at the array's ends, a plateau, fewer than two peaks, a negative mean, a mean per column."""
    t = np.zeros((600, 4))
    t[100:, 0] += 1.0
    t[350:, 0] -= 1.0
    t[500:, 0] += 1.0                                            # three gaps: periods 250 and 150
    t[2:, 1] -= 1.0
    t[598:, 1] += 1.0                                            # gaps at the first and the last difference a peak can sit on
    t[:, 1] -= 5.0
    t[300:, 2] += 1.0                                            # one gap: nan
    t[10:, 3] += 0.7
    t[12:, 3] += 0.7                                             # a plateau of two equal differences apart... and a second peak
    t[200:, 3] += 0.9
    for per_column in (0, 1):
        got = emu.calcClockDrift(t, per_column)
        want = rs.clock_drift(t) if not per_column else np.array([rs.clock_drift(t[:, k])[0] for k in range(4)])
        assert np.array_equal(got, want, equal_nan=True), (per_column, got, want)
    assert np.isnan(emu.calcClockDrift(t)[2]) and np.all(emu.calcClockDrift(t)[[0, 1]] < 0)
    assert np.array_equal(emu.calcClockDrift(np.zeros(2)), [np.nan], equal_nan=True)


@pytest.mark.parametrize("i", range(len(sc.INTERP_ROWS)))
def test_interpolation_rows(emu, i):
    x, inFs, outFs = sc.interp_input(i)
    y = emu.clockSamplingInterp(x, inFs, outFs)
    assert y.dtype == x.dtype and np.array_equal(y, rs.clock_interp(x, inFs, outFs))


def test_quantizer_table_of_one_level_more(emu):
    k = sc.LONG_TABLE
    d = rs.quant_levels(k["nBits"], k["maxV"], k["minV"])
    assert len(d) == 2 ** k["nBits"] + 1
    x = np.concatenate([d, (d[:-1] + d[1:]) / 2, [d[-1] + 1, d[0] - 1, k["maxV"]], np.linspace(d[0], d[-1], 61)]).reshape(-1, 1)
    y = emu.quantizer(x, k["nBits"], k["maxV"], k["minV"])
    assert np.array_equal(y, rs.quantizer(x, k["nBits"], k["maxV"], k["minV"])) and d[-1] in y


@pytest.mark.parametrize("i", range(len(sc.MINMAX_ROWS)))
def test_minmax_rows(emu, i):
    x = sc.minmax_input(i)
    want = (min(x.real.min(), x.imag.min()), max(x.real.max(), x.imag.max())) if x.dtype.kind == "c" else (x.min(), x.max())
    assert emu.minmax(x) == (float(want[0]), float(want[1]))
    if x.dtype.kind == "c":
        assert want[1] == 3.5 and (len(x) == 1 or want[0] == -2.5)


def test_complex_clip_is_lexicographic(emu):
    rng = np.random.default_rng(9)
    z = (rng.uniform(-2, 2, size=(300, 2)) + 1j * rng.uniform(-2, 2, size=(300, 2)))
    z[:6, 0] = [-1 - 3j, -1 + 3j, 1 - 3j, 1 + 3j, -1 - 1j, 1 + 1j]        # real parts on the bounds
    for x in (z, z.astype(np.complex64), z.real.copy(), z.real.astype(np.float32)):
        if x.dtype.kind == "c":
            want = np.clip(x, -1 - 1j, 1 + 1j)
            assert np.any(np.abs(want.imag) > 1)                 # a real part strictly inside leaves the imaginary part alone
        else:
            want = np.clip(x, -1, 1)
        got = emu.clip(x, -1, 1)
        assert got.dtype == x.dtype and np.array_equal(got, want)
