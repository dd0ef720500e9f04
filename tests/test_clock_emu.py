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
    assert (k["chunk"], k["flush"], k["lag"]) == (sc.C, sc.F, sc.LAG) and k["lag"] + k["flush"] + 2 <= k["ring"]


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
    expect = r.get("status", [0] * r["cols"])
    assert status.tolist() == expect and [int(v) for v, s in zip(last, expect) if not s] == [v for v, s in zip(info["last_n"], expect) if not s]
    ok = [k for k, s in enumerate(expect) if not s]            # a refused column holds what it had when it was refused
    assert len(ok) >= 1 and tv.shape == tvw.shape and np.array_equal(tv[:, ok].view(np.uint64), tvw[:, ok].view(np.uint64))
    rows = sc.reach(r, info)
    if not any(expect):
        out = full[0:min(max(0, int(np.max(last))), q["Ln"]), :]
        assert out.shape == want.shape and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    else:
        assert rows <= want.shape[0]
        assert np.array_equal(np.ascontiguousarray(full[:rows, ok]).view(np.uint32), np.ascontiguousarray(want[:rows, ok]).view(np.uint32))
    assert not np.any(full[rows:][:, ok])                      # nothing beyond the furthest output


@pytest.mark.parametrize("name", list(sc.DRIFT_ROWS))
def test_clock_drift_rows(emu, name):
    """Peaks owned by chosen lanes and waves, at the array's ends, plateaus, fewer than two peaks, the sign of the mean, a mean per
    column: tests/clock_shape_cases.py DRIFT_ROWS."""
    r, t, want, per_column = sc.drift_expect(name)
    assert np.array_equal(emu.calcClockDrift(t), want, equal_nan=True), (emu.calcClockDrift(t), want)
    assert np.array_equal(emu.calcClockDrift(t, 1), per_column, equal_nan=True), (emu.calcClockDrift(t, 1), per_column)
    if name == "mixed600":
        assert np.isnan(want[2]) and np.all(want[[0, 1]] < 0)
        assert np.array_equal(emu.calcClockDrift(np.zeros(2)), [np.nan], equal_nan=True)


FORMS = dict(real=_lib.CLOCK_REAL, complex=_lib.CLOCK_COMPLEX, components=_lib.CLOCK_COMPONENTS)


@pytest.mark.parametrize("name", list(sc.TIMES_ROWS))
def test_interpolation_at_explicit_times(emu, name):
    r, x, inFs, outFs, t_re, t_im, want = sc.interp_times_row(name)
    kw = dict(t_re=np.array(t_re)) if t_im is None else dict(t_re=np.array(t_re), t_im=np.array(t_im))
    y = emu._interp(np.array(x), inFs, outFs, FORMS[r["form"]], **kw)
    assert sc.same_bits(y, want), np.argwhere(~(y == want))[:8]


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


def test_the_rows_cover_what_they_claim():
    sc.check_coverage()
