"""The synthetic shape rows of tests/clock_shape_cases.py on the GPU (run with -m gpu): the clock recovery bit-equal to the
restatement at every chunk, flush and end-of-output edge, at every fall the kernel accepts and refused where it must refuse, the
element-wise passes bit-equal to numpy at every size at which a kernel takes another path and at chosen output times, the clock
drift at peaks owned by chosen lanes and waves; through numpy arguments and through DeviceArrays."""
import numpy as np
import pytest

import clock_cases as cc
import clock_restatement as rs
import clock_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import _lib, clock
from test_gpu_clock import both_ways

pytestmark = pytest.mark.gpu


def test_the_rows_cover_what_they_claim():
    sc.check_coverage()


@pytest.mark.parametrize("name", [n for n in sc.GARDNER_ROWS if sc.GARDNER_ROWS[n]["want"] != "refuse"])
def test_clock_recovery_rows(name):
    r, want, tvw, info = sc.gardner_expect(name)
    out, tv = both_ways(lambda x: oa.gardnerClockRecovery(x, cc.Param(returnTiming=True, **r["p"])), np.array(r["x"]))
    assert out.shape == want.shape and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert tv.shape == tvw.shape and np.array_equal(tv.view(np.uint64), tvw.view(np.uint64))


@pytest.mark.parametrize("name", [n for n in sc.GARDNER_ROWS if sc.GARDNER_ROWS[n]["want"] == "refuse"])
def test_clock_recovery_refuses_a_fall_behind_what_left_lds(name):
    """Column 1 alone falls below f + 2: the call raises with that mode named (an error code of the engine, no fault), and the next
    call in the same process gives an ordinary row's bits."""
    r, _, _, info = sc.gardner_expect(name)
    assert r["status"] == [0, 1, 0] and [sc.kernel_status(col) for col in info["falls"]] == r["status"]
    for x in (np.array(r["x"]), oa.to_device(np.array(r["x"]))):
        with pytest.raises(RuntimeError, match="the loop of mode 1 fell back") as e:
            oa.gardnerClockRecovery(x, cc.Param(returnTiming=True, **r["p"]))
        assert "mode 0" not in str(e.value) and "mode 2" not in str(e.value)
        test_clock_recovery_rows("three_each")


def test_clock_recovery_one_dimensional_input_gives_one_dimension():
    r, want, tvw, _ = sc.gardner_expect("three_each")
    out, tv = both_ways(lambda x: oa.gardnerClockRecovery(x, cc.Param(returnTiming=True, **r["p"])), np.array(r["x"][:, 0]))
    assert out.shape == (want.shape[0],) and tv.shape == tvw.shape and np.array_equal(out, want[:, 0]) and np.array_equal(tv, tvw)


@pytest.mark.parametrize("i", range(len(sc.INTERP_ROWS)))
def test_interpolation_rows(i):
    x, inFs, outFs = sc.interp_input(i)
    y = both_ways(lambda v: oa.clockSamplingInterp(v, inFs, outFs), x)
    assert y.dtype == x.dtype and np.array_equal(y, rs.clock_interp(x, inFs, outFs))


def test_quantizer_table_of_one_level_more():
    k = sc.LONG_TABLE
    d = rs.quant_levels(k["nBits"], k["maxV"], k["minV"])
    assert len(d) == 2 ** k["nBits"] + 1
    x = np.concatenate([d, (d[:-1] + d[1:]) / 2, [d[-1] + 1, d[0] - 1, k["maxV"]], np.linspace(d[0], d[-1], 61)]).reshape(-1, 1)
    y = both_ways(lambda v: oa.quantizer(v, k["nBits"], k["maxV"], k["minV"]), x)
    assert np.array_equal(y, rs.quantizer(x, k["nBits"], k["maxV"], k["minV"])) and d[-1] in y


@pytest.mark.parametrize("i", range(len(sc.MINMAX_ROWS)))
def test_minmax_rows(i):
    x = sc.minmax_input(i)
    want = (min(x.real.min(), x.imag.min()), max(x.real.max(), x.imag.max())) if x.dtype.kind == "c" else (x.min(), x.max())
    for v in (x, oa.to_device(x)):
        assert clock._minmax(v) == (float(want[0]), float(want[1]))
        assert clock._minmax(v) == (float(want[0]), float(want[1]))


FORMS = dict(real=_lib.CLOCK_REAL, complex=_lib.CLOCK_COMPLEX, components=_lib.CLOCK_COMPONENTS)


@pytest.mark.parametrize("name", list(sc.TIMES_ROWS))
def test_interpolation_at_explicit_times(name):
    r, x, inFs, outFs, t_re, t_im, want = sc.interp_times_row(name)
    kw = dict(t_re=np.array(t_re)) if t_im is None else dict(t_re=np.array(t_re), t_im=np.array(t_im))
    for v in (np.array(x), oa.to_device(np.array(x))):
        for _ in range(2):
            y = clock._interp(v, inFs, outFs, FORMS[r["form"]], **kw)
            assert type(y) is type(v)
            assert sc.same_bits(y.get() if isinstance(y, oa.DeviceArray) else y, want)
    assert np.array_equal(kw["t_re"], t_re, equal_nan=True) and (t_im is None or np.array_equal(kw["t_im"], t_im, equal_nan=True))


@pytest.mark.parametrize("name", list(sc.DRIFT_ROWS))
def test_clock_drift_rows(name):
    r, t, want, per_column = sc.drift_expect(name)
    for v in (np.array(t), oa.to_device(np.array(t))):
        for _ in range(2):
            assert np.array_equal(oa.calcClockDrift(v), want, equal_nan=True)
            assert np.array_equal(clock._drift(v, 1), per_column, equal_nan=True)
    if name == "mixed600":
        assert np.isnan(want[2]) and np.all(want[[0, 1]] < 0)
        assert np.array_equal(oa.calcClockDrift(np.zeros(2)), [np.nan], equal_nan=True)
