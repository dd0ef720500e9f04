"""The synthetic shape rows of tests/clock_shape_cases.py on the GPU (run with -m gpu): the clock recovery bit-equal to the
restatement at every chunk, flush and end-of-output edge, the element-wise passes bit-equal to numpy at every size at which a kernel
takes another path, through numpy arguments and through DeviceArrays."""
import numpy as np
import pytest

import clock_cases as cc
import clock_restatement as rs
import clock_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import clock
from test_gpu_clock import both_ways

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sc.GARDNER_ROWS))
def test_clock_recovery_rows(name):
    r, want, tvw, info = sc.gardner_expect(name)
    out, tv = both_ways(lambda x: oa.gardnerClockRecovery(x, cc.Param(returnTiming=True, **r["p"])), np.array(r["x"]))
    assert out.shape == want.shape and np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert tv.shape == tvw.shape and np.array_equal(tv.view(np.uint64), tvw.view(np.uint64))


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
