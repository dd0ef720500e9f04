"""The sampling clock on the GPU against the reference's recorded results (tests/golden/clock/*.npz, tools/gen_golden_clock.py),
through numpy arguments and through DeviceArrays (run with -m gpu), at the bounds of tests/clock_cases.py.  Every call is made
twice: numpy and device calls give the same bits, repeat calls give the same bits, inputs are never written and no
DeviceArray.get / .set happens inside a call on DeviceArrays."""
import logging

import numpy as np
import pytest

import clock_cases as cc
import clock_restatement as rs
import opticommpy_amd as oa
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


def host(a):
    if isinstance(a, tuple):
        return tuple(host(v) for v in a)
    return a.get() if isinstance(a, oa.DeviceArray) else a


def as_tuple(a):
    return a if isinstance(a, tuple) else (a,)


def both_ways(run, x0):
    """run(x) on a numpy copy and on a DeviceArray, twice each: the host result, after the checks the docstring lists."""
    results = {}
    for kind in ("numpy", "device"):
        x = oa.to_device(x0) if kind == "device" else x0.copy()
        before = device.transfer_counts()
        first, second = run(x), run(x)
        after = device.transfer_counts()
        for r in as_tuple(first):
            assert type(r) is (oa.DeviceArray if kind == "device" else np.ndarray), kind
        if kind == "device":
            assert after == before, (before, after)
            assert np.array_equal(x.get(), x0)
        else:
            assert np.array_equal(x, x0)
        a, b = host(first), host(second)
        for u, v in zip(as_tuple(a), as_tuple(b)):
            assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), kind
        results[kind] = a
    for u, v in zip(as_tuple(results["numpy"]), as_tuple(results["device"])):
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
    return results["numpy"]


@pytest.mark.parametrize("name", cc.INTERP)
def test_interpolation_matches_the_reference(name):
    g = cc.load("interp", name)
    cc.check_conditions("interp", g)
    y = both_ways(lambda x: cc.run_interp(oa, g, x), g["x"])
    assert y.dtype == g["y"].dtype and np.array_equal(y, g["y"])


@pytest.mark.parametrize("name", cc.QUANT)
def test_quantizer_matches_the_reference(name):
    g = cc.load("quant", name)
    cc.check_conditions("quant", g)
    c = g["cfg"]
    assert np.array_equal(both_ways(lambda x: cc.run_quant(oa, g, x), g["x"]), g["y"])
    x32 = g["x"].astype(np.float32)
    assert np.array_equal(both_ways(lambda x: cc.run_quant(oa, g, x), x32), rs.quantizer(x32, c["nBits"], c["maxV"], c["minV"]))
    z = g["x"] + 1j * g["x"][::-1]
    assert np.array_equal(both_ways(lambda x: cc.run_quant(oa, g, x), z), g["y"])          # of complex data the real part


@pytest.mark.parametrize("name", cc.CONV)
def test_converters_match_the_reference(name):
    g = cc.load("conv", name)
    cc.check_conditions("conv", g)
    sig = g["sigIn"]
    if sig.dtype == np.complex128:
        out = both_ways(lambda x: cc.run_conv(oa, g, x), sig)
    else:                                   # real or single-precision input: numpy only (the device filters take complex128)
        out = cc.run_conv(oa, g, sig.copy())
        assert cc.run_conv(oa, g, sig.copy()).tobytes() == out.tobytes()
        with pytest.raises(TypeError, match="complex128"):
            cc.run_conv(oa, g, oa.to_device(sig))
    print(name, "distance to the reference / max |ref|:", cc.check_conv(name, g, out))


def test_converter_defaults_are_written_back():
    g = cc.load("conv", "adc_defaults")
    p = cc.Param()
    oa.adc(oa.to_device(g["sigIn"]), p)
    assert vars(p) == dict(inFs=1, outFs=1, jitter=0, nBits=8, ENOB=8, Vmax=1, Vmin=-1, AAF=True, N=201)
    p = cc.Param()
    oa.dac(g["sigIn"], p)
    assert vars(p) == dict(inFs=1, outFs=1, nBits=8, ENOB=8, jitter=0, Vpp=2, AIF=True, N=201)


@pytest.mark.parametrize("name", cc.GARDNER)
def test_clock_recovery_matches_restatement_and_reference(name):
    g = cc.load("gardner", name)
    cc.check_conditions("gardner", g)
    out, tv = both_ways(lambda x: cc.run_gardner(oa, g, x), g["x"])
    print(name, cc.check_gardner(g, out, tv))
    alone = oa.gardnerClockRecovery(g["x"], cc.Param(**dict(g["cfg"]["p"], returnTiming=False)))
    assert isinstance(alone, np.ndarray) and alone.tobytes() == out.tobytes()
    for t in (tv, oa.to_device(tv)):
        before = device.transfer_counts()
        drift = oa.calcClockDrift(t)
        assert device.transfer_counts() == before
        assert np.array_equal(drift, rs.clock_drift(tv), equal_nan=True)
    assert [None if np.isnan(v) else float(v) for v in oa.calcClockDrift(g["tv"])] == g["cfg"]["drift"]


def test_clock_recovery_logs_the_drift_only_at_info(caplog):
    g = cc.load("gardner", "p300_nyq_c128")
    with caplog.at_level(logging.INFO):
        cc.run_gardner(oa, g)
    lines = [r.getMessage() for r in caplog.records if "Estimated clock drift" in r.getMessage()]
    assert lines == [f"Estimated clock drift mode 0: {g['cfg']['drift'][0]:.2f} ppm"]
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        cc.run_gardner(oa, g)
    assert not caplog.records


def test_chain_adc_pnorm_clock_recovery_stays_on_the_device():
    """adc -> pnorm -> gardnerClockRecovery on DeviceArrays: no host copy in between, the result of the same calls on host arrays;
    on the signal sampled 300 ppm fast the recovered symbols ``out[0::2]`` decide with BER <= 0.02 in both modes (1500 symbols
    discarded each side) and the unrecovered adc output with BER >= 0.3.  These are conditions, not measurements: the reference
    alone, on the signal its own functions build from the same seed (tools/gen_golden_clock.py chain_ber; tests/clock_cases.py:
    CHAIN_REFERENCE_BER), gives BER [0.00430, 0.00385] recovered and [0.49475, 0.49905] unrecovered."""
    mid, symb = cc.chain_signal(oa)
    prm = cc.chain_adc_param(mid)
    runs = {}
    for kind in ("numpy", "device"):
        x = oa.to_device(mid) if kind == "device" else mid
        np.random.seed(5)
        before = device.transfer_counts()
        rx = oa.pnorm(oa.adc(x, cc.Param(**vars(prm))))
        out = oa.gardnerClockRecovery(rx, cc.Param(**cc.CHAIN_GARDNER))
        if kind == "device":
            assert device.transfer_counts() == before and isinstance(out, oa.DeviceArray) and isinstance(rx, oa.DeviceArray)
        runs[kind] = (host(rx), host(out))
    assert runs["numpy"][0].tobytes() == runs["device"][0].tobytes() and runs["numpy"][1].tobytes() == runs["device"][1].tobytes()
    rx, out = runs["device"]
    assert out.dtype == np.complex64 and out.shape[1] == 2
    for label, y in (("recovered", out[0::2]), ("unrecovered", rx[0::2])):
        n = min(len(y), len(symb))
        ber = oa.fastBERcalc(np.ascontiguousarray(y[:n]).astype(np.complex128), symb[:n], 16, "qam", discard=1500)[0]
        print(label, "BER", ber)
        assert np.all(ber <= 0.02) if label == "recovered" else np.all(ber >= 0.3), (label, ber)
