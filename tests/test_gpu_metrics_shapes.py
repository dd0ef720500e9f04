"""The link-metrics kernels on the GPU against the numpy restatement (tests/metrics_restatement.py) at the shapes no recorded
fixture has (run with -m gpu): every label width, every input type, lengths either side of a wave, a workgroup and the grid-stride
threshold, up to 64 modes in both layouts with a first-row offset, the blind EVM's float32 pairwise sum across its chunk edge and
with a second workgroup of leaves, and calls in an order where a small one follows a large one on the cached work buffers.

The rows and their conditions are in tests/metrics_shape_cases.py; tests/test_metrics_restatement.py holds the restatement to
the reference's fixtures at 1e-12 and runs the same rows through the emulator of the kernel bodies.

Bounds: BER and SER equal the restatement's with == (a decision margin of 1e-6 is asserted, so rounding cannot flip a decision);
SNR [dB], GMI, NGMI, MI and EVM within metrics_cases.REL = 1e-9; the blind EVM within 1e-12 of the numpy expression (a float32
sum in another order is about 1e-8 off); hard decisions bit for bit; pnorm within 1e-12 rel-L2 and signalPower within 1e-12
relative.  Every row runs through numpy arguments and through DeviceArrays, which must agree bit for bit."""
import numpy as np
import pytest

import metrics_restatement as mr
import metrics_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


def call(row, rx, tx, px):
    if row.kind == "metrics":
        return dict(oa.metrics(rx, tx, row.M, row.ct, px=px, discard=row.discard))
    if row.kind == "blind":
        return {"EVM": oa.calcEVM(rx, row.M, row.ct, discard=row.discard)}
    return {"bits": oa.demodulateGray(rx, row.M, row.ct)}


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.id)
def test_row_matches_the_restatement(row):
    rx0, tx0, px = sc.arrays(row)
    want = sc.expected(row)
    sc.check_conditions(row, want)

    rx, tx = rx0.copy(), None if tx0 is None else tx0.copy()
    a = call(row, rx, tx, px)
    sc.compare(row, a, want, "numpy")
    assert np.array_equal(rx, rx0) and (tx is None or np.array_equal(tx, tx0))

    rd, td = oa.to_device(rx0), None if tx0 is None else oa.to_device(tx0)
    assert rd.dtype == rx0.dtype and rd.shape == rx0.shape
    before = device.transfer_counts()
    b = call(row, rd, td, px)
    assert device.transfer_counts() == before
    if row.kind == "demod":
        assert isinstance(b["bits"], oa.DeviceArray)
        b["bits"] = b["bits"].get()
    sc.compare(row, b, want, "device")
    for k in a:
        assert np.array_equal(a[k], b[k]), (row.id, k)
    assert np.array_equal(rd.get(), rx0) and (td is None or np.array_equal(td.get(), tx0))


def test_numpy_arguments_of_two_types_are_widened_and_device_arrays_are_not():
    """rx complex64 with tx complex128 is the call with both complex128; the same pair on the device raises."""
    row = sc.BY_ID["type-psk8-2085x2-complex64"]
    rx32, tx32, _ = sc.arrays(row)
    tx = tx32.astype(np.complex128)
    want = mr.restate(rx32, tx, row.M, row.ct)
    sc.check_conditions(row, want)
    mixed = dict(oa.metrics(rx32, tx, row.M, row.ct))
    sc.compare(row, mixed, want, "complex64 / complex128")
    wide = oa.metrics(rx32.astype(np.complex128), tx, row.M, row.ct)
    for k in mixed:
        assert np.array_equal(mixed[k], wide[k]), k
    for f in (oa.metrics, oa.fastBERcalc, oa.monteCarloGMI, oa.monteCarloMI):
        with pytest.raises(TypeError):
            f(oa.to_device(rx32), oa.to_device(tx), row.M, row.ct)
    with pytest.raises(TypeError):
        oa.calcEVM(oa.to_device(rx32), row.M, row.ct, symbTx=oa.to_device(tx))


def _helper_inputs():
    rng = np.random.default_rng(5)
    return {"float32-1000x3": (1.7 * rng.normal(size=(1000, 3))).astype(np.float32),
            "complex64-131073": (0.4 * (rng.normal(size=131073) + 1j * rng.normal(size=131073))).astype(np.complex64),
            "one-element": np.array([-2.5 + 1.5j])}


@pytest.mark.parametrize("name", ["float32-1000x3", "complex64-131073", "one-element"])
def test_pnorm_and_signal_power(name):
    x = _helper_inputs()[name]
    want_y, want_p = mr.pnorm(x), mr.signal_power(x)
    xd = oa.to_device(x)
    before = device.transfer_counts()
    yd, pd = oa.pnorm(xd), oa.signalPower(xd)
    assert device.transfer_counts() == before
    y, p = oa.pnorm(x), oa.signalPower(x)
    assert isinstance(y, np.ndarray) and y.shape == x.shape and y.dtype == want_y.dtype
    assert isinstance(yd, oa.DeviceArray) and yd.shape == x.shape and np.array_equal(yd.get(), y) and pd == p
    assert np.array_equal(xd.get(), x)
    e_y = float(np.linalg.norm(np.ravel(y) - np.ravel(want_y)) / np.linalg.norm(np.ravel(want_y)))
    e_p = abs(p - want_p) / want_p
    print(f"{name}: pnorm rel-L2 {e_y:.2e}, signalPower rel {e_p:.2e}")
    assert e_y <= 1e-12 and e_p <= 1e-12


def test_a_small_call_after_a_large_one_on_the_cached_buffers():
    """The work buffers only grow and the functions share them: each call of the sequence (10 elements, 64 modes, 3 x 40001 blind,
    3 symbols, 131073 elements) gives, bit for bit, what the same call gave when it was made first, and that is the restatement's."""
    x10 = _helper_inputs()["float32-1000x3"].reshape(-1)[:10].copy()
    xbig = _helper_inputs()["complex64-131073"]
    wide, tiny, blind = sc.BY_ID["layout-qam16-300x64"], sc.BY_ID["n-qam16-3"], sc.BY_ID["blind-qam64-40001x3"]
    steps = [lambda: {"y": oa.pnorm(x10)},
             lambda: call(wide, *sc.arrays(wide)),
             lambda: call(blind, *sc.arrays(blind)),
             lambda: call(tiny, *sc.arrays(tiny)),
             lambda: {"p": np.array(oa.signalPower(xbig))}]
    # made first: smallest call first, so that none of them follows a larger one of this test
    first = [None] * len(steps)
    for i in (0, 3, 1, 4, 2):
        first[i] = steps[i]()
    for i, step in enumerate(steps):
        got = step()
        for k in got:
            assert np.array_equal(got[k], first[i][k]), (i, k)
    # and against the restatement: the values are right, not only repeated
    assert np.linalg.norm(first[0]["y"] - mr.pnorm(x10)) <= 1e-12 * np.linalg.norm(mr.pnorm(x10))
    sc.compare(wide, first[1], sc.expected(wide), "first")
    sc.compare(blind, first[2], sc.expected(blind), "first")
    sc.compare(tiny, first[3], sc.expected(tiny), "first")
    assert abs(float(first[4]["p"]) - mr.signal_power(xbig)) <= 1e-12 * mr.signal_power(xbig)
