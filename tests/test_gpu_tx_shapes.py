"""The WDM transmitter on the GPU at every row of tests/tx_shape_cases.py (run with -m gpu): simpleWDMTx through ssf_wdm_tx against
oracle/tx_oracle.py -- symbols, wdmFreqGrid and pmf bit for bit, the field within 1e-12 of the largest expected sample, the bound
tests/test_gpu_tx.py holds the transmitter to -- at every block length, block edge, tap count, stuffing factor, grid, alphabet
and walk of the table; the device-generated walk against its extended-precision restatement; the C ABI's phi_rows and refusals.
Every row then runs again and must return the same bytes (every sum in the path has a fixed order, the device walk with a fixed key
included), and once more into a DeviceArray whose .get() has those bytes.  The rows run in table order, large and small in turn."""
import ctypes as C
import types

import numpy as np
import pytest

import opticommpy_amd as oa
import tx_shape_cases as ts
from opticommpy_amd import _lib, device

pytestmark = pytest.mark.gpu

REFUSAL = {"unsupported": RuntimeError}                # what simpleWDMTx ends in on this backend (_lib.raise_for)


def _wdm_tx(p, symbols, taps, phi, amp, deltaF, out, power):
    from opticommpy_amd.models import _state
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None   # noqa: E731
    return _lib.load().ssf_wdm_tx(_state["device"], C.byref(p), symbols.ctypes.data_as(C.c_void_p), dp(taps), dp(phi), dp(amp), dp(deltaF),
                                  device.out_ptr(out), dp(power))


API = types.SimpleNamespace(simpleWDMTx=oa.simpleWDMTx, wdm_tx=_wdm_tx, empty=lambda dev, shape: device.empty(dev, shape, np.complex128))


@pytest.mark.parametrize("row", ts.ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_expected_output(row):
    ts.check_conditions(row)
    if row.kind == "abi" and row.raises:
        assert ts.call(row, API) == ts.ERR_CODE[row.raises], row.id
        return
    if row.raises:
        with pytest.raises(REFUSAL[row.raises]):
            ts.call(row, API)
        return
    got = ts.call(row, API)
    ts.compare(row, got, "gpu")
    again = ts.call(row, API)
    assert again.sig.tobytes() == got.sig.tobytes(), row.id
    dev = ts.call(row, API, device_output=True)
    assert isinstance(dev.sig, oa.DeviceArray), row.id
    held = dev.sig.get()
    assert held.shape == got.sig.shape and held.tobytes() == got.sig.tobytes(), row.id
    if row.kind != "abi":
        assert np.array_equal(dev.symb, got.symb), row.id


def test_two_keys_give_two_fields():
    a, b = (ts.call(ts.BY_ID[f"walk-device-key{i}-n4100"], API) for i in (0, 1))
    assert np.array_equal(a.symb, b.symb)
    assert np.max(np.abs(a.sig - b.sig)) > 1e-3 * np.max(np.abs(a.sig))
