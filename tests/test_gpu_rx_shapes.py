"""The receiver front end on the GPU at every row of tests/rx_shape_cases.py (run with -m gpu): filters, delays and decimate
against the extended-precision time-domain restatement (tests/rx_restatement.py), the receiver models and the chain against
oracle/rx_oracle.py, at the bounds tests/test_gpu_rx.py and tests/test_round6.py already hold them to -- filters rel-L2 1e-13,
receiver 1e-12 and chain 1e-11 of the largest expected value, decimate and the hybrid bit for bit.  Every row then runs again on
DeviceArrays where the function takes them: no transfer, a DeviceArray back, the numpy call's bits, the inputs untouched.  (One
exception: balancedPD of two 1-D DeviceArrays is two photodiode calls and a subtraction, the numpy call one launch that subtracts
in front of the common filter -- two roundings of one result, so that row's DeviceArray call is held to the oracle's bound.)"""
import builtins
import ctypes as C
import types

import numpy as np
import pytest

import opticommpy_amd as oa
import rx_shape_cases as rs
from opticommpy_amd import _lib, device

pytestmark = pytest.mark.gpu


def _overlap_save(N, ncols, nfft, K, H, x):
    lib = _lib.load()
    out = np.empty_like(x)
    _lib.raise_for(lib, None, lib.ssf_overlap_save(0, N, ncols, _lib.SSF_C128, nfft, K, H.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                                   out.ctypes.data_as(C.c_void_p)))
    return out


API = types.SimpleNamespace(parameters=oa.parameters, overlap_save=_overlap_save,
                            **{f: getattr(oa, f) for f in ("firFilter", "delaySignal", "decimate", "opticalHybrid2x4", "pdmCoherentReceiver",
                                                           "coherentReceiver", "iqMixing", "photodiode", "balancedPD", "pdmCoherentReceiverChain",
                                                           "edc")})


@pytest.mark.parametrize("row", rs.ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_expected_output(row):
    rs.check_conditions(row)
    if row.raises:
        with pytest.raises(getattr(builtins, row.raises)):
            rs.call(row, API)
        return
    out = rs.call(row, API)
    rs.compare(row, out, "numpy")
    names = [n for n in rs.DEVICE_ARGS.get(row.kind, ()) if rs.signals(row)[n] is not None]
    if not names or rs.params(row).get("dtype") == "float32":          # (the C ABI of overlap_save; a DeviceArray filter is complex128)
        return
    sig = dict(rs.signals(row))
    for n in names:
        sig[n] = oa.to_device(sig[n])
    before = device.transfer_counts()
    outd = rs.call(row, API, sig)
    assert device.transfer_counts() == before and isinstance(outd, oa.DeviceArray), row.id
    got = outd.get()
    if row.id == "bpd-1d-n3000":
        rs.compare(row, got, "device")
    else:
        assert got.shape == out.shape and got.tobytes() == out.tobytes(), row.id
    for n in names:
        assert sig[n].get().tobytes() == rs.signals(row)[n].tobytes(), (row.id, n)
    if row.kind == "chain":                                              # ... and the one call is the four calls
        four = rs.call_four(row, API, sig).get()
        assert np.max(np.abs(got - four)) <= 1e-13 * np.max(np.abs(four)), row.id
