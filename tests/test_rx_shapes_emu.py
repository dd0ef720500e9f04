"""The receiver front end without a GPU at every row of tests/rx_shape_cases.py marked for the emulator: the kernel bodies of
rx_kernels.h / fused_kernels.h and the host sequencing of rx_pipeline.h are the ones the GPU runs (tests/emu/emu.cpp), the
marshalling is opticommpy_amd/rx.py itself with its backend swapped.  Bounds as on the GPU (tests/test_gpu_rx_shapes.py); the
receiver rows also pin the number of kernel launches, and with it the launch plan the row is named for.  Every row's conditions
are checked, emulated or not."""
import builtins
import ctypes as C
import types

import numpy as np
import pytest

import emu_binding as eb
import opticommpy_amd as oa
import rx_shape_cases as rs
from opticommpy_amd import rx as rxmod


@pytest.fixture(autouse=True)
def emu_backend(monkeypatch):
    monkeypatch.setattr(rxmod, "_backend", eb.EmuRxBackend())


def _overlap_save(N, ncols, nfft, K, H, x):
    out = np.empty_like(x)
    assert eb.load().emu_overlap_save(N, ncols, nfft.bit_length() - 1, K, H.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p),
                                      out.ctypes.data_as(C.c_void_p)) == 0
    return out


API = types.SimpleNamespace(parameters=oa.parameters, overlap_save=_overlap_save,
                            **{f: getattr(oa, f) for f in ("firFilter", "delaySignal", "decimate", "opticalHybrid2x4", "pdmCoherentReceiver",
                                                           "coherentReceiver", "iqMixing", "photodiode", "balancedPD", "pdmCoherentReceiverChain")})


@pytest.mark.parametrize("row", rs.ROWS, ids=lambda r: r.id)
def test_row_conditions(row):
    rs.check_conditions(row)


@pytest.mark.parametrize("row", rs.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_kernels_match_the_expected_output(row):
    if row.raises:
        with pytest.raises(getattr(builtins, row.raises)):
            rs.call(row, API)
        return
    out = rs.call(row, API)
    rs.compare(row, out, "emu")
    if row.launches is not None:
        e = eb.load()
        e.emu_rx_launches.restype = C.c_long
        assert e.emu_rx_launches() == row.launches, (row.id, e.emu_rx_launches())
