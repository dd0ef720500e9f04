"""symbolSync on the GPU at every shape of tests/sync_shape_cases.py against the extended-precision time-domain restatement
(tests/sync_restatement.py), at the bounds of tests/test_gpu_sync.py: the output equal, delay, swap, rot and conj equal,
corrMatrix within 1e-9 of its largest entry (run with -m gpu).  Every row's smallest decision margin is asserted >= 1e-6."""
import numpy as np
import pytest

import opticommpy_amd as oa
import sync_shape_cases as ss
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", ss.ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_restatement(row):
    ss.check_conditions(row)
    rx, tx = ss.signals(row)
    out, info = oa.symbolSync(rx, tx, row.SpS, row.mode, return_info=True)
    assert type(out) is np.ndarray
    ss.compare(row, out, info, "numpy")
    rxd, txd = oa.to_device(rx), oa.to_device(tx)
    before = device.transfer_counts()
    outd, infod = oa.symbolSync(rxd, txd, row.SpS, row.mode, return_info=True)
    assert device.transfer_counts() == before and isinstance(outd, oa.DeviceArray)
    assert outd.get().tobytes() == out.tobytes() and np.array_equal(infod.corrMatrix, info.corrMatrix), row.id
