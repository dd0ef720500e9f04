"""Every row of tests/enc_shape_cases.py on the GPU (run with -m gpu): the sizes around the codeword tile, the rows per workgroup
and the spans of the scan, one and two parity blocks, a generator matrix without a systematic part, empty rows and a run of ones
whose carry crosses every boundary; the mapper at one symbol, around a wave and past several workgroups, M = 2 and 1024, int8 and
uint8.  Held to tests/enc_restatement.py with ``np.array_equal``, from numpy and from DeviceArrays, in both orientations."""
import numpy as np
import pytest

import enc_shape_cases as es
import opticommpy_amd as oa

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", es.ENC_ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_restatement(row):
    prm, bits, want = es.make(row)
    es.check_conditions(row, prm, bits, want)
    for transposed in (False, True):
        x = np.ascontiguousarray(bits.T if transposed else bits)
        got = oa.encodeLDPC(x, prm, transposed=transposed)
        got_d = oa.encodeLDPC(oa.to_device(x.astype(np.int8)), prm, transposed=transposed)
        assert type(got) is np.ndarray and type(got_d) is oa.DeviceArray and got.dtype == np.uint8 and got_d.dtype == np.uint8
        assert got.shape == (want.T.shape if transposed else want.shape) and got_d.shape == got.shape
        assert np.array_equal(got.T if transposed else got, want), (row.id, transposed)
        assert got_d.get().tobytes() == got.tobytes(), (row.id, transposed)


@pytest.mark.parametrize("row", es.MOD_ROWS, ids=lambda r: r.id)
def test_mapper_shape_row_matches_the_restatement(row):
    bits, want = es.mod_make(row)
    got = oa.modulateGray(bits, row.M, row.constType)
    got_d = oa.modulateGray(oa.to_device(bits), row.M, row.constType)
    assert got.shape == (row.nsymb,) and got.dtype == np.complex128 and np.array_equal(got, want)
    assert type(got_d) is oa.DeviceArray and got_d.get().tobytes() == want.tobytes()
