"""modulateOFDM and demodulateOFDM on the GPU at the smallest shapes where a kernel can go wrong (tests/ofdm_shape_cases.py),
against the numpy restatement at the bounds of tests/ofdm_cases.py (run with -m gpu)."""
import numpy as np
import pytest

import ofdm_shape_cases as sc
import opticommpy_amd as oa

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.id)
def test_shape_row_matches_the_restatement(row):
    c = sc.make(row)
    sc.check_conditions(c)
    wide = oa.modulateOFDM(c.symb, c.param, dtype=np.complex128)
    d = [sc.check_mod(c, wide, np.complex128)]
    got = oa.modulateOFDM(c.symb, c.param)
    d.append(sc.check_mod(c, got, np.complex64))
    assert wide.astype(np.complex64).tobytes() == got.tobytes()
    for dtype in (np.complex128, np.complex64):
        x = c.rx.astype(dtype)
        dem, H = oa.demodulateOFDM(x, c.param)
        d.append(sc.check_demod(c, dem, H, dtype))
        assert np.array_equal(x, c.rx.astype(dtype))
    print(row.id, d)


def test_the_rows_cover_what_they_claim():
    from opticommpy_amd import _lib
    L = {r.SpS * r.Nfft for r in sc.ROWS}
    assert {16, 32, 256, 4096, 8192, 12, 500, 765, 1000} <= L
    assert {r.SpS for r in sc.ROWS} >= {1, 2, 3, 4, 8} and {len(r.pilots) for r in sc.ROWS} >= {0, 2, 3}
    assert any(r.G == 0 for r in sc.ROWS) and any(r.G == 1 for r in sc.ROWS) and any(r.G == r.Nfft for r in sc.ROWS)
    for n in (16, 32, 256):
        fpw = _lib.ofdm_frames_per_workgroup(n)
        assert {fpw - 1, fpw, fpw + 1} <= {r.frames for r in sc.ROWS if r.SpS == 1 and r.Nfft == n}
    assert {1, 2} <= {r.frames for r in sc.ROWS if r.Nfft == 4096 and r.SpS == 1}
    assert {1, 2} <= {r.frames for r in sc.ROWS if r.Nfft == 8192} and any(r.frames == 257 for r in sc.ROWS)
    assert all(r.frames * r.SpS * (r.Nfft + r.G) <= sc.MAX_SAMPLES for r in sc.ROWS)
