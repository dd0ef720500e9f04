"""modulateOFDM and demodulateOFDM on the GPU at the smallest shapes where a kernel can go wrong (tests/ofdm_shape_cases.py),
against the numpy restatement at the bounds of tests/ofdm_cases.py (run with -m gpu)."""
import numpy as np
import pytest

import ofdm_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import _lib

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
    # complex64 symbols: the frame is single precision either way, so nothing may change
    narrow = c.symb.astype(np.complex64)
    assert oa.modulateOFDM(narrow, c.param, dtype=np.complex128).tobytes() == wide.tobytes()
    assert oa.modulateOFDM(narrow, c.param).tobytes() == got.tobytes()
    for dtype in (np.complex128, np.complex64):
        x = c.rx.astype(dtype)
        dem, H = oa.demodulateOFDM(x, c.param)
        d.append(sc.check_demod(c, dem, H, dtype))
        assert np.array_equal(x, c.rx.astype(dtype))
    # a register length: the same calls around rocFFT, at the same bounds
    if _lib.ofdm_lds_length(row.SpS * row.Nfft):
        for dtype in (np.complex128, np.complex64):
            for symb in (c.symb, narrow):
                d.append(sc.check_mod(c, oa.modulateOFDM(symb, c.param, dtype=dtype, _route="rocfft"), dtype))
    if _lib.ofdm_lds_length(row.Nfft):
        for dtype in (np.complex128, np.complex64):
            dem, H = oa.demodulateOFDM(c.rx.astype(dtype), c.param, _route="rocfft")
            d.append(sc.check_demod(c, dem, H, dtype))
    print(row.id, d)


@pytest.mark.parametrize("row", sc.BIG_ROWS, ids=lambda r: r.id)
def test_big_row_takes_every_grid_stride_loop_round_twice(row):
    c = sc.make(row)
    sc.check_conditions(c)
    d = [sc.check_mod(c, oa.modulateOFDM(c.symb, c.param, dtype=np.complex128), np.complex128)]
    dem, H = oa.demodulateOFDM(c.rx, c.param)
    d.append(sc.check_demod(c, dem, H, np.complex128))
    print(row.id, d)


def test_the_rows_cover_what_they_claim():
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
    # every register length, as the modulator's and as the demodulator's, with a partly idle last workgroup; with and without pilots
    for lg in range(4, 14):
        n, fpw = 1 << lg, _lib.ofdm_frames_per_workgroup(1 << lg)
        assert _lib.ofdm_lds_length(n)
        assert any(r.SpS * r.Nfft == n and r.frames == fpw + 1 for r in sc.ROWS), n
        assert any(r.Nfft == n and r.frames == fpw + 1 for r in sc.ROWS), n
    assert not _lib.ofdm_lds_length(8) and not _lib.ofdm_lds_length(16384)
    fresh = [r for r in sc.ROWS if r.id.endswith("fpw+1") and r.SpS * r.Nfft in (64, 128, 512, 1024, 2048)]
    assert {r.SpS * r.Nfft for r in fresh} == {64, 128, 512, 1024, 2048} and 2 * sum(bool(r.pilots) for r in fresh) >= len(fresh)
    # the quadrants: each kind at 16 and 256 carriers' worth of register kernel, at a rocFFT length, and one with Hermitian symmetry
    kinds = {k: [r for r in sc.ROWS if sc.kind(r) == k] for k in ("II", "III", "alternating", "delay")}
    for k, rows in kinds.items():
        assert rows and all(r.pilots and r in sc.EMU_ROWS for r in rows), k
        assert any(_lib.ofdm_lds_length(r.Nfft) for r in rows) and any(not _lib.ofdm_lds_length(r.Nfft) for r in rows), k
    turned = [r for rows in kinds.values() for r in rows]
    assert {16, 256} <= {r.SpS * r.Nfft for r in turned} and {16, 256} <= {r.Nfft for r in turned}
    assert any(r.hermit for r in turned) and any(r.hermit for r in kinds["delay"])
    assert all(r.G >= 2 for r in kinds["delay"])
    # the big row: more elements than the 8192 x 256 lanes of an element-wise launch, in all five grid-stride loops
    lanes = 8192 * 256
    for r in sc.BIG_ROWS:
        Ni = r.Nfft - len(r.pilots) - len(r.nulls)
        assert not r.hermit and not _lib.ofdm_lds_length(r.SpS * r.Nfft) and r.pilots           # the element-wise kernels run
        assert r.frames * r.SpS * r.Nfft > lanes and r.frames * r.Nfft > lanes and r.frames * Ni > lanes
    assert sc.BIG_ROWS and not set(sc.BIG_ROWS) & set(sc.ROWS)
