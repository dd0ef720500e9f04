"""The shapes at which the OFDM kernels can go wrong, as rows shared by tests/test_gpu_ofdm_shapes.py (every row) and
tests/test_ofdm_emu.py (EMU_ROWS: the rows small enough for the fibre emulator).  Both functions are held to the numpy restatement
(tests/ofdm_restatement.py) at the bounds of tests/ofdm_cases.py.

What the rows cover: transform lengths L = SpS Nfft that are powers of two -- 16 and 32 (one pass, no LDS exchange at 16), 256,
4096 and 8192 (512 lanes, 139 KiB of LDS) -- and lengths that are none (12, 500, 765, 1000: rocFFT); SpS 1, 2, 3, 4, 8; G = 0, 1
and Nfft (every sample stored twice); 1 and 2 frames, one fewer than, exactly and one more than a workgroup holds at that length
(256 frames at 16 points, 128 at 32, 16 at 256, 1 from 4096 on) and 257; Np = 0, 2, 3; pilots next to each other; pilots on
carriers 0 and Ns - 1 (no end segment to run on) and away from both (both run on); one data carrier; nulls over half the band;
Hermitian symmetry at Nfft = 4, the smallest that leaves a data carrier.  No row has more than 2^16 samples."""
import functools
from collections import namedtuple

import numpy as np

import ofdm_cases as oc
import ofdm_restatement as rs
from opticommpy_amd import _lib

Row = namedtuple("Row", "id Nfft SpS G hermit pilots nulls frames")
Case = namedtuple("Case", "row param kwargs symb tx rx dem H")
MAX_SAMPLES = 1 << 16


def _r(id, Nfft, SpS, G, frames, pilots=(), nulls=(), hermit=False):
    return Row(id, Nfft, SpS, G, hermit, tuple(pilots), tuple(nulls), frames)


FPW16, FPW32, FPW256 = (_lib.ofdm_frames_per_workgroup(L) for L in (16, 32, 256))

ROWS = [
    # ---- powers of two
    _r("L16_f1", 16, 1, 0, 1),
    _r("L16_f2_pilots_at_ends", 16, 1, 1, 2, pilots=[0, 15]),
    _r("L16_fpw-1", 16, 1, 0, FPW16 - 1, pilots=[3, 9, 12]),
    _r("L16_fpw", 16, 1, 1, FPW16),
    _r("L16_fpw+1", 16, 1, 16, FPW16 + 1, pilots=[7, 8]),                                       # pilots adjacent, G = Nfft
    _r("L16_one_data_carrier", 16, 1, 2, 3, pilots=[0, 15], nulls=[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]),
    _r("L16_half_band_null", 16, 1, 2, 3, pilots=[1, 6], nulls=range(8, 16)),
    _r("L32_fpw-1", 32, 1, 1, FPW32 - 1, pilots=[2, 30]),
    _r("L32_fpw", 32, 1, 0, FPW32, pilots=[5, 16, 31]),
    _r("L32_fpw+1", 32, 1, 32, FPW32 + 1),
    _r("L32_f257", 32, 1, 1, 257, pilots=[0, 13, 31]),
    _r("L32_sps2", 16, 2, 1, 3, pilots=[4, 11]),
    _r("L256_fpw-1", 256, 1, 4, FPW256 - 1, pilots=[0, 85, 170, 255], nulls=[128]),
    _r("L256_fpw", 256, 1, 0, FPW256, nulls=[128]),
    _r("L256_fpw+1", 256, 1, 1, FPW256 + 1, pilots=[200, 3, 90]),
    _r("L256_sps4", 64, 4, 64, 3, pilots=[10, 50]),
    _r("L256_sps8", 32, 8, 1, 2, pilots=[15, 16, 17]),
    _r("L256_hermit", 128, 2, 3, 3, pilots=[0, 62], hermit=True),
    _r("L4096_f1", 4096, 1, 1, 1, pilots=[0, 2048, 4095]),
    _r("L4096_f2", 4096, 1, 0, 2),
    _r("L4096_sps4_G_Nfft", 1024, 4, 1024, 2, pilots=[100, 400], nulls=range(512, 1024)),
    _r("L8192_f1", 8192, 1, 1, 1, pilots=[1, 4000, 8000]),
    _r("L8192_f2", 8192, 1, 0, 2),
    _r("L8192_sps2", 4096, 2, 1, 3, pilots=[0, 4095]),
    _r("L16_hermit_smallest", 4, 4, 1, 3, hermit=True),                                           # Ns = Ni = 1
    # ---- every other length: rocFFT
    _r("L12", 12, 1, 1, 3, pilots=[0, 11]),
    _r("L12_sps3", 4, 3, 0, 2),
    _r("L12_sps2_hermit", 6, 2, 6, 3, hermit=True),                                               # Ns = 2
    _r("L500", 250, 2, 8, 3, pilots=[0, 124, 249]),
    _r("L765_odd", 255, 3, 1, 3, nulls=[10, 100]),            # odd Nfft: the two fftshifts are one carrier apart, so no pilots
    _r("L1000", 1000, 1, 0, 2, pilots=[999, 1]),
    _r("L1000_sps4", 250, 4, 250, 3, pilots=[100, 101]),
    _r("L20_f257", 20, 1, 1, 257, pilots=[2, 17]),          # L = 20: 257 frames through the batched transform
]
EMU_ROWS = [r for r in ROWS if r.frames * r.SpS * (r.Nfft + r.G) <= 6000 and r.SpS * r.Nfft <= 1024]


@functools.lru_cache(maxsize=None)
def make(row):
    """Symbols, the restated transmit signal, a received signal (decimated, scaled by sqrt(SpS), through the fixtures' channel) and
    its restated demodulation -- computed once per row and shared."""
    kw = dict(Nfft=row.Nfft, G=row.G, hermitSymmetry=row.hermit, pilot=0.52 * (7 + 7j) / np.sqrt(42.0), SpS=row.SpS,
              pilotCarriers=list(row.pilots), nullCarriers=list(row.nulls))
    Ns, data = rs.layout(row.Nfft, row.hermit, row.pilots, row.nulls)
    rng = np.random.default_rng(sum(map(ord, row.id)))
    lv = np.arange(-7, 8, 2)
    n = row.frames * len(data)
    symb = (rng.choice(lv, n) + 1j * rng.choice(lv, n)) / np.sqrt(42.0)
    tx = rs.modulate(symb, **kw)
    rx = np.convolve(np.sqrt(row.SpS) * tx[::row.SpS], oc.CHANNEL)[:len(tx) // row.SpS]
    dem, H = rs.demodulate(rx, **kw)
    prm = oc.Param(**dict(kw, pilotCarriers=np.array(row.pilots, dtype=np.int64), nullCarriers=np.array(row.nulls, dtype=np.int64),
                          returnChannel=True))
    for a in (symb, tx, rx, dem):
        a.setflags(write=False)
    return Case(row, prm, kw, symb, tx, rx, dem, H)


def check_conditions(c):
    """The row is what its name says, and nothing passes emptily."""
    r = c.row
    assert len(c.tx) == r.frames * r.SpS * (r.Nfft + r.G) <= MAX_SAMPLES
    assert len(c.dem) == len(c.symb) >= 1 and np.max(np.abs(c.tx)) > 0 and np.max(np.abs(c.dem)) > 0
    if r.pilots:
        assert r.Nfft % 2 == 0 and np.all(np.abs(c.H) >= 0.3)
        F = r.frames
        Y = np.array([np.fft.fftshift(np.fft.fft(fr[r.G:])) / np.sqrt(r.Nfft) for fr in c.rx.reshape(F, -1)])
        if r.hermit:
            Y = Y[:, 1:1 + c.H.shape[0]]
        est = Y[:, list(r.pilots)] / c.kwargs["pilot"]
        assert np.max(np.abs(np.angle(est))) <= 1.5, r.id                # far from the cut of the angle at +-pi


def check_mod(c, got, dtype):
    if np.dtype(dtype) == np.complex128:
        d = oc.rel(got, c.tx)
        assert got.dtype == np.complex128 and d <= oc.TOL_MOD128, (c.row.id, d)
    else:
        d = oc.rel(got, c.tx.astype(np.complex64))
        assert got.dtype == np.complex64 and d <= oc.EPS32, (c.row.id, d)
    return d


def check_demod(c, got, H, dtype):
    if np.dtype(dtype) == np.complex128:
        d = oc.rel(got, c.dem)
        assert got.dtype == np.complex128 and d <= oc.TOL_DEMOD128, (c.row.id, d)
    else:
        want, _ = rs.demodulate(c.rx.astype(np.complex64), **c.kwargs)
        d = oc.rel(got, want.astype(np.complex64))
        assert got.dtype == np.complex64 and d <= oc.EPS32, (c.row.id, d)
    if c.row.pilots:
        if np.dtype(dtype) == np.complex128:
            assert H.dtype == np.complex128 and oc.rel(H, c.H) <= oc.TOL_DEMOD128, c.row.id
    else:
        assert isinstance(H, complex) and H == 0
    return d
