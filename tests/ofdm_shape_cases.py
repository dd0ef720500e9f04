"""The shapes at which the OFDM kernels can go wrong, as rows shared by tests/test_gpu_ofdm_shapes.py (every row) and
tests/test_ofdm_emu.py (EMU_ROWS: the rows small enough for the fibre emulator).  Both functions are held to the numpy restatement
(tests/ofdm_restatement.py) at the bounds of tests/ofdm_cases.py.

What the rows cover: transform lengths L = SpS Nfft that are powers of two -- 16 and 32 (one pass, no LDS exchange at 16), 256,
4096 and 8192 (512 lanes, 139 KiB of LDS) -- and lengths that are none (12, 500, 765, 1000: rocFFT); SpS 1, 2, 3, 4, 8; G = 0, 1
and Nfft (every sample stored twice); 1 and 2 frames, one fewer than, exactly and one more than a workgroup holds at that length
(256 frames at 16 points, 128 at 32, 16 at 256, 1 from 4096 on) and 257; Np = 0, 2, 3; pilots next to each other; pilots on
carriers 0 and Ns - 1 (no end segment to run on) and away from both (both run on); one data carrier; nulls over half the band;
Hermitian symmetry at Nfft = 4, the smallest that leaves a data carrier.  No row of ROWS has more than 2^16 samples.

Second pass.  Every register length 16 .. 8192, as the modulator's L and as the demodulator's Nfft, with one frame more than a
workgroup holds (the idle groups of the last workgroup sit in the barriers).  Rows whose received frames are turned (``turn``,
cycled over the frames) so that every pilot estimate lies in quadrant II, in quadrant III, or alternates between the two from
frame to frame (the mean of the angles is then near 0 while the angle of the mean is near pi), and rows through a channel that
delays by one sample (``channel``), where the angle falls by 2 pi / Nfft per carrier and the line through the pilots at Nfft / 4
and 3 Nfft / 4 runs past pi on an end segment -- at 16 and 256 carriers, at a rocFFT length and with Hermitian symmetry.
BIG_ROWS holds one row of 116 600 frames, beyond 2^21 lanes in every element-wise kernel, so each grid-stride loop goes round
twice; the GPU test runs it once."""
import functools
from collections import namedtuple

import numpy as np

import ofdm_cases as oc
import ofdm_restatement as rs
from opticommpy_amd import _lib

CHANNEL = tuple(oc.CHANNEL.tolist())            # the fixtures' channel
DELAY = (0, 1, 0.2 + 0.1j)                      # one sample late: the angle falls by 2 pi / Nfft per carrier; needs G >= 2
# channel: the taps the decimated transmit signal goes through.  turn: rotations in radians of the received frames, cycled over them
Row = namedtuple("Row", "id Nfft SpS G hermit pilots nulls frames channel turn", defaults=(CHANNEL, (0.0,)))
Case = namedtuple("Case", "row param kwargs symb tx rx dem H")
MAX_SAMPLES = 1 << 16
LOOP_FRAMES = 1000                              # from here on the restatement runs with the frames as an array axis


def _r(id, Nfft, SpS, G, frames, pilots=(), nulls=(), hermit=False, channel=CHANNEL, turn=(0.0,)):
    return Row(id, Nfft, SpS, G, hermit, tuple(pilots), tuple(nulls), frames, tuple(channel), tuple(turn))


def kind(row):
    """Which quadrant row this is: "II", "III", "alternating", "delay", or None for a row with the defaults."""
    if row.channel != CHANNEL:
        return "delay"
    if row.turn == (0.0,):
        return None
    if all(t > np.pi / 2 for t in row.turn):
        return "II"
    if all(t < -np.pi / 2 for t in row.turn):
        return "III"
    return "alternating"


FPW = {L: _lib.ofdm_frames_per_workgroup(L) for L in (1 << lg for lg in range(4, 14))}
FPW16, FPW32, FPW256 = FPW[16], FPW[32], FPW[256]

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
    # ---- the register lengths the rows above leave out, each with one frame more than a workgroup holds; SpS = 1 rows count for the
    # modulator (L) and the demodulator (Nfft) alike
    _r("L64_fpw+1", 64, 1, 1, FPW[64] + 1, pilots=[5, 40, 63]),
    _r("L128_fpw+1", 128, 1, 0, FPW[128] + 1),
    _r("L512_fpw+1", 512, 1, 3, FPW[512] + 1, pilots=[0, 511]),
    _r("L1024_fpw+1", 1024, 1, 0, FPW[1024] + 1, nulls=[512]),
    _r("L2048_fpw+1", 2048, 1, 1, FPW[2048] + 1, pilots=[100, 1024, 2000]),
    _r("L64_sps4_fpw+1", 16, 4, 2, FPW[64] + 1),                                                  # 65 frames of 16 carriers
    _r("L1024_sps2_fpw+1", 512, 2, 1, FPW[1024] + 1, pilots=[7, 300]),
    # ---- every pilot estimate beyond a quarter turn: quadrant II, quadrant III, alternating from frame to frame
    _r("q2_L16", 16, 1, 1, 3, pilots=[2, 13], turn=[2.3]),
    _r("q3_L16", 16, 1, 1, 3, pilots=[0, 7, 15], turn=[-2.3]),
    _r("alt_L16", 16, 1, 1, 4, pilots=[3, 12], turn=[2.3, -2.3]),
    _r("q2_L256", 256, 1, 4, 3, pilots=[0, 85, 170, 255], nulls=[128], turn=[2.25, 2.3, 2.35]),
    _r("q3_L256_sps2", 128, 2, 2, FPW[256] + 1, pilots=[20, 100], turn=[-2.3]),
    _r("alt_L256", 256, 1, 1, 6, pilots=[200, 3, 90], turn=[2.2, -2.4]),
    _r("q2_L20", 20, 1, 1, 3, pilots=[2, 17], turn=[2.3]),
    _r("q3_L500", 250, 2, 8, 3, pilots=[0, 124, 249], turn=[-2.3]),
    _r("alt_L12", 12, 1, 1, 4, pilots=[0, 11], turn=[-2.3, 2.3]),
    _r("q3_L256_hermit", 128, 2, 3, 3, pilots=[0, 62], hermit=True, turn=[-2.3]),
    _r("alt_L64_hermit", 64, 1, 2, 4, pilots=[5, 25], hermit=True, turn=[2.3, -2.3]),
    # ---- one sample of delay, pilots near Nfft / 4 and 3 Nfft / 4, and a turn: the line through the mean angles passes pi on the
    # end segment below the first pilot
    _r("delay_L16", 16, 1, 2, 3, pilots=[4, 12], channel=DELAY, turn=[0.5]),
    _r("delay_L256", 256, 1, 2, 3, pilots=[64, 192], channel=DELAY, turn=[0.5]),
    _r("delay_L20", 20, 1, 2, 3, pilots=[5, 15], channel=DELAY, turn=[0.5]),
    _r("delay_L128_hermit", 128, 1, 4, 3, pilots=[31, 47], hermit=True, channel=DELAY, turn=[0.5]),           # carriers of one sign only
]
# every grid-stride loop goes round twice: F Nfft and F Ni both exceed the 8192 x 256 = 2^21 lanes of a launch, and k_chan adds 116 600
# frames.  Kept out of ROWS: the GPU test runs it once, in complex128
BIG_ROWS = [_r("L20_f116600", 20, 1, 1, 116600, pilots=[2, 17])]
EMU_ROWS = [r for r in ROWS if r.frames * r.SpS * (r.Nfft + r.G) <= 6000 and r.SpS * r.Nfft <= 1024]


@functools.lru_cache(maxsize=None)
def make(row):
    """Symbols, the restated transmit signal, a received signal (decimated, scaled by sqrt(SpS), through the row's channel, every
    frame turned by the row's angle) and its restated demodulation -- computed once per row and shared."""
    kw = dict(Nfft=row.Nfft, G=row.G, hermitSymmetry=row.hermit, pilot=0.52 * (7 + 7j) / np.sqrt(42.0), SpS=row.SpS,
              pilotCarriers=list(row.pilots), nullCarriers=list(row.nulls))
    Ns, data = rs.layout(row.Nfft, row.hermit, row.pilots, row.nulls)
    rng = np.random.default_rng(sum(map(ord, row.id)))
    lv = np.arange(-7, 8, 2)
    n = row.frames * len(data)
    symb = (rng.choice(lv, n) + 1j * rng.choice(lv, n)) / np.sqrt(42.0)
    loops = row.frames < LOOP_FRAMES
    tx = (rs.modulate if loops else rs.modulate_frames)(symb, **kw)
    rx = np.convolve(np.sqrt(row.SpS) * tx[::row.SpS], np.array(row.channel))[:len(tx) // row.SpS]
    if row.turn != (0.0,):
        rx = (rx.reshape(row.frames, -1) * np.exp(1j * np.resize(np.array(row.turn), row.frames))[:, None]).ravel()
    dem, H = (rs.demodulate if loops else rs.demodulate_frames)(rx, **kw)
    prm = oc.Param(**dict(kw, pilotCarriers=np.array(row.pilots, dtype=np.int64), nullCarriers=np.array(row.nulls, dtype=np.int64),
                          returnChannel=True))
    for a in (symb, tx, rx, dem):
        a.setflags(write=False)
    return Case(row, prm, kw, symb, tx, rx, dem, H)


def check_conditions(c):
    """The row is what its name says, and nothing passes emptily."""
    r = c.row
    assert len(c.tx) == r.frames * r.SpS * (r.Nfft + r.G) and (len(c.tx) <= MAX_SAMPLES or r in BIG_ROWS)
    assert len(c.dem) == len(c.symb) >= 1 and np.max(np.abs(c.tx)) > 0 and np.max(np.abs(c.dem)) > 0
    if r.pilots:
        assert r.Nfft % 2 == 0 and np.all(np.abs(c.H) >= 0.3)
        F = r.frames
        Y = np.fft.fftshift(np.fft.fft(c.rx.reshape(F, -1)[:, r.G:], axis=1), axes=1) / np.sqrt(r.Nfft)
        if r.hermit:
            Y = Y[:, 1:1 + c.H.shape[0]]
        ang = np.angle(Y[:, list(r.pilots)] / c.kwargs["pilot"])         # frames x pilots
        k = kind(r)
        if k is None:
            assert np.max(np.abs(ang)) <= 1.5, r.id                      # far from the cut of the angle at +-pi
            return
        assert r.frames * r.SpS * (r.Nfft + r.G) <= 6000 and r.SpS * r.Nfft <= 1024, r.id         # small enough for EMU_ROWS
        assert np.all(np.pi - np.abs(ang) >= 0.2), r.id                  # the cut is not where a rounding decides the sign
        mean = np.sum(ang, axis=0) / F
        if k == "II":
            assert np.all((ang > np.pi / 2 + 0.1) & (ang < np.pi - 0.2)), r.id
        elif k == "III":
            assert np.all((ang < -np.pi / 2 - 0.1) & (ang > -np.pi + 0.2)), r.id
        elif k == "alternating":                                        # the mean of the angles is not the angle of the mean
            assert np.all(np.abs(ang) > np.pi / 2 + 0.1) and np.any(ang > 0) and np.any(ang < 0), r.id
            assert np.max(np.abs(mean)) < 0.5, r.id
        else:
            assert r.G >= 2 and np.max(np.abs(rs.line_through(r.pilots, mean, np.arange(c.H.shape[0])))) > np.pi + 0.1, r.id
    else:
        assert kind(r) is None, r.id


def check_mod(c, got, dtype):
    fr, pre = got.reshape(c.row.frames, -1), c.row.SpS * c.row.G
    assert fr[:, :pre].tobytes() == fr[:, fr.shape[1] - pre:].tobytes(), c.row.id       # the prefix is a copy of the frame's tail
    if np.dtype(dtype) == np.complex128:
        d = oc.rel(got, c.tx)
        assert got.dtype == np.complex128 and d <= oc.TOL_MOD128, (c.row.id, d)
    else:
        d = oc.rel(got, c.tx.astype(np.complex64))
        assert got.dtype == np.complex64 and d <= oc.EPS32, (c.row.id, d)
    return d


@functools.lru_cache(maxsize=None)
def _dem64(row):
    """The restated demodulation of the row's signal rounded to complex64, itself rounded once; computed once per row."""
    c = make(row)
    want = rs.demodulate(c.rx.astype(np.complex64), **c.kwargs)[0].astype(np.complex64)
    want.setflags(write=False)
    return want


def check_demod(c, got, H, dtype):
    if np.dtype(dtype) == np.complex128:
        d = oc.rel(got, c.dem)
        assert got.dtype == np.complex128 and d <= oc.TOL_DEMOD128, (c.row.id, d)
    else:
        d = oc.rel(got, _dem64(c.row))
        assert got.dtype == np.complex64 and d <= oc.EPS32, (c.row.id, d)
    if c.row.pilots:
        if np.dtype(dtype) == np.complex128:
            assert H.dtype == np.complex128 and oc.rel(H, c.H) <= oc.TOL_DEMOD128, c.row.id
    else:
        assert isinstance(H, complex) and H == 0
    return d
