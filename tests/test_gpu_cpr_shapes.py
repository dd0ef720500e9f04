"""Carrier phase recovery on the GPU against the extended-precision restatement (tests/cpr_restatement.py) at the shapes no
recorded fixture has (run with -m gpu): the unwrap's scan at every edge of its lanes and blocks with jumps of exactly pi, more
than one block sum per lane of the offsets kernel (n > 262 144), the grid-stride loops of the apply and scale kernels, every
segment length of the search's prefix sums (half windows 0 ... 1023, signals shorter than the window), every chunking of the
test phases (B = 1 ... 1024, a partial last chunk in both searches), 1, 2, 3 and 7 modes, and the frequency offset estimation
at odd, prime and even lengths with three modes in one batched transform.

The rows and their conditions are in tests/cpr_shape_cases.py; tests/test_cpr_restatement.py holds the restatement to the
reference's fixtures and runs the same rows through the emulator of the kernel bodies.

Bounds (tests/cpr_cases.py): raw test phases bit-equal to the restatement's wherever its margin is >= 1e-9 (a crafted row:
everywhere, and equal to the crafted sequence); unwrapped phases within PHASE_ABS = 1e-9 rad of the extended-precision unwrap of
the device's own raw phases; sigOut and the frequency-compensated signal within REL = 1e-9, rel-L2 and per element; fo equal to
numpy's grid value.  Every row runs through numpy arguments and through DeviceArrays, which must agree bit for bit; inputs are
never written and a DeviceArray call moves nothing across the bus."""
import numpy as np
import pytest

import cpr_cases as cc
import cpr_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def call(row, x, xb=None):
    """The row through the package: a dict of what sc.compare judges.  xb: the input of the search of a cprfoe row (the
    restatement's compensated and normalised signal), for the raw phases that cpr itself does not return.  Those are then
    the search's decisions on the restatement's signal, not on the device's own, which differs from it by rounding: sound
    while every symbol near a tie is decided alike on both.  A symbol whose margin lies between the two signals' difference
    (about 1e-12) and 1e-9 could be decided differently and make a correct kernel miss the phase bound; it cannot hide a
    wrong one, since phases and sigOut are still judged against the unwrap of decisions a correct search would take."""
    table = sc.table(row)
    if row.kind == "bps":
        return dict(raw=oa.bps(x, row.Nh, table, row.B))
    got = {}
    if row.kind in ("foe", "cprfoe"):
        got["sig_foe"], got["fo"] = oa.fourthPowerFOE(x, row.Fs, row.P)
        if row.kind == "foe":
            return got
    Ts = 1 / row.Fs
    assert 1 / Ts == row.Fs
    prm = cc.Param(M=row.M, constType="qam", N=2 * row.Nh + row.seed % 2, B=row.B, Ts=Ts, runFOE=row.kind == "cprfoe", returnPhases=True)
    got["sig"], got["phase"] = oa.cpr(x, prm)
    got["raw"] = oa.bpsGPU(x if xb is None else xb, row.Nh, table, row.B)
    return got


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.id)
def test_row_matches_the_restatement(row):
    sc.check_conditions(row)
    x0 = sc.signal(row)
    xb0 = None
    if row.kind == "cprfoe":
        xb0 = np.ascontiguousarray(sc.prepared(row)["xb"].reshape(x0.shape))

    x, xb = x0.copy(), None if xb0 is None else xb0.copy()
    a = call(row, x, xb)
    assert all(type(v) is np.ndarray for v in a.values())
    assert np.array_equal(x, x0) and (xb is None or np.array_equal(xb, xb0))
    sc.compare(row, a, "numpy")

    xd, xbd = oa.to_device(x0), None if xb0 is None else oa.to_device(xb0)
    assert xd.dtype == x0.dtype and xd.shape == x0.shape
    before = device.transfer_counts()
    b = call(row, xd, xbd)
    assert device.transfer_counts() == before
    for k, v in b.items():
        assert type(v) is (np.ndarray if k == "fo" else oa.DeviceArray), (row.id, k, type(v))
        assert np.array_equal(host(v), a[k]), (row.id, k)                      # numpy and device calls: the same bits
    assert np.array_equal(xd.get(), x0) and (xbd is None or np.array_equal(xbd.get(), xb0))


def test_a_small_call_after_a_large_one_on_the_cached_buffers():
    """The work buffers only grow and the FFT plans are kept per length: a small cpr and a small fourthPowerFOE, then the
    525 315-symbol row and the 263 169 x 2 row with its transform, then the small calls again give the same bits, and those
    are the restatement's."""
    small, tone = sc.BY_ID["scan-M4-257x1-Nh0-B8"], sc.BY_ID["foe-M4-257x3-Nh0-B1-P4"]
    first = call(small, sc.signal(small)), call(tone, sc.signal(tone))
    for big in (sc.BY_ID["long-M4-525315x1-Nh0-B8"], sc.BY_ID["foe-M4-263169x2-Nh2-B8-P4"]):
        xb = sc.prepared(big)["xb"].reshape(sc.signal(big).shape) if big.kind == "cprfoe" else None
        sc.compare(big, call(big, sc.signal(big), xb), "between")
    again = call(small, sc.signal(small)), call(tone, sc.signal(tone))
    for f, g in zip(first, again):
        for k in f:
            assert np.array_equal(f[k], g[k]), k
    sc.compare(small, first[0], "first")
    sc.compare(tone, first[1], "first")
