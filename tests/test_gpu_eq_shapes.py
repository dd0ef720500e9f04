"""The adaptive equalizer on the GPU against the numpy restatement (tests/eq_restatement.py, pinned to the reference's fixtures by
tests/test_eq_restatement.py) on the smallest shapes at which the kernels can go wrong (run with -m gpu): every number of
coefficients per lane (nModes nTaps = 64, 68, 128, 192, 256 and below), taps 1, 2, 15, 16, 17, 64, one to four modes, 1 to 3
samples per symbol, a stage of one symbol, one and three passes over stage 0, stages that end before the signal does, a static
stage first (it sees the spike, or param.H) and between adaptive runs, and stages of C - 1, C, C + 1 and 2 C + 1 symbols, C the
staging chunk of the serial kernel.

Bounds (tests/eq_cases.py): sigOut and H within 1e-9 rel-L2 and per element against max |ref|, errSq within 1e-9 of max |ref|.
Every decision of a 'dd-lms' or 'rde' stage in the restatement has its two nearest candidates at least 1e-9 apart (asserted): the
two computations agree to about 1e-15, so none can fall the other way.

test_every_row_of_the_shape_table runs the named rows of tests/eq_shape_cases.py (tables wider than a wave, every pair of
argument types at every number of coefficients per lane, lane counts either side of 64 .. 256, chunks shorter than 64, runs of
8 .. 17 stages, the end of the signal, exact ties), each with numpy arguments and with DeviceArrays, which must agree bit for
bit; tests/test_eq_shapes_emu.py runs the same rows through the g++ emulation."""
import numpy as np
import pytest

import eq_cases as ec
import eq_restatement as er
import eq_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import _lib
from opticommpy_amd import equalization as oeq

pytestmark = pytest.mark.gpu

C = _lib.EQ_CHUNK
ALL = ["nlms", "cma", "da-rde", "rde", "dd-lms"]
signal = sc.signal


def check(x, prm, tx, label, device):
    want = er.restate(x, prm, tx)
    assert want[3] >= 1e-9, (label, want[3])
    prm.returnResults = True
    if device:
        out, H, errSq, Hiter = oa.mimoAdaptEqualizer(oa.to_device(x), prm, oa.to_device(tx))
        assert isinstance(out, oa.DeviceArray)
        out = out.get()
    else:
        out, H, errSq, Hiter = oa.mimoAdaptEqualizer(x, prm, tx)
    assert np.array_equal(Hiter[:, :, 0], H)
    for a, b, what in zip((out, H, errSq), want, ("sigOut", "H", "errSq")):
        ec.compare(a, b, f"{label} {what}")
    return out, H, errSq


@pytest.mark.parametrize("modes,taps,sps", [
    (1, 1, 1), (1, 2, 2), (1, 64, 1), (2, 15, 2), (2, 16, 3), (2, 17, 1), (2, 64, 2), (3, 15, 3), (3, 64, 2), (4, 16, 2), (4, 17, 3),
    (4, 64, 1),
])
def test_every_rule_at_every_lane_layout(modes, taps, sps):
    """Five adaptive stages, one of a single symbol, three passes over stage 0, and symbols left over behind the last stage."""
    L = [C + 3, 1, 40, 50, C + 1]
    nsym = sum(L) + 7
    x, tx = signal(nsym, modes, sps, 100 * modes + taps)
    prm = ec.Param(alg=ALL, mu=[4e-3, 2e-3, 3e-3, 2e-3, 3e-3], L=L, nTaps=taps, SpS=sps, M=16, numIter=3, prec=np.complex128)
    total = oeq.total_symbols(len(x), taps, sps)
    assert total > sum(L)
    out, H, errSq = check(x, prm, tx, f"{modes} x {taps} taps, {sps} SpS", device=(modes + taps) % 2 == 0)
    assert out.shape == (total, modes) and np.all(out[sum(L):] == 0) and np.all(errSq[:, sum(L):] == 0)
    assert np.linalg.norm(H - ec.spike(modes, taps)) > 1e-3


@pytest.mark.parametrize("numIter", [1, 3])
@pytest.mark.parametrize("count", [C - 1, C, C + 1, 2 * C + 1])
def test_stage_lengths_around_the_staging_chunk(count, numIter):
    x, tx = signal(2 * C + 1, 2, 2, 7)
    assert _lib.eq_chunk(2, 15, 2) == C
    for alg in (["nlms"], ["dd-lms"]):
        prm = ec.Param(alg=alg, mu=[3e-3], L=[count], nTaps=15, SpS=2, M=16, numIter=numIter, prec=np.complex128)
        check(x, prm, tx, f"{alg[0]}, {count} symbols, {numIter} passes", device=True)


def test_a_geometry_whose_chunk_is_shorter_than_a_wave():
    """8 samples per symbol, 64 taps, 4 modes: a chunk of 64 symbols would need 2272 input values, the buffer holds 1024."""
    c = _lib.eq_chunk(4, 64, 8)
    assert c == 25
    x, tx = signal(2 * c + 3, 4, 8, 9)
    prm = ec.Param(alg=["nlms", "cma"], mu=[3e-3, 1e-3], L=[c + 1, c], nTaps=64, SpS=8, M=16, numIter=2, prec=np.complex128)
    check(x, prm, tx, "4 x 64 taps, 8 SpS", device=True)


@pytest.mark.parametrize("given", [False, True])
def test_static_stages_first_and_between(given):
    """A static stage first filters with the spike, or with param.H; one between adaptive runs with what the run before left."""
    modes, taps, sps = 2, 15, 2
    x, tx = signal(200, modes, sps, 11)
    kw = dict(alg=["static", "nlms", "static", "rde", "static"], mu=[0.0, 5e-3, 0.0, 2e-3, 0.0], L=[30, 70, 20, 50, 25], nTaps=taps, SpS=sps,
              M=16, numIter=3, prec=np.complex128)
    H0 = None
    if given:
        rng = np.random.default_rng(12)
        H0 = ec.spike(modes, taps) + 0.05 * (rng.normal(size=(4, taps)) + 1j * rng.normal(size=(4, taps)))
        kw["H"] = H0.copy()
    out, H, errSq = check(x, ec.Param(**kw), tx, f"static stages, H given: {given}", device=given)
    if given:
        assert np.array_equal(kw["H"], H0)                                   # param.H is not written
    xp = np.concatenate((np.zeros((7, modes)), x, np.zeros((7, modes))))
    first = ec.spike(modes, taps) if H0 is None else H0
    y0 = [sum(np.sum(first[k + N * modes] * xp[0:taps, N]) for N in range(modes)) for k in range(modes)]
    assert np.allclose(out[0], y0, rtol=0, atol=1e-12)
    for a, b in ((0, 30), (100, 120), (170, 195)):
        assert np.all(errSq[:, a:b] == 0)
    assert np.all(errSq[:, 30:100] > 0) and np.all(out[195:] == 0)


def test_single_precision_inputs_are_widened():
    x, tx = signal(150, 2, 2, 13)
    x32, t32 = x.astype(np.complex64), tx.astype(np.complex64)
    prm = ec.Param(alg=["nlms", "dd-lms"], mu=[5e-3, 2e-3], L=[70, 80], nTaps=15, SpS=2, M=16, numIter=2, prec=np.complex128)
    a = check(x32, prm, t32, "complex64 arguments", device=True)
    b = check(x32.astype(np.complex128), prm, t32.astype(np.complex128), "the same values as complex128", device=False)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def test_more_adaptive_stages_than_one_launch_takes():
    """Ten adaptive stages in a row: the serial kernel takes eight per launch, the coefficients carry over."""
    x, tx = signal(150, 2, 2, 15)
    alg = (ALL * 2)[:10]
    prm = ec.Param(alg=alg, mu=[3e-3] * 10, L=[13] * 10, nTaps=15, SpS=2, M=16, numIter=2, prec=np.complex128)
    check(x, prm, tx, "ten stages", device=True)


def run_row(row, device, widen=False):
    """(sigOut, H, errSq) of one call for a row (errSq None where the row asks for no results); inputs and param.H unwritten."""
    x, prm, tx = sc.widened(row) if widen else sc.build(row)
    x0, t0, H0 = x.copy(), tx.copy(), (prm.H.copy() if hasattr(prm, "H") else None)
    dx, dt = (oa.to_device(x), oa.to_device(tx)) if device else (x, tx)
    got = oa.mimoAdaptEqualizer(dx, prm, dt)
    if prm.returnResults:
        out, H, errSq, Hiter = got
        assert np.array_equal(Hiter[:, :, 0], H) and H.dtype == np.complex128 and errSq.dtype == np.float64
    else:
        out, H, errSq = got, None, None
    if device:
        assert isinstance(out, oa.DeviceArray) and np.array_equal(dx.get(), x0) and np.array_equal(dt.get(), t0), row.id
        out = out.get()
    assert isinstance(out, np.ndarray) and out.dtype == np.complex128 and out.shape == sc.expected(row)[0].shape, row.id
    assert np.array_equal(x, x0) and np.array_equal(tx, t0) and (H0 is None or np.array_equal(prm.H, H0)), row.id
    return out, H, errSq


def same_bits(a, b, label):
    for u, v in zip(a, b):
        assert (u is None and v is None) or np.array_equal(u, v), label


@pytest.mark.parametrize("name", [r.id for r in sc.ROWS])
def test_every_row_of_the_shape_table(name):
    row = sc.BY_ID[name]
    sc.check_conditions(row)
    host, dev = run_row(row, device=False), run_row(row, device=True)
    same_bits(host, dev, f"{name}: numpy arguments and DeviceArrays")
    if "noresults" in row.opt:
        sc.compare(row, host, "gpu", only_sigout=True)
    else:
        sc.compare(row, host, "gpu")
    sc.zero_regions(row, host[0], host[2])
    same_bits(host, run_row(row, device=True), f"{name}: a second call")
    if row.xdtype != "complex128" or row.rdtype != "complex128":       # the same values widened on the host: the same bits
        same_bits(host, run_row(row, device=False, widen=True), f"{name}: widened arguments")
