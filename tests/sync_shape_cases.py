"""The case table of tests/test_gpu_sync_shapes.py, shared with tests/test_sync_emu.py (which runs the rows marked for it through
the g++ emulator): synthetic signals with literal seeds at the sizes at which the launch code of
opticommpy_amd/csrc/engine_sync.hip takes another path, judged against tests/sync_restatement.py.

The engine's geometry: every kernel has 256 lanes (four waves of 64); the peak search strides over the n_tx + n_rx - 1 lags and
the gather over the n_tx * nModes outputs with at most 1024 workgroups, so one grid round is 262 144 elements; the preparation
gives one lane a row and strides over the rows in the same way; a complex64 sequence in 'amp' has its mean from numpy's pairwise
sum (leaves of at most 128 elements, chunks of 8192).

Inputs.  `gauss`: complex normal symbols; received mode n is transmitted mode src[n], circularly shifted, turned by a phase (in
'real' a multiple of pi/2 plus 0.1) and conjugated as the row says, repeated SpS times with the off-phase samples at 0.6, plus
noise of 0.05.  `impulse`: amplitudes near 1 with one of 10 at the first or last index of either side, so that the peak is the
first, the zero or the last lag and the delay -(n_tx - 1), n_rx - n_tx or n_rx - 1.  `sparse`: zeros but for 48 symbols, for the lengths at which
only a sparse direct correlation is affordable.  Every row must pass margin >= 1e-6 in the restatement (check_conditions)."""
import collections
import functools

import numpy as np

import sync_cases as sc
import sync_restatement as sr

Row = collections.namedtuple("Row", "id mode gen n_tx n_rx modes SpS tx_dtype rx_dtype seed quarter conj emu")
# modes = 0: 1-D input; n_rx in symbols; quarter: the rotation of every mode in quarter turns ('real'); conj: every mode conjugated

BLOCK, GRID = 256, 262144                   # kBlock; kMaxBlocks * kBlock of sync_kernels.h
OFF_PHASE, SIGMA = 0.6, 0.05


def _row(mode, gen, n_tx, n_rx, modes, seed, SpS=1, tx_dtype="complex128", rx_dtype="complex128", quarter=0, conj=0, emu=True, tag=""):
    shape = f"{n_tx}v{n_rx}" + ("" if modes == 0 else f"x{modes}")
    parts = [mode, gen, shape, f"sps{SpS}"] + [d for d in (tx_dtype, rx_dtype) if d != "complex128"] + \
        ([f"q{quarter}c{conj}"] if quarter or conj else []) + ([tag] if tag else [])
    return Row("-".join(parts), mode, gen, n_tx, n_rx, modes, SpS, tx_dtype, rx_dtype, seed, quarter, conj, emu)


def _rows():
    rows = []
    # the smallest lengths, a wave and its neighbours
    for i, n in enumerate((2, 3, 63, 64, 65)):
        rows.append(_row("amp", "gauss", n, n, 2, 100 + i, SpS=(1, 2)[i % 2]))
        rows.append(_row("real", "gauss", n, n, (0, 2)[i % 2], 110 + i, SpS=(2, 1)[i % 2]))
    # lags one below, at and one above a workgroup of the peak search; outputs around a workgroup of the gather
    for i, (n_tx, n_rx) in enumerate(((128, 128), (128, 129), (129, 129))):
        rows.append(_row("amp", "gauss", n_tx, n_rx, 0, 120 + i))
        rows.append(_row("real", "gauss", n_tx, n_rx, 2, 130 + i))
    for i, n_tx in enumerate((255, 256, 257)):
        rows.append(_row("amp", "gauss", n_tx, 64, 0, 140 + i, tag="gather"))
    # ... and around one full grid round: lags 262 143, 262 144, 262 145; more rows than one round of the preparation
    for i, (n_tx, n_rx) in enumerate(((131072, 131072), (131072, 131073), (131073, 131073))):
        rows.append(_row("real", "sparse", n_tx, n_rx, 0, 150 + i, emu=i == 1))
    rows.append(_row("amp", "sparse", 131073, 131072, 0, 160, emu=False))
    rows.append(_row("amp", "sparse", 262145, 262145, 0, 161, emu=False))
    rows.append(_row("real", "sparse", 262147, 262145, 2, 162, emu=False))
    # modes and samples per symbol
    for i, modes in enumerate((1, 2, 3, 4, 8)):
        rows.append(_row("amp", "gauss", 200, 200, modes, 170 + i, SpS=(1, 2, 3, 8, 2)[i]))
        rows.append(_row("real", "gauss", 200, 200, modes, 180 + i, SpS=(8, 3, 2, 1, 3)[i]))
    # types: float32 amplitudes below and above a leaf and a chunk of the pairwise sum; a single-precision received signal
    for i, n in enumerate((7, 100, 129, 9000)):
        rows.append(_row("amp", "gauss", n, n, (0, 2)[i % 2], 190 + i, tx_dtype="complex64"))
    rows.append(_row("amp", "gauss", 300, 300, 2, 195, SpS=2, rx_dtype="complex64"))
    rows.append(_row("amp", "gauss", 300, 300, 2, 196, tx_dtype="complex64", rx_dtype="complex64"))
    rows.append(_row("real", "gauss", 300, 300, 2, 197, SpS=2, tx_dtype="complex64", rx_dtype="complex64", quarter=1))
    # peaks at the first, the zero and the last lag: delays -(n - 1), 0, n - 1 and the roll's modulo
    for i, where in enumerate(("first", "zero", "last")):
        rows.append(_row("amp", "impulse", 100, 100, 0, 200 + i, tag=where))
        rows.append(_row("amp", "impulse", 90, 100, 2, 210 + i, tag=where))
    # each of the four rotations, with and without conjugation
    for q in range(4):
        for cj in (0, 1):
            rows.append(_row("real", "gauss", 300, 300, (0, 2)[q % 2], 220 + 2 * q + cj, quarter=q, conj=cj))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
EMU_ROWS = [r for r in ROWS if r.emu]


@functools.lru_cache(maxsize=None)
def _build(row):
    rng = np.random.default_rng(row.seed)
    cols, n_tx, n_rx, SpS = max(row.modes, 1), row.n_tx, row.n_rx, row.SpS
    if row.gen == "impulse":
        tx = (1 + 0.3 * rng.uniform(-1, 1, size=(n_tx, cols))) * np.exp(2j * np.pi * rng.uniform(size=(n_tx, cols)))
        sym = (1 + 0.3 * rng.uniform(-1, 1, size=(n_rx, cols))) * np.exp(2j * np.pi * rng.uniform(size=(n_rx, cols)))
        where = row.id.rsplit("-", 1)[1]
        tx[{"first": 0, "zero": 0, "last": n_tx - 1}[where]] *= 10
        sym[{"first": n_rx - 1, "zero": 0, "last": 0}[where]] *= 10
    else:
        if row.gen == "sparse":
            tx = np.zeros((n_tx, cols), dtype=np.complex128)
            for k in range(cols):
                at = rng.choice(n_tx, size=48, replace=False)
                tx[at, k] = (1 + rng.uniform(size=48)) * np.exp(2j * np.pi * rng.uniform(size=48))
        else:
            tx = rng.normal(size=(n_tx, cols)) + 1j * rng.normal(size=(n_tx, cols))
        src = rng.permutation(cols)
        sym = np.empty((n_rx, cols), dtype=np.complex128)
        for k in range(cols):
            s = np.resize(np.roll(tx[:, src[k]], int(rng.integers(-n_tx // 3, n_tx // 3 + 1))), n_rx)
            if row.conj:
                s = s.conj()
            phase = row.quarter * np.pi / 2 + 0.1 if row.mode == "real" else rng.uniform(0, 2 * np.pi)
            sym[:, k] = s * np.exp(1j * phase)
    gain = np.full(SpS, OFF_PHASE)
    gain[rng.integers(0, SpS)] = 1.0
    rx = (sym[:, None, :] * gain[None, :, None]).reshape(n_rx * SpS, cols)
    if row.gen != "sparse":
        rx = rx + (rng.normal(size=rx.shape) + 1j * rng.normal(size=rx.shape)) * SIGMA
    if row.modes == 0:
        rx, tx = rx[:, 0], tx[:, 0]
    rx, tx = np.ascontiguousarray(rx, dtype=row.rx_dtype), np.ascontiguousarray(tx, dtype=row.tx_dtype)
    rx.setflags(write=False)
    tx.setflags(write=False)
    return rx, tx


def signals(row):
    """(rx, tx) of a row; read-only, built once per process."""
    return _build(row)


@functools.lru_cache(maxsize=None)
def expected(row):
    """The restatement's (out, info) for a row, computed once per process."""
    rx, tx = signals(row)
    out, info = sr.symbolSync(rx, tx, row.SpS, row.mode)
    out.setflags(write=False)
    return out, info


def check_conditions(row):
    """The row cannot pass or fail by rounding, and it holds what its name says."""
    out, info = expected(row)
    assert info.margin >= sc.MARGIN, (row.id, info.margin)
    if row.gen == "impulse":
        where = row.id.rsplit("-", 1)[1]
        want = {"first": -(row.n_tx - 1), "zero": row.n_rx - row.n_tx, "last": row.n_rx - 1}[where]
        assert np.all(info.delay == want), (row.id, info.delay, want)
    if row.mode == "real" and row.gen == "gauss" and row.modes <= 2 and row.n_tx >= 63:     # (a permutation of two modes is its own inverse)
        if not row.conj:
            assert np.all(info.rot == sr.ROT[(0, 2, 1, 3)[row.quarter]]), (row.id, info.rot)
        assert np.all(info.conj == bool(row.conj)), (row.id, info.conj)
    if row.n_tx + row.n_rx - 1 > GRID:
        assert row.gen == "sparse"


def compare(row, out, info, label=""):
    want_out, want = expected(row)
    sc.compare(out, info, want_out, want, f"{label} {row.id}")
