"""The case table of tests/test_gpu_cpr_shapes.py, shared with tests/test_cpr_restatement.py (which runs every row it can
through the g++ emulator): synthetic signals with literal seeds at the lengths, mode counts, windows and numbers of test phases at
which the launch code of opticommpy_amd/csrc/engine_cpr.hip takes another path, judged against tests/cpr_restatement.py.

Two kinds of input.

Crafted decisions.  With half window 0 every symbol decides alone, so x[k] = table[s_k] exp(-1j testph[b_k]) plus noise of 1e-4
makes the raw phase sequence known exactly: testph[b_k] (checked for QPSK and 16-QAM up to B = 1024: smallest margin >= 7).  The
index walks in steps drawn from {0, +-1, 3, +-B/2, B/2 +- 1}, which gives jumps of 4 phi of exactly pi (0 <-> B/2 is exact for a
power of two B; other pairs are an ulp either side), the jumps every recorded fixture excludes.  Exact jumps 0 <-> B/2 are also
placed at the edges of the unwrap's scan: elements 0 and 3 of a lane's four, lanes 63/64, the blocks' borders 1023/1024 and
2047/2048 (placed_jumps; check_conditions asserts each of them).  Every mode has its own sequence, so a transposed index fails.
A single symbol of a larger table is ambiguous between neighbouring test phases once they are fine enough: `corners` rows draw
s_k from the points of largest modulus only.

Exact ties.  An all-zero signal is the same point under every rotation, so every test phase gives the same minimum distances,
the same prefix sums and the same window sums, bit for bit: all B candidates tie at every symbol and the lowest index, test
phase 0, is the answer (np.argmin's rule).  With B = 17 and 33 the tie runs across the chunks of the search.  This is the only
input that tells a strict running minimum from a non-strict one; the noisy and crafted rows hold no exact tie.

Noisy walks.  cpr_cases.noisy_qam16 for every window case with Nh > 0; QPSK tones with a frequency offset per mode for the FOE.

Conditions a row must meet by the restatement alone (check_conditions): crafted rows a smallest margin >= 1e-9, no symbol left
out and the crafted index found; noisy rows at most 1e-4 of the symbols below a margin of 1e-9; scan and long rows at least 10
jumps of exactly pi and a span beyond 4 pi; long rows more than 256 scan blocks and more than 262 144 elements; FOE rows a
spectral margin >= 1e-6 and fo != 0.  The scan rows with n <= 5 cannot hold 10 jumps or span 4 pi ((n - 1) jumps of at most pi):
they assert that their first jump is exactly pi in every mode instead; the scan rows with B = 64 also hold jumps an ulp either
side of pi (NEAR_PI_MIN of them from 256 symbols on), which B = 8 cannot.  Zero rows: every margin exactly 0."""
import collections
import functools

import numpy as np

import cpr_cases as cc
import cpr_restatement as cr
from opticommpy_amd import cpr as ocpr

Row = collections.namedtuple("Row", "id group kind gen n modes M Nh B dtype seed P Fs emu")
# kind: cpr (cpr without FOE, and bps) | bps (bps with a scattered table) | foe (fourthPowerFOE) | cprfoe (cpr with runFOE)
# gen: crafted | corners | segments | noisy | scattered | zeros | tone;  modes = 0: a 1-D signal

SCAN_BLOCK, MAX_GRID = 1024, 262144         # kScanBlock; kMaxBlocks * kBlock of engine_cpr.hip
LEFT_OUT = 1e-4
LONG_SPAN = 9e4                             # [rad] of 4 phi: the condition under which the blocked sums were measured
FOE_MARGIN = 1e-6
NOISE = 1e-4
FS = 2.0 ** 35                              # a sampling rate that cpr's Fs = 1 / Ts returns exactly (1 / (1 / 32e9) != 32e9)
PLACED = (4, 7, 8, 11, 255, 256, 1023, 1024, 2047, 2048)
CRAFTED = ("crafted", "corners")            # the gens whose raw phase sequence is known exactly
NEAR_PI_MIN = 10                            # jumps within an ulp of pi, not exact, that a scan row with B = 64 and n >= 256 holds


def _row(group, kind, gen, n, modes, M, Nh, B, seed, dtype="complex128", P=4, Fs=1.0, emu=True, tag=""):
    shape = f"{n}" if modes == 0 else f"{n}x{modes}"
    parts = [group, f"M{M}", shape, f"Nh{Nh}", f"B{B}"] + ([f"P{P}"] if kind in ("foe", "cprfoe") else []) + \
        ([dtype] if dtype != "complex128" else []) + ([tag] if tag else [])
    return Row("-".join(parts), group, kind, gen, n, modes, M, Nh, B, dtype, seed, P, Fs, emu)


def _rows():
    rows = []
    # scan: either side of a lane's four elements, of a wave's share, of one and two scan blocks; 1, 3 and 7 modes
    for i, n in enumerate((2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)):
        M, B = ((4, 8), (16, 64))[i % 2]
        rows.append(_row("scan", "cpr", "crafted", n, (1, 3, 7)[i % 3], M, 0, B, 100 + i))
    for modes in (3, 7):
        rows.append(_row("scan", "cpr", "crafted", 2049, modes, 4, 0, 8, 120 + modes))
    # long: more than one block sum per lane of k_unwrap_offsets (nblk = 258: two, lanes >= 129 idle; 514: three), and more
    # elements than one pass of the grid-stride kernels
    rows.append(_row("long", "cpr", "crafted", 263169, 2, 4, 0, 8, 131))
    rows.append(_row("long", "cpr", "crafted", 525315, 1, 4, 0, 8, 132))
    rows.append(_row("long", "cpr", "segments", 263169, 1, 4, 2, 8, 133))
    # window: W = 256 + 2 Nh in 16 segments of ceil(W / 16): every residue of W mod 16 that exists, trailing segments empty
    # (Nh = 4, 8: W = 264, 272 ...), the longest window; n below, at and above a tile, and two tiles and one symbol
    for Nh in (0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 127, 128, 511, 1023):
        for n in (255, 256, 257, 513):
            rows.append(_row("window", "cpr", "noisy", n, 2 if n == 257 else 1, 16, Nh, 32, 200 + Nh))
    # ... and n < Nh: both ends of every window in the zero padding
    for n, Nh in ((5, 16), (100, 127), (300, 511), (2, 1023)):
        rows.append(_row("window", "cpr", "noisy", n, 1, 16, Nh, 32, 300 + Nh, tag="short"))
    # phases: one chunk, a partial last chunk, one phase beyond a chunk, 64 chunks
    for B in (1, 2, 15, 16, 17, 31, 33, 1024):
        rows.append(_row("phases", "cpr", "crafted", 301, 1, 4, 0, B, 400 + B))
    for B in (17, 33):
        rows.append(_row("phases", "bps", "scattered", 300, 2, 64, 3, B, 450 + B))
    # ... and an exact tie between all test phases at every symbol, across the chunks, in both searches
    for B in (17, 33):
        rows.append(_row("phases", "bps", "zeros", 300, 2, 4, 3, B, 470 + B, tag="tie"))
        rows.append(_row("phases", "bps", "zeros", 300, 2, 64, 3, B, 480 + B, tag="tie"))
    # foe: odd, prime and even lengths; negative, positive and near-the-edge offsets in one batched transform
    for n in (257, 4099, 6000):
        for P in (1, 2, 4, 16):
            rows.append(_row("foe", "foe", "tone", n, 3, 4, 0, 1, 500 + P, P=P, Fs=FS if P == 4 else 1.0))
    rows.append(_row("foe", "foe", "tone", 4099, 3, 4, 0, 1, 520, dtype="complex64", P=4, Fs=FS))
    rows.append(_row("foe", "cprfoe", "tone", 4099, 3, 4, 8, 32, 521, P=4, Fs=FS))
    rows.append(_row("foe", "cprfoe", "tone", 263169, 2, 4, 2, 8, 522, P=4, Fs=FS, emu=False))      # (the emulator's DFT is O(n^2))
    # types
    for dtype in ("complex64", "complex128"):
        for modes in (0, 2):
            rows.append(_row("types", "cpr", "crafted", 1300, modes, 4, 0, 8, 600, dtype=dtype))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
EMU_ROWS = [r for r in ROWS if r.emu]


def table(row):
    """The constellation of a row as the library receives it."""
    if row.M == 64:                          # the scattered, non-separable table
        rng = np.random.default_rng(row.seed + 1000)
        return rng.normal(size=row.M) + 1j * rng.normal(size=row.M)
    return ocpr._table(row.M, "qam", 0)


def crafted_index(row):
    """(n, modes) index sequence of a crafted row: a walk in the steps named above, exact jumps 0 <-> B/2 placed on top."""
    rng = np.random.default_rng(row.seed)
    n, modes, B = row.n, max(row.modes, 1), row.B
    h = B // 2
    steps = np.array([0, 1, -1, 3, h, -h, h + 1, h - 1])
    # the long rows drift slowly, so that 4 phi spans no more than LONG_SPAN
    prob = [0.43, 0.1, 0.1, 0.05, 0.08, 0.08, 0.08, 0.08] if row.group == "long" else [0.2, 0.1, 0.1, 0.1, 0.125, 0.125, 0.125, 0.125]
    b = np.cumsum(rng.choice(steps, p=prob, size=(n, modes)), axis=0) % B
    for m in range(modes):
        for k in placed_jumps(row):
            b[k - 1, m], b[k, m] = ((0, h), (h, 0))[(k + m) % 2]
    return b


def placed_jumps(row):
    """The k at which crafted_index places a jump b[k - 1] <-> b[k] of 0 <-> B/2 in every mode."""
    if row.B < 2 or row.B % 2:
        return ()
    return tuple(k for k in ((1, 2) if row.n <= 5 else PLACED + (row.n - 1,)) if 1 <= k < row.n)


@functools.lru_cache(maxsize=None)
def _build(row):
    rng = np.random.default_rng(row.seed + 5000)
    n, modes = row.n, max(row.modes, 1)

    def noise(scale):
        return scale * (rng.normal(size=(n, modes)) + 1j * rng.normal(size=(n, modes)))

    if row.gen in CRAFTED:
        tab = table(row).astype(np.complex128)
        if row.gen == "corners":
            tab = tab[np.abs(tab) >= np.max(np.abs(tab)) * (1 - 1e-12)]
        x = tab[rng.integers(0, len(tab), size=(n, modes))] * np.exp(-1j * cr.phase_grid(row.B)[crafted_index(row)]) + noise(NOISE)
    elif row.gen == "segments":
        # the same walk, one step per 20 symbols, under a window of 2 Nh + 1 = 5
        tab = table(row).astype(np.complex128)
        seg = crafted_index(row._replace(n=-(-n // 20)))
        x = tab[rng.integers(0, row.M, size=(n, modes))] * np.exp(-1j * cr.phase_grid(row.B)[np.repeat(seg, 20, axis=0)[:n]]) + noise(0.01)
    elif row.gen == "noisy":
        x, _ = cc.noisy_qam16(n, modes, 20, 0.02, seed=row.seed)
    elif row.gen == "zeros":
        x = np.zeros((n, modes), dtype=np.complex128)
    elif row.gen == "scattered":
        x = table(row)[rng.integers(0, row.M, size=(n, modes))] * np.exp(-0.2j) + noise(1e-3)
    else:
        # unit-power P-PSK with a frequency offset per mode: 0.2 of a bin off the grid, at about -0.31 n, +0.12 n and two bins
        # inside the positive edge of the range +-Fs / (2 P); the longer cpr rows add a Wiener walk for the search to follow
        bins = np.array([-int(0.31 * n), int(0.12 * n), (n - 1) // 2 - 2])[:modes] + 0.2
        k = np.arange(n)[:, None]
        walk = np.cumsum(rng.normal(size=(n, modes)) * 0.003, axis=0) if row.kind == "cprfoe" else 0.0
        angle = 2 * np.pi * (bins[None, :] / row.P) * k / n + 2 * np.pi * rng.integers(0, row.P, size=(n, modes)) / row.P + np.pi / row.P
        x = np.exp(1j * (angle + walk)) + noise(0.01)
    if row.modes == 0:
        x = x[:, 0]
    x = np.ascontiguousarray(x, dtype=row.dtype)
    x.setflags(write=False)
    return x


def signal(row):
    """The input of a row; read-only, built once per process."""
    return _build(row)


@functools.lru_cache(maxsize=None)
def prepared(row):
    """The restatement's search (and frequency offset compensation) for a row, computed once per process."""
    if row.kind == "foe":
        return dict(zip(("sig_foe", "fo", "foe_margin"), cr.foe(signal(row), row.Fs, row.P)))
    return cr.prepare(signal(row), table(row), row.Nh, row.B, row.kind == "cprfoe", row.P, row.Fs)


@functools.lru_cache(maxsize=None)
def expected(row):
    """... and the rest of the chain on the restatement's own decisions."""
    return prepared(row) if row.kind == "foe" else cr.finish(prepared(row))


def check_conditions(row):
    """The row cannot make a test pass emptily: every condition holds for the restatement alone."""
    if row.gen == "zeros":
        pre = prepared(row)
        assert not np.any(signal(row)) and np.all(pre["margin"] == 0) and not np.any(pre["index"]), row.id
        assert row.B > 16 and row.B % 16, row.id                                # more than one chunk, the last one partial
        return
    want = expected(row)
    if row.kind in ("foe", "cprfoe"):
        assert np.all(want["foe_margin"] >= FOE_MARGIN) and np.all(want["fo"] != 0), (row.id, want["foe_margin"], want["fo"])
        assert len(set(np.sign(want["fo"]))) == 2, (row.id, want["fo"])
        if row.modes >= 3:                     # the third offset lies at the edge of the range +-Fs / (2 P)
            assert np.max(np.abs(want["fo"])) > 0.49 * row.Fs / row.P * (1 - 8 / row.n), (row.id, want["fo"])
        if row.kind == "foe":
            return
    if row.gen in CRAFTED + ("segments",):
        assert want["min_margin"] >= cr.MARGIN and want["left_out"] == 0, (row.id, want["min_margin"], want["left_out"])
    if row.gen in CRAFTED:
        assert np.array_equal(want["index"], crafted_index(row)), row.id
        p4 = 4.0 * want["raw"]
        for k in placed_jumps(row):
            assert np.all(np.abs(p4[k] - p4[k - 1]) == np.pi), (row.id, "no exact jump at", k)
    assert want["left_out"] <= LEFT_OUT, (row.id, want["left_out"])
    if row.group in ("scan", "long"):
        if row.n <= 5:
            raw = want["raw"]
            assert np.all(np.abs(4.0 * raw[1] - 4.0 * raw[0]) == np.pi), row.id
        else:
            assert want["exact_pi"] >= 10 and want["span"] > 4 * np.pi, (row.id, want["exact_pi"], want["span"])
        if row.group == "scan" and row.B == 64 and row.n >= 256:
            assert want["near_pi"] >= NEAR_PI_MIN, (row.id, want["near_pi"])
    if row.group == "long":
        assert -(-row.n // SCAN_BLOCK) > 256 and row.n * max(row.modes, 1) > MAX_GRID, row.id
        assert want["span"] <= LONG_SPAN, (row.id, want["span"])


def signal_errors(got, want):
    """(rel-L2, largest element error / max |want|) in extended precision."""
    got, want = cr.as_2d(got).astype(np.clongdouble), cr.as_2d(want)
    d = np.abs(got - want)
    return float(np.sqrt(np.sum(d * d) / np.sum(np.abs(want) ** 2))), float(np.max(d) / np.max(np.abs(want)))


def compare(row, got, label=""):
    """got (a dict: raw, phase, sig for cpr rows; raw for bps rows; sig_foe, fo for FOE rows) against the restatement at the
    bounds of cpr_cases: raw phases bit-equal wherever the restatement's margin is >= 1e-9 (everywhere for a crafted row; a
    zero row: test phase 0 at every symbol, the lowest index of the exact tie),
    unwrapped phases within PHASE_ABS of the extended-precision unwrap of got's own raw phases, signals within REL (rel-L2 and
    per element), fo equal to numpy's grid value.  Prints and returns the row's errors."""
    pre = prepared(row)
    x = signal(row)
    errs = {}
    for k, v in got.items():
        if k != "fo":
            assert v.shape == x.shape, (label, row.id, k, v.shape)
    if row.kind in ("foe", "cprfoe"):
        assert isinstance(got["fo"], np.ndarray) and got["fo"].dtype == np.float64 and got["fo"].shape == pre["fo"].shape
        assert np.array_equal(got["fo"], pre["fo"]), (label, row.id, got["fo"], pre["fo"])
        if "sig_foe" in got:
            assert got["sig_foe"].dtype == np.complex128
            errs["foe_l2"], errs["foe_max"] = signal_errors(got["sig_foe"], pre["sig_foe"])
    if row.kind != "foe":
        raw = cr.as_2d(got["raw"])
        assert raw.dtype == np.float64
        sure = pre["margin"] >= cr.MARGIN
        ref = cr.phase_grid(row.B)[pre["index"]]
        if row.gen == "zeros":
            assert not np.any(sure) and not np.any(ref)
            wrong = np.count_nonzero(raw != 0.0)
            assert wrong == 0, (label, row.id, "an exact tie did not go to test phase 0 at", wrong, "of", raw.size)
        if row.gen in CRAFTED:
            assert np.all(sure) and np.array_equal(raw, cr.phase_grid(row.B)[crafted_index(row)]), (label, row.id)
        wrong = np.count_nonzero(raw[sure] != ref[sure])
        assert wrong == 0, (label, row.id, "raw phases differ at", wrong, "of", raw.size)
    if row.kind in ("cpr", "cprfoe"):
        want = cr.finish(pre, raw)
        assert got["phase"].dtype == np.float64 and got["sig"].dtype == np.complex128
        errs["phase"] = float(np.max(np.abs(cr.as_2d(got["phase"]).astype(cr.LD) - want["phase"])))
        errs["sig_l2"], errs["sig_max"] = signal_errors(got["sig"], want["sig"])
    print(f"{label} {row.id}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs.get("phase", 0.0) <= cc.PHASE_ABS, (label, row.id, errs)
    for k in ("sig_l2", "sig_max", "foe_l2", "foe_max"):
        assert errs.get(k, 0.0) <= cc.REL, (label, row.id, k, errs)
    return errs
