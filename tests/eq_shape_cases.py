"""The case table of the adaptive equalizer's shape tests, shared by its two runners: tests/test_eq_shapes_emu.py (the g++
emulation of the kernel bodies, tests/emu/emu_eq.cpp) and tests/test_gpu_eq_shapes.py (the GPU).  Every row is a name, literal
parameters and a literal seed; ``build(row)`` gives ``(x, param, symbRef)`` and the rows are judged against
tests/eq_restatement.py at ``eq_cases.REL``.  Signals are table symbols repeated SpS times, scaled, lightly mixed between
neighbouring modes, with small noise (``signal``).

Groups, named after the edge of opticommpy_amd/csrc/engine_eq.hip a failure points at:

  table   'dd-lms' and 'rde' behind a short 'nlms' stage on QAM 4 .. 1024 and PSK 2 .. 1024: with more than 64 points or radii
          a lane's further candidates come from LDS (the loops over ``lane + kWave``); 1024-PSK gives 129 radii, three for lane 0
  types   x / symbRef in complex128 and complex64, every pair, at 1, 2 and 4 coefficients per lane
  lanes   nModes nTaps either side of 64, 128, 192 and 256, all five adaptive rules
  chunk   geometries whose staging chunk is 63, 62, 57, 49 and 35 symbols, and the last that fits 64; stage lengths around it
  stages  runs of 8, 9, 16 and 17 adaptive stages (a launch takes 8), static stages behind, first and in a row, numIter > 1
  ends    L left empty (the last windows reach into the trailing padding), n off SpS and off 64, n == nTaps, one-symbol tails
  ties    symbol 0 exactly between four points, between two points and between two radii: the lower index wins

Conditions a row must meet by the restatement alone (``check_conditions``): every deciding update that is not a named tie has
its two nearest candidates ('rde': its two nearest radius clusters, eq_restatement.CLUSTER) at least 1e-9 apart; the updates
whose two nearest radii lie in one cluster can move the result by no more than CONSEQUENCE in all (each by at most
mu 2 R width max|y| max|x|: a pick inside a cluster changes r2 by at most 2 R width); the named ties are exact (gap == 0) and
go to the lowest index; tables wider than a wave are decided beyond index 63 at least once; and what the row's name promises
(chunk, staged elements, class of nRadii, lengths of the adaptive runs, where the signal ends) holds."""
import collections
import functools

import numpy as np

import eq_cases as ec
import eq_restatement as er
from opticommpy_amd import _lib
from opticommpy_amd import equalization as oeq

Row = collections.namedtuple("Row", "id group modes taps sps M const alg mu L numIter nsym n seed xdtype rdtype prec shaping opt "
                                    "chunk elems radii runs")
# modes = 0: a 1-D signal and a 1-D reference;  L = (): param.L left empty;  n: samples kept of nsym * sps (None: all)
# opt: noresults | Hgiven | refextra | tie0 | tiemid | tierde | lastone | exact
# chunk, elems, radii, runs: what the row's name promises (None: nothing), asserted by check_conditions

ALL = ("nlms", "cma", "da-rde", "rde", "dd-lms")
ADAPTIVE_MU = {"nlms": 4e-3, "cma": 2e-3, "da-rde": 2e-3, "rde": 2e-3, "dd-lms": 3e-3, "static": 0.0}
GAP = 1e-9
CONSEQUENCE = 1e-10          # a tenth of eq_cases.REL
WAVE = 64                    # kWave (eq_kernels.h)
RADII_CLASSES = {"1": lambda r: r == 1, "<=64": lambda r: 1 < r <= 64, ">64": lambda r: 64 < r <= 128, ">128": lambda r: r > 128}
# exact ties between two radii (rde_ties; 16-QAM has none), one per mode.  Gray-mapped neighbours differ in one bit of their index
# and the lower index has it clear, so a butterfly that lost its index comparison still ends with the lower index in lane 0 for
# every tie between points; radii are numbered in order, and a tie (3, 4) or (67, 68) goes to the higher index there.  67 and 68
# are the second candidates of lanes 3 and 4.
RDE_TIES = {64: ((2, 3), (3, 4)), 1024: ((62, 63), (67, 68))}


@functools.lru_cache(maxsize=None)
def signal(nsym, modes, sps, seed, M=16, const="qam", shaping=0):
    """M-ary symbols at sps samples per symbol, scaled, mixed between neighbouring modes, with a little noise; and its symbols."""
    rng = np.random.default_rng(seed)
    table = oeq._tables(M, const, shaping, np.complex128)[0]
    tx = table[rng.integers(0, M, size=(nsym, modes))]
    x = np.repeat(tx, sps, axis=0) * 0.9 + 0.04 * (rng.normal(size=(nsym * sps, modes)) + 1j * rng.normal(size=(nsym * sps, modes)))
    x = x + 0.2 * np.exp(0.3j) * np.roll(x, 1, axis=1) if modes > 1 else x
    x.setflags(write=False), tx.setflags(write=False)
    return x, tx


def _row(group, name, modes, taps, sps, alg, L, nsym, seed, M=16, const="qam", mu=None, numIter=1, n=None, xdtype="complex128",
         rdtype="complex128", prec="complex128", shaping=0, opt=(), chunk=None, elems=None, radii=None, runs=None):
    mu = tuple(ADAPTIVE_MU[a] for a in alg) if mu is None else tuple(mu)
    return Row(f"{group}-{name}", group, modes, taps, sps, M, const, tuple(alg), mu, tuple(L), numIter, nsym, n, seed, xdtype, rdtype,
               prec, shaping, tuple(opt), chunk, elems, radii, runs)


def _rows():
    rows = []
    # table: (constellation, M, class of nRadii); an 'rde' stage on 64- and 128-PSK is short and slow: their radius clusters are up to
    # 3e-9 wide and most decisions fall inside one
    for const, M, radii in (("qam", 4, "1"), ("qam", 64, "<=64"), ("qam", 256, "<=64"), ("qam", 1024, ">64"), ("psk", 2, "1"),
                            ("psk", 8, "<=64"), ("psk", 64, "<=64"), ("psk", 128, "<=64"), ("psk", 1024, ">128")):
        for rule in ("dd-lms", "rde"):
            short = rule == "rde" and const == "psk" and M in (64, 128)
            L = (60, 12) if short else (60, 90)
            rows.append(_row("table", f"{const}{M}-{rule}", 2, 15, 2, ("nlms", rule), L, sum(L) + 5, 1000 + M + (rule == "rde"), M=M,
                             const=const, mu=(4e-3, 5e-4) if short else None, numIter=2, radii=radii))
    rows.append(_row("table", "qam1024-rde-prec64", 2, 15, 2, ("nlms", "rde"), (60, 90), 155, 1101, M=1024, numIter=2, prec="complex64",
                     radii=">64"))
    rows.append(_row("table", "qam1024-ddlms-prec64", 2, 15, 2, ("nlms", "dd-lms"), (60, 90), 155, 1102, M=1024, numIter=2,
                     prec="complex64", radii=">64"))
    rows.append(_row("table", "qam256-shaped-rde", 2, 15, 2, ("nlms", "rde", "dd-lms"), (60, 50, 40), 155, 1103, M=256, numIter=2,
                     mu=(4e-3, 5e-4, 1e-3), shaping=0.01, radii="<=64"))
    for rule in ("dd-lms", "rde"):
        rows.append(_row("table", f"qam1024-{rule}-4x64", 4, 64, 1, ("nlms", rule), (70, 70), 145, 1110 + (rule == "rde"), M=1024,
                         numIter=2, radii=">64"))
    rows.append(_row("table", "psk1024-rde-4x17", 4, 17, 2, ("nlms", "rde", "dd-lms"), (50, 40, 30), 125, 1120, M=1024, const="psk",
                     numIter=2, radii=">128"))
    # types
    for xdtype, rdtype in (("complex128", "complex128"), ("complex64", "complex64"), ("complex128", "complex64"),
                           ("complex64", "complex128")):
        for modes, taps, sps in ((2, 15, 2), (4, 17, 2), (4, 64, 1)):
            rows.append(_row("types", f"x{xdtype[7:]}-ref{rdtype[7:]}-{modes}x{taps}", modes, taps, sps, ("nlms", "da-rde", "dd-lms"),
                             (40, 30, 30), 100, 2000 + modes * taps, numIter=2, xdtype=xdtype, rdtype=rdtype))
    rows.append(_row("types", "x128-ref64-refextra", 2, 15, 2, ("nlms", "da-rde", "dd-lms"), (40, 30, 30), 131, 2100, numIter=2,
                     rdtype="complex64", opt=("refextra",)))
    rows.append(_row("types", "x64-ref128-1d", 0, 15, 2, ("nlms", "da-rde", "dd-lms"), (40, 30, 30), 104, 2101, numIter=2, xdtype="complex64"))
    rows.append(_row("types", "x128-ref64-1d-64taps", 0, 64, 2, ("da-rde", "nlms", "rde"), (40, 30, 30), 104, 2102, numIter=2,
                     rdtype="complex64"))
    # lanes
    for modes, taps in ((3, 21), (2, 33), (3, 43), (4, 33), (4, 49), (4, 63)):
        rows.append(_row("lanes", f"{modes * taps}-{modes}x{taps}", modes, taps, 2, ALL, (45, 1, 30, 35, 40), 156, 3000 + modes * taps,
                         numIter=3))
    # chunk: (modes, taps, sps) -> symbols per chunk, elements of the staging buffer a full chunk uses where that is the point
    for (modes, taps, sps), c, elems in (((4, 8, 4), 63, 1024), ((4, 5, 4), 63, None), ((4, 9, 4), 62, None), ((3, 5, 6), 57, 1023),
                                         ((4, 64, 3), 64, 1012), ((4, 64, 4), 49, None), ((3, 64, 8), 35, None), ((2, 64, 8), 57, None)):
        for count in (c - 1, c, c + 1, 2 * c + 1):
            for numIter in (1, 3):
                for rule in ("nlms", "dd-lms"):
                    rows.append(_row("chunk", f"{modes}x{taps}x{sps}-{count}of{c}-{numIter}pass-{rule}", modes, taps, sps, (rule,), (count,),
                                     2 * c + 1, 4000 + 100 * modes + taps + sps, mu=(3e-3,), numIter=numIter, chunk=c, elems=elems))
    # stages
    for k in (8, 9, 16, 17):
        rows.append(_row("stages", f"run{k}", 2, 15, 2, (ALL * 4)[:k], [5 + i % 4 for i in range(k)], 135, 5000 + k, numIter=2,
                         runs=(k,)))
    rows.append(_row("stages", "run8-static-run2", 2, 15, 2, (ALL * 2)[:8] + ("static", "rde", "nlms"), [9] * 8 + [11, 20, 20], 130, 5020,
                     numIter=2, runs=(8, 2)))
    rows.append(_row("stages", "one-symbol-first-3pass", 2, 15, 2, ("nlms", "dd-lms", "cma"), (1, 40, 30), 75, 5021, numIter=3, runs=(3,)))
    rows.append(_row("stages", "static-first-3pass-Hgiven", 2, 15, 2, ("static", "nlms", "rde"), (20, 50, 40), 115, 5022, numIter=3,
                     opt=("Hgiven",), runs=(2,)))
    rows.append(_row("stages", "static-static", 3, 15, 2, ("nlms", "static", "static", "cma"), (50, 10, 15, 40), 120, 5023, numIter=2,
                     runs=(1, 1)))
    rows.append(_row("stages", "all-one-symbol", 2, 15, 2, ALL * 2, [1] * 10, 14, 5024, numIter=2, runs=(10,)))
    rows.append(_row("stages", "noresults", 2, 15, 2, ("nlms", "static", "dd-lms"), (50, 20, 40), 115, 5025, numIter=2,
                     opt=("noresults",), runs=(1, 1)))
    # ends
    rows.append(_row("ends", "Lempty-odd-taps", 2, 15, 2, ("nlms",), (), 100, 6000))
    rows.append(_row("ends", "Lempty-even-taps", 2, 16, 2, ("nlms",), (), 100, 6001, n=198))
    rows.append(_row("ends", "Lempty-even-taps-ddlms", 3, 44, 1, ("dd-lms",), (), 90, 6002))
    rows.append(_row("ends", "Lempty-n-off-sps", 2, 15, 3, ("nlms",), (), 100, 6003, n=299))
    rows.append(_row("ends", "Lempty-n-off-64", 3, 15, 2, ("cma",), (), 67, 6004))
    rows.append(_row("ends", "n-is-taps-one-symbol", 2, 5, 8, ("nlms",), (), 1, 6005, n=5))
    rows.append(_row("ends", "n-is-taps", 2, 15, 2, ("nlms",), (), 8, 6006, n=15))
    rows.append(_row("ends", "n-is-taps-64", 4, 64, 2, ("dd-lms",), (), 32, 6007, n=64))
    rows.append(_row("ends", "three-stages-to-the-end", 2, 15, 2, ("nlms", "cma", "dd-lms"), (50, 30, 40), 120, 6008, numIter=2,
                     opt=("exact",)))
    rows.append(_row("ends", "last-chunk-one-symbol", 2, 15, 2, ("nlms",), (), 129, 6009, opt=("lastone",)))
    rows.append(_row("ends", "last-chunk-one-symbol-short-chunk", 3, 64, 8, ("dd-lms",), (), 71, 6010, n=560, opt=("lastone",), chunk=35))
    # ties
    for M in (16, 256, 1024):
        rows.append(_row("ties", f"four-points-qam{M}", 2, 15, 2, ("dd-lms",), (60,), 64, 7000 + M, M=M, opt=("tie0",)))
        rows.append(_row("ties", f"two-points-qam{M}", 4, 15, 2, ("dd-lms",), (60,), 64, 7001 + M, M=M, opt=("tiemid",)))
    for M in RDE_TIES:
        rows.append(_row("ties", f"two-radii-qam{M}", 2, 15, 2, ("rde",), (60,), 64, 7100 + M, M=M, opt=("tierde",)))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
GROUPS = ("table", "types", "lanes", "chunk", "stages", "ends", "ties")


@functools.lru_cache(maxsize=None)
def midpoint_pairs(M):
    """(lower index, higher index, midpoint) of every pair of horizontally neighbouring M-QAM points whose midpoint is at a
    bit-equal distance from both, in the restatement's |y - c| and in the kernel's squared distance alike."""
    table = oeq._tables(M, "qam", 0, np.complex128)[0]
    pairs = []
    for a in range(M):
        for b in range(a + 1, M):
            if table[a].imag != table[b].imag:
                continue
            y = complex((table[a].real + table[b].real) / 2, table[a].imag)
            d = np.abs(y - table)
            if np.argmin(d) == a and d[a] == d[b] and np.partition(d, 2)[2] - d[a] >= GAP and y.real - table[a].real == table[b].real - y.real:
                pairs.append((a, b, y))
    return pairs


@functools.lru_cache(maxsize=None)
def rde_ties(M):
    """(lower index, higher index, a) for every pair of neighbouring radius clusters of M-QAM with a double ``a`` between them
    that is at a bit-equal distance from the nearest radius of either and survives the kernel's sqrt(a * a).  Looked for at the
    midpoint and up to four doubles either side of it."""
    radii = oeq._tables(M, "qam", 0, np.complex128)[2]
    cl, _ = er.radius_clusters(radii)
    found = []
    for c in range(cl[-1]):
        lo, hi = int(np.flatnonzero(cl == c)[-1]), int(np.flatnonzero(cl == c + 1)[0])
        a = (radii[lo] + radii[hi]) / 2
        for cand in [a] + [f(a, k) for k in range(1, 5) for f in (_up, _down)]:
            if abs(radii[lo] - cand) == abs(radii[hi] - cand) and np.sqrt(cand * cand) == cand and np.abs(complex(cand, 0.0)) == cand:
                found.append((lo, hi, float(cand)))
                break
    return found


def _up(a, k):
    for _ in range(k):
        a = np.nextafter(a, np.inf)
    return a


def _down(a, k):
    for _ in range(k):
        a = np.nextafter(a, -np.inf)
    return a


def tie_targets(row):
    """Per mode: (value of x[0], index that must win) of a tie row."""
    modes = max(row.modes, 1)
    if "tie0" in row.opt:
        a = np.abs(oeq._tables(row.M, row.const, 0, np.complex128)[0])
        inner = np.flatnonzero(a == a.min())
        assert len(inner) == 4, row.id
        return [(0j, int(inner[0]))] * modes
    if "tiemid" in row.opt:
        pairs = midpoint_pairs(row.M)
        assert pairs, row.id
        return [(pairs[(5 * k) % len(pairs)][2], pairs[(5 * k) % len(pairs)][0]) for k in range(modes)]
    ties = {(lo, hi): a for lo, hi, a in rde_ties(row.M)}
    return [(complex(ties[RDE_TIES[row.M][k % 2]], 0.0), RDE_TIES[row.M][k % 2][0]) for k in range(modes)]


@functools.lru_cache(maxsize=None)
def _arrays(row):
    modes = max(row.modes, 1)
    x, tx = signal(row.nsym, modes, row.sps, row.seed, row.M, row.const, row.shaping)
    x = np.array(x[:row.n] if row.n else x)
    if set(row.opt) & {"tie0", "tiemid", "tierde"}:
        x[0, :] = [v for v, _ in tie_targets(row)]
    total = oeq.total_symbols(len(x), row.taps, row.sps)
    tx = np.array(tx if "refextra" in row.opt else tx[:sum(row.L) if row.L else total])
    if row.modes == 0:
        x, tx = x[:, 0], tx[:, 0]
    x, tx = np.ascontiguousarray(x, dtype=row.xdtype), np.ascontiguousarray(tx, dtype=row.rdtype)
    H = None
    if "Hgiven" in row.opt:
        rng = np.random.default_rng(row.seed + 1)
        H = ec.spike(modes, row.taps) + 0.05 * (rng.normal(size=(modes ** 2, row.taps)) + 1j * rng.normal(size=(modes ** 2, row.taps)))
        H.setflags(write=False)
    x.setflags(write=False), tx.setflags(write=False)
    return x, tx, H


def build(row, **extra):
    """(x, param, symbRef) of a row: the arrays are read-only and built once per process, the parameter object is fresh."""
    x, tx, H = _arrays(row)
    kw = dict(alg=list(row.alg), mu=list(row.mu), L=list(row.L), nTaps=row.taps, SpS=row.sps, M=row.M, constType=row.const,
              numIter=row.numIter, prec=np.dtype(row.prec).type, shapingFactor=row.shaping, returnResults="noresults" not in row.opt)
    if H is not None:
        kw["H"] = H.copy()
    kw.update(extra)
    return x, ec.Param(**kw), tx


def widened(row):
    """The same values as complex128 arguments."""
    x, prm, tx = build(row)
    return x.astype(np.complex128), prm, tx.astype(np.complex128)


@functools.lru_cache(maxsize=None)
def expected(row):
    """(sigOut, H, errSq, gap, detail) of the restatement for a row, computed once per process."""
    x, prm, tx = build(row)
    want = er.restate(x, prm, tx, detail=True)
    for a in want[:3]:
        a.setflags(write=False)
    return want


def adaptive_runs(alg):
    """Lengths of the runs of consecutive adaptive stages."""
    runs, k = [], 0
    for a in tuple(alg) + ("static",):
        if a == "static":
            runs += [k] if k else []
            k = 0
        else:
            k += 1
    return tuple(runs)


def launch_path(row):
    """(coefficients per lane, input dtype, the point loop runs, the radius loop runs) from the row's literals and the tables."""
    q = oeq._prepare(*build(row))
    p = q["params"]
    R = -(-p.nModes * p.nTaps // WAVE)
    return (4 if R == 3 else R), row.xdtype, "dd-lms" in row.alg and p.M > WAVE, "rde" in row.alg and p.nRadii > WAVE


def coverage():
    """instantiation of k_eq_serial or candidate loop -> names of the rows that reach it."""
    cov = collections.defaultdict(list)
    for row in ROWS:
        R, xdtype, points, radii = launch_path(row)
        if adaptive_runs(row.alg):
            cov[f"k_eq_serial<{R}, {'Cplx' if xdtype == 'complex128' else 'CplxF'}>"].append(row.id)
        if points:
            cov["points beyond lane + 64"].append(row.id)
        if radii:
            cov["radii beyond lane + 64"].append(row.id)
    return dict(cov)


def check_conditions(row):
    """The row cannot make a test pass emptily: every condition holds for the restatement alone."""
    x, prm, tx = build(row)
    q = oeq._prepare(x, prm, tx)
    p = q["params"]
    modes, total = p.nModes, q["total"]
    sigOut, H, errSq, gap, info = expected(row)
    dec = info["decisions"]
    assert len(row.alg) == len(row.mu) == len(q["L"]) and sum(q["L"]) <= total, row.id

    # what the name promises
    if row.radii is not None:
        nrad = len(np.unique(np.abs(oeq._tables(row.M, row.const, row.shaping, np.dtype(row.prec))[0])))
        assert p.nRadii == nrad == len(q["radii"]) and RADII_CLASSES[row.radii](nrad), (row.id, nrad)
    if row.chunk is not None:
        assert _lib.eq_chunk(modes, row.taps, row.sps) == row.chunk, (row.id, _lib.eq_chunk(modes, row.taps, row.sps))
    if row.elems is not None:
        assert ((row.chunk - 1) * row.sps + row.taps) * modes == row.elems <= _lib.EQ_STAGE_ELEMS, row.id
    if row.runs is not None:
        assert adaptive_runs(row.alg) == row.runs, (row.id, adaptive_runs(row.alg))
    if row.group == "lanes":
        assert row.id.startswith(f"lanes-{modes * row.taps}-") and (modes * row.taps) % WAVE, row.id
    if row.group == "ends":
        name = row.id
        assert ("Lempty" in name or "n-is-taps" in name or "last-chunk" in name) == (row.L == ()), name
        if row.L == ():                        # the last window ends in the trailing padding
            assert q["L"] == [total] and ("Lempty" not in name or (total - 1) * row.sps + row.taps > row.taps // 2 + p.n), name
        if "odd-taps" in name or "even-taps" in name:
            assert row.taps % 2 == ("odd-taps" in name), name
        if "off-sps" in name:
            assert p.n % row.sps, name
        if "off-64" in name:
            assert (p.n * modes) % 64, name
        if "n-is-taps" in name:
            assert p.n == row.taps and (total == 1) == ("one-symbol" in name), (name, total)
        if "exact" in row.opt:
            assert len(row.L) == 3 and sum(row.L) == total, name
        if "lastone" in row.opt:
            assert total % _lib.eq_chunk(modes, row.taps, row.sps) == 1 and total > 1, (name, total)
    if "refextra" in row.opt:
        assert len(tx) > sum(row.L), row.id
    elif q["ref"] is not None:
        assert len(tx) == sum(q["L"]), row.id
    if row.modes == 0:
        assert x.ndim == 1 and tx.ndim == 1 and sigOut.ndim == 1, row.id

    # decisions: named ties exact and to the lowest index, every other one clear
    named = np.zeros(len(dec), dtype=bool)
    if row.group == "ties":
        named = (dec["stage"] == 0) & (dec["rep"] == 0) & (dec["symbol"] == 0)
        assert np.count_nonzero(named) == modes and np.all(dec["gap"][named] == 0.0), (row.id, dec[named])
        for r in dec[named]:
            assert r["winner"] == tie_targets(row)[r["mode"]][1], (row.id, r)
    rest = dec[~named]
    assert np.all(rest["cgap"] >= GAP), (row.id, rest[rest["cgap"] < GAP])
    for s, a in enumerate(row.alg):
        if a == "dd-lms" and row.M > WAVE:
            assert np.any(dec["winner"][dec["stage"] == s] >= WAVE), row.id
        if a == "rde" and p.nRadii > WAVE:
            assert np.any(dec["winner"][dec["stage"] == s] >= (2 * WAVE if p.nRadii > 2 * WAVE else WAVE)), row.id

    # what the picks inside a radius cluster can do to the result
    xmax = float(np.max(np.abs(x)))
    moved = sum(np.count_nonzero(dec["same"] & (dec["stage"] == s)) * row.mu[s] * 2 * float(np.max(q["radii"])) * info["width"]
                * info["ymax"] * xmax for s in range(len(row.alg)))
    assert moved <= CONSEQUENCE, (row.id, moved, info["in_cluster"], info["width"])

    # the coefficients moved, and differently in every mode
    if adaptive_runs(row.alg) and total > 1:
        assert np.linalg.norm(H - q["H"]) > 1e-4, row.id
    return dict(moved=moved, in_cluster=info["in_cluster"], width=info["width"], cluster_gap=info["cluster_gap"])


def compare(row, got, label, only_sigout=False):
    """(sigOut, H, errSq) of a runner against the restatement at eq_cases.REL; returns the largest of the printed errors."""
    want = expected(row)
    worst = 0.0
    for a, b, what in list(zip(got, want, ("sigOut", "H", "errSq")))[:1 if only_sigout else 3]:
        ec.compare(a, b, f"{label} {row.id} {what}")
        worst = max(worst, ec.rel_l2(a, b), float(np.max(np.abs(np.asarray(a) - b)) / np.max(np.abs(b))))
    print(f"{label} {row.id} worst {worst:.3e}")
    return worst


def zero_regions(row, sigOut, errSq):
    """Outputs behind the last stage and errSq of static stages are exactly 0."""
    q = oeq._prepare(*build(row))
    out = np.asarray(sigOut).reshape(q["total"], -1)
    assert np.all(out[sum(q["L"]):] == 0), row.id
    if errSq is not None:
        assert np.all(errSq[:, sum(q["L"]):] == 0), row.id
        start = 0
        for a, ln in zip(q["alg"], q["L"]):
            if a == "static":
                assert np.all(errSq[:, start:start + ln] == 0), (row.id, start)
            start += ln
