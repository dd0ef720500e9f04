"""The shapes at which the perturbation-model kernels can go wrong, as rows shared by tests/test_gpu_nlin_shapes.py (every row) and
tests/test_nlin_emu.py (EMU_ROWS: the rows small enough for the fibre emulator).  Every row is held to the numpy restatement
(tests/nlin_restatement.py) at the bounds of tests/nlin_cases.py: 1e-9 in double, 2^-23 where the compared values are complex64.

The main kernel takes a tile of T = 256 symbols per workgroup, four consecutive outputs per lane, walks the coefficients of a pass
four at a time (2L + 1 of them: a remainder of 3 at odd L, of 1 at even L), and deals the 2L + 3 passes of a dense plan into
``nlin_split(N, npass)`` shares: at most 16 and at most one per pass, fewer as the tiles grow beyond 128.  So the rows are:
N = 1, 2, L, 2L, 2L + 1 (the window wider than the signal); N = T - 1, T, T + 1, 2T + 1; N no multiple of four; matrixOrder 1, 2,
3, 4; 6 and 7 (15 and 17 passes: either side of the 16 shares); two passes per share and five (N beyond 2^18: the line buffers
alternate inside one workgroup) at two shares and at one; matrixOrder 128 at N = 300; 'AMR' plans with m groups that are empty,
with a single kept coefficient, with every coefficient, and at N = 1.  Every row runs in both precisions."""
import functools
from collections import namedtuple

import numpy as np

import nlin_cases as nc
import nlin_restatement as rs
from opticommpy_amd import _lib
from opticommpy_amd import perturbation as pt

Row = namedtuple("Row", "id N L mode tol")
Case = namedtuple("Case", "row mats x y Ein Pin plan want want64")
T = _lib.NLIN_TILE
OUT = _lib.NLIN_OUT


def _r(id, N, L, mode="AM", tol=None):
    return Row(id, N, L, mode, tol)


ROWS = [
    _r("n1", 1, 2),
    _r("n2", 2, 2),
    _r("n_eq_L", 5, 5),
    _r("n_eq_2L", 10, 5),
    _r("n_eq_2L+1", 11, 5),
    _r("tile-1", T - 1, 3),
    _r("tile", T, 3),
    _r("tile+1", T + 1, 3),
    _r("two_tiles+1", 2 * T + 1, 10),
    _r("order1", 301, 1),
    _r("order2", 302, 2),
    _r("order4", 303, 4),
    _r("order6_15_passes", 2 * T + 3, 6),
    _r("order7_17_passes", 2 * T + 2, 7),
    _r("two_shares", 1024 * T + 3, 1),
    _r("one_share", 2048 * T + 1, 1),
    _r("order128", 300, 128),
    _r("amr_empty_groups", 2 * T + 1, 10, "AMR", -20),
    _r("amr_single", T + 1, 5, "AMR", -0.1),
    _r("amr_everything", T + 1, 3, "AMR", -400),
    _r("amr_default_order", 2 * T + 1, 25, "AMR", -20),
    _r("amr_n1", 1, 4, "AMR", -20),
]
EMU_ROWS = [r for r in ROWS if r.N * (2 * r.L + 1) ** 2 <= 25_000_000 and r.N <= 1024 * T + 3]      # what the emulator walks in seconds


@functools.lru_cache(maxsize=None)
def make(row):
    """Random symbols of unequal power, the matrices of ``calcPertCoeffMatrix`` at the row's order, the plan and the restated
    results in both precisions -- computed once per row and shared."""
    rng = np.random.default_rng(sum(map(ord, row.id)))
    x = (rng.standard_normal(row.N) + 1j * rng.standard_normal(row.N)) * 0.7
    y = (rng.standard_normal(row.N) + 1j * rng.standard_normal(row.N)) * 1.9
    _, Ci, Cx, Cs = pt.calcPertCoeffMatrix(nc.Param(matrixOrder=row.L))
    keep = off = None
    if row.mode == "AMR":
        keep, _, _, off = rs.select(Ci, Cx, Cs, row.tol)
    Ein = np.stack([x, y], axis=1)
    Pin = 2.0
    want, want64 = [], []
    for single, dst in ((False, want), (True, want64)):
        dst.extend(rs.nlin(Ci, Cx, Cs, x, y, keep, off, False, single))
        dst.append(rs.perturbation_nlin(Ein, Pin, Ci, Cx, Cs, keep, off, single))
    plan = pt._coeff_plan(Ci, Cx, Cs, row.mode, row.tol)
    for a in (x, y, Ein, Ci, Cx) + tuple(want) + tuple(want64):
        a.setflags(write=False)
    return Case(row, (Ci, Cx, Cs), x, y, Ein, Pin, plan, tuple(want), tuple(want64))


def param(c, prec):
    """The parameter object that makes perturbationNLIN build the row's matrices."""
    kw = dict(matrixOrder=c.row.L, mode=c.row.mode, Pin=c.Pin, prec=prec, Fc=193.2e12)
    if c.row.mode == "AMR":
        kw["coeffTol"] = c.row.tol
    return nc.Param(**kw)


def prepare_calc(c, prec):
    Ci, Cx, Cs = c.mats
    return pt._prepare_calc(Ci, Cx, Cs, c.x, c.y, prec, c.row.mode, c.row.tol)


def check_calc(c, got, prec):
    p64 = np.dtype(prec) == np.complex64
    want = c.want64 if p64 else c.want
    for k, v, w in zip(nc.OUTPUTS, got, want):
        v = np.asarray(v)
        assert v.dtype == (np.dtype(prec) if k[0] == "d" else np.float64) and np.all(np.isfinite(v)), (c.row.id, k)
        if np.max(np.abs(w)) == 0:                   # (a single symbol sees no neighbour: the phases of N = 1 are exactly zero)
            assert np.all(v == 0), (c.row.id, k)
            continue
        d = nc.rel(v, w)
        assert d <= (nc.EPS32 if p64 and k[0] == "d" else nc.TOL128), (c.row.id, k, d)


def check_nlin(c, got, prec):
    got = np.asarray(got)
    p64 = np.dtype(prec) == np.complex64
    want = (c.want64 if p64 else c.want)[4]
    assert got.dtype == np.complex128 and got.shape == c.Ein.shape and np.all(np.isfinite(got))
    if np.max(np.abs(want)) == 0:
        assert np.all(got == 0), c.row.id
        return
    d = nc.rel(got, want)
    assert d <= (nc.EPS32 if p64 else nc.TOL128), (c.row.id, d)
