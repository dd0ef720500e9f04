"""Shapes, inputs and bounds of the array layer's tests (tests/test_gpu_array.py on the GPU, tests/test_array_emu.py with g++): the
smallest shapes at which the kernels of engine_array.hip can go wrong, inputs built so that no row can pass emptily, and the derived
bounds of the multi-rounding operations against tests/array_restatement.py.

u is 2^-53 for float64 / complex128 results and 2^-24 for float32 / complex64 ones.
    complex x complex     per component 3 u (|p1| + |p2|), p1 and p2 the two products that form it (two roundings of products and
                          one of their sum or difference are 2 u (|p1| + |p2|) to first order; a single-precision result adds its own)
    complex / complex     8 u |exact| on the complex value: Smith's form has five roundings per component
    abs, abs2             4 u |exact|
    exp, angle, sqrt      no derived bound (the device math library's accuracy is not documented): 4 x numpy's own largest relative
                          distance to the restatement on the same inputs, and not less than 4 u
    sum, mean             n u64 sum|x_i| with u64 = 2^-53 whatever the type (the accumulation is double, in any order), plus one
                          rounding of the result type; var and std the same on the squared deviations
Movement and single-rounding operations are numpy's bytes (same_bits), NaNs with their sign and payload included.  The one exception
is + - x / and sqrt, which can GENERATE a NaN from operands that are none (inf - inf, 0 x inf, 0 / 0, sqrt(-1)): the sign of such a
NaN is the hardware's -- x86 makes it negative, gfx950 positive, numpy itself differs between machines there -- so for those
operations alone a NaN of numpy's may be any NaN here; every other byte is still compared."""
import numpy as np

import array_restatement as ar
from opticommpy_amd import _lib

LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025]
SPAN = _lib.ARRAY_MAX_BLOCKS * _lib.ARRAY_BLOCK              # lanes of a capped element-wise or movement grid: 2^20
RED_SPAN = _lib.ARRAY_RED_BLOCKS * _lib.ARRAY_BLOCK          # rows one walk of a capped reduction grid covers: 2^16
ARITH = [np.float32, np.float64, np.complex64, np.complex128]
MOVE = [np.uint8, np.int16, np.int32, np.float64, np.complex128]          # item sizes 1, 2, 4, 8, 16
SHAPES = [lambda n: (n,), lambda n: (n, 1), lambda n: (n, 2), lambda n: (n, 3), lambda n: (n, 5), lambda n: (n, 2, 3)]
SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.5, 1e-30, -2.5e20, np.inf, np.nan, 0.0]


def vec_width(dtype):
    return 16 // np.dtype(dtype).itemsize


def values(shape, dtype, seed, scale=1.0):
    """Standard normal values of the dtype (any of MOVE or ARITH): no two alike, so a misplaced element shows."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        return rng.integers(0, np.iinfo(dtype).max, size=shape, dtype=dtype)
    x = rng.standard_normal(shape) * scale
    if dtype.kind == "c":
        x = x + 1j * rng.standard_normal(shape) * scale
    return x.astype(dtype)


def specials(dtype, partner=False):
    """A row of NaN, +-Inf, +-0 and ordinary values; partner: the same values in another order, so that every pair meets."""
    v = np.array(SPECIALS[::-1] if partner else SPECIALS)
    v = np.roll(v, 3) if partner else v
    dtype = np.dtype(dtype)
    return (v + 1j * np.roll(v, 5)).astype(dtype) if dtype.kind == "c" else v.astype(dtype)


def same_bits(got, want, generates_nan=False):
    """Equal dtype, shape and bytes.  generates_nan: the operation can make a NaN out of operands that are none (inf - inf, 0 x inf,
    0 / 0, sqrt(-1)); only then a NaN of numpy's may be any NaN here.  An operation that carries a NaN through (movement, negation,
    conj, real, imag, astype, abs, min / max) must hand on numpy's sign and payload."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not generates_nan or got.dtype.kind not in "fc":
        return got.tobytes() == want.tobytes()
    g = got.view(ar.REAL_OF[got.dtype.name]) if got.dtype.kind == "c" else got
    w = want.view(ar.REAL_OF[want.dtype.name]) if want.dtype.kind == "c" else want
    nan = np.isnan(w)
    return bool(np.isnan(g[nan]).all()) and g[~nan].tobytes() == w[~nan].tobytes()


def u_of(dtype):
    return ar.U[np.dtype(dtype).name]


def check_product(got, a, b):
    """A complex product against the restatement: per component 3 u (|p1| + |p2|).  a and b as the kernel takes them."""
    exact = ar.binary("mul", a, b)
    tre, tim = ar.product_terms(a, b)
    u = u_of(got.dtype)
    g = ar.widen(got)
    assert np.all(np.abs(g.real - exact.real) <= 3 * u * tre), float(np.max(np.abs(g.real - exact.real) / (u * tre)))
    assert np.all(np.abs(g.imag - exact.imag) <= 3 * u * tim), float(np.max(np.abs(g.imag - exact.imag) / (u * tim)))
    assert np.all(tre + tim > 0)                                            # (no row passes with everything zero)


def check_relative(got, exact, units):
    """|got - exact| <= units u |exact| on the (complex) value; returns the largest distance in units of u |exact|."""
    u = u_of(got.dtype)
    d = np.abs(ar.widen(got) - exact)
    assert np.all(np.abs(exact) > 0) and np.all(np.isfinite(got))
    worst = float(np.max(d / (u * np.abs(exact))))
    assert np.all(d <= units * u * np.abs(exact)), worst
    return worst


def library_distance(op, x, got):
    """exp, angle, sqrt: (the device's, numpy's) largest relative distance to the restatement in units of u, and the allowance."""
    exact = ar.unary(op, x)
    with np.errstate(all="ignore"):
        ref = {"exp": np.exp, "angle": np.angle, "sqrt": np.sqrt}[op](x)
    u = u_of(got.dtype)
    ok = np.abs(exact) > 0
    dist = lambda v: float(np.max(np.abs(ar.widen(v)[ok] - exact[ok]) / (u * np.abs(exact[ok]))))     # noqa: E731
    return dist(got), dist(ref), max(4 * dist(ref), 4.0)


def angle_input(n, dtype, seed):
    """Points all round the circle that keep |im| >= 1e-6 |re| where re < 0 (near the cut the result's relative error is that of
    pi - tiny), and two explicit samples on the cut: im = +0.0 and -0.0 with re < 0, which must give +pi and -pi."""
    z = values((n,), dtype, seed)
    near = (z.real < 0) & (np.abs(z.imag) < 1e-6 * np.abs(z.real))
    z[near] = z[near] + 1j * np.abs(z[near].real)
    if n >= 2:
        z[0], z[1] = complex(-1.5, 0.0), complex(-2.5, -0.0)
    return z


def reduction_input(shape, dtype, seed):
    """Values with |x_i| in [0.1, 1]: every |x_i| >= 1e-3 max|x| and n <= 2^17, so a dropped or doubled element moves the sum by far
    more than the bound (n^2 u <= 1.9e-6 << 1e-3).  Asserted here, so that no row can pass emptily."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    mod = rng.uniform(0.1, 1.0, size=shape)
    if dtype.kind == "c":
        x = (mod * np.exp(2j * np.pi * rng.uniform(size=shape))).astype(dtype)
    else:
        x = (mod * rng.choice([-1.0, 1.0], size=shape)).astype(dtype)
    n = x.shape[0] if x.ndim == 2 else x.size
    assert n <= 2 ** 17 and np.all(np.abs(x) >= 1e-3 * np.max(np.abs(x)))
    return x


def check_sum(got, x, axis, mean=False):
    """sum (or mean, scaled by 1 / n) within n u64 sum|x_i| of the restatement, plus one rounding of the result type."""
    n = x.shape[0] if axis == 0 else x.size
    exact, mass = ar.total(x, axis)
    k = ar.LD(1) / n if mean else ar.LD(1)
    single = u_of(x.dtype) > 2.0 ** -53
    bound = n * 2.0 ** -53 * mass * k + (u_of(x.dtype) * np.abs(exact) * k if single else 0)
    assert np.all(np.abs(ar.widen(got) - exact * k) <= bound), (float(np.max(np.abs(ar.widen(got) - exact * k))), float(np.max(bound)))


def check_var(got, x, axis, std=False):
    n = x.shape[0] if axis == 0 else x.size
    var, mass = ar.variance(x, axis)
    single = u_of(x.dtype) > 2.0 ** -53
    bound = n * 2.0 ** -53 * mass / n + (u_of(x.dtype) * var if single else 0)
    if std:                                                                 # d sqrt(v) = dv / (2 sqrt(v)), and the root's own rounding
        exact = np.sqrt(var)
        with np.errstate(all="ignore"):                                     # (one row: var = 0 exactly, and so is the root)
            bound = np.where(exact > 0, bound / (2 * exact) + u_of(x.dtype) * exact, 0)
    else:
        exact = var
    assert np.all(np.abs(ar.widen(got) - exact) <= bound), (float(np.max(np.abs(ar.widen(got) - exact))), float(np.max(bound)))


def extreme_rows():
    """(name, 1-D float64 row) for min / max / argmin / argmax: the cases numpy's rule is made of."""
    rng = np.random.default_rng(99)
    rows = {}
    base = rng.standard_normal(300)
    rows["plain"] = base.copy()
    t = base.copy()
    t[[17, 150, 299]] = t.max() + 1.0
    t[[40, 41, 280]] = t.min() - 1.0
    rows["tie"] = t
    t = base.copy()
    t[[120, 250]] = np.nan
    rows["nan"] = t
    t = base.copy()
    t[0], t[-1] = t.max() + 1, t.min() - 1
    rows["first_max_last_min"] = t
    t = base.copy()
    t[0], t[-1] = t.min() - 1, t.max() + 1                       # element 299: the last lane (43) of the partial second workgroup
    rows["first_min_last_max"] = t
    rows["one"] = np.array([-0.0])
    rows["all_equal"] = np.full(257, 2.5)
    rows["all_nan"] = np.full(65, np.nan)
    rows["inf"] = np.array([1.0, -np.inf, np.inf, -np.inf, np.inf, 0.0])
    return rows
