"""The array layer of DeviceArray on the GPU: indexing, transposes, concatenation, element-wise arithmetic, conversion, reductions
and freqShift, with numpy as the definition.  Movement and the single-rounding operations are numpy's bit for bit; the multi-rounding
operations and the reductions are held to the extended-precision restatement within the bounds tests/array_shape_cases.py derives;
freqShift to the reference's fixtures within 1e-12 of the largest sample, the bound of the same operation inside simpleWDMTx.
No operation may download anything: ``transfer_counts()["d2h"]`` stays as it was until the test's own ``.get()``."""
import json
import os

import numpy as np
import pytest

import array_restatement as ar
import array_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import device as dev

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "array")


class NoDownload:
    """The body may upload but not download."""

    def __enter__(self):
        self.before = dev.transfer_counts()["d2h"]

    def __exit__(self, *exc):
        assert dev.transfer_counts()["d2h"] == self.before, "an operation downloaded its operand"


def on_device(fn, *host):
    """fn(*DeviceArrays) computed without a download -> the result on the host."""
    ds = [oa.to_device(h) for h in host]
    with NoDownload():
        r = fn(*ds)
    assert isinstance(r, oa.DeviceArray)
    return r.get()


def same(got, want, generates_nan=False):
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert sc.same_bits(got, want, generates_nan)


def same_arith(got, want):
    """+ - x / and sqrt: a NaN they generate has the hardware's sign (tests/array_shape_cases.py)."""
    same(got, want, generates_nan=True)


# ------------------------------------------------------------------ movement: bit-equal to numpy
STEPS = [1, -1, 2, -2, 3, -3, 16, 5000]


@pytest.mark.parametrize("dtype", sc.MOVE)
def test_slices_at_every_length_and_step(dtype):
    for n in sc.LENGTHS:
        x = sc.values((n,), dtype, n)
        d = oa.to_device(x)
        with NoDownload():
            keys = [slice(None, None, s) for s in STEPS] + [slice(1, None, 2), slice(-3, None), slice(None, -2), slice(-1000, 1000), slice(2, 1),
                                                            slice(n // 2, -n, -1), slice(n, n), slice(-1, None, -3)]
            got = [d[k] for k in keys]
        for k, g in zip(keys, got):
            same(g.get(), x[k])


@pytest.mark.parametrize("make", sc.SHAPES[1:])
def test_slices_and_integers_on_every_axis(make):
    for n in (1, 5, 65, 257):
        x = sc.values(make(n), np.complex128, n)
        d = oa.to_device(x)
        keys = [(slice(1, None, 2),), (slice(None), 0), (slice(None), -1), (Ellipsis, 0), (0,), (-1, Ellipsis), (slice(None, None, -1), slice(None, None, -1)),
                (slice(2, -2), slice(None)), (slice(None), slice(0, 0)), (slice(n, None),)]
        if x.ndim == 3:
            keys += [(slice(None), slice(None), 2), (slice(None), 1, slice(None, None, -2)), (0, 1, 2), (slice(None, None, 3), 1, -1), (Ellipsis, slice(1, 3)),
                     (-1, slice(None), 0)]
        else:
            keys += [(0, 0), (-1, -1)]
        for k in keys:
            with NoDownload():
                g = d[k]
            same(g.get(), x[k])


def test_slices_across_the_grid_cap():
    """One element either side of what a capped grid covers in one walk: the 16-byte path (contiguous, aligned) and the strided one."""
    for n in (sc.SPAN - 1, sc.SPAN + 1):
        x = sc.values((n + 2,), np.complex128, 1)                          # 16 MiB: one pack per lane
        d = oa.to_device(x)
        same(d[1:n + 1].get(), x[1:n + 1])                                # offset 16 bytes: aligned, the flat path
        b = sc.values((2 * n + 1,), np.uint8, 2)
        db = oa.to_device(b)
        same(db[::2].get(), b[::2])
        same(db[::-2].get(), b[::-2])
        same(db[3:n + 3].get(), b[3:n + 3])                               # contiguous but not 16-byte aligned: element by element


def test_flat_path_tail_bytes():
    for n in (1, 15, 16, 17, 31, 33, 4099):
        b = sc.values((n + 32,), np.uint8, n)
        same(oa.to_device(b)[16:16 + n].get(), b[16:16 + n])
        same(oa.to_device(b)[:n].get(), b[:n])


INDEXES = {"increasing": lambda n: np.arange(0, n, 2), "repeated": lambda n: np.repeat(np.arange(n)[:: max(n // 3, 1)], 3),
           "reversed": lambda n: np.arange(n)[::-1], "negative": lambda n: -1 - np.arange(0, n, 3), "empty": lambda n: np.zeros(0, dtype=np.int64)}


@pytest.mark.parametrize("kind", list(INDEXES))
@pytest.mark.parametrize("dtype", sc.MOVE)
def test_index_arrays_host_and_device(kind, dtype):
    for n in (1, 5, 64, 257, 1025):
        ind = INDEXES[kind](n)
        for shape in ((n,), (n, 2), (n, 5), (n, 2, 3)):
            x = sc.values(shape, dtype, n)
            d = oa.to_device(x)
            routes = [ind, list(ind), ind.astype(np.int32), oa.to_device(ind.astype(np.int64)), oa.to_device(ind.astype(np.int32))]
            for r in routes:
                with NoDownload():
                    g = d[r]
                same(g.get(), x[ind])
            if x.ndim >= 2:
                di = oa.to_device(ind.astype(np.int64))
                same(d[ind, :].get(), x[ind, :])
                same(d[di, 1].get(), x[ind, 1])
                same(d[ind, ::-1].get(), x[ind, ::-1])
            if x.ndim == 3:
                same(d[list(ind), 1, 1:].get(), x[ind, 1, 1:])


def test_device_index_is_clamped_as_documented():
    x = sc.values((7, 2), np.float64, 0)
    ind = np.array([-9, -8, -7, 6, 7, 100], dtype=np.int64)
    same(oa.to_device(x)[oa.to_device(ind)].get(), x[[0, 0, 0, 6, 6, 6]])
    with pytest.raises(IndexError):
        oa.to_device(x)[ind]


@pytest.mark.parametrize("dtype", sc.MOVE)
def test_transposes(dtype):
    for r in (31, 32, 33):
        for c in (1, 2, 63, 64, 65):
            x = sc.values((r, c), dtype, r * c)
            same(on_device(lambda d: d.T, x), np.ascontiguousarray(x.T))
            same(on_device(lambda d: d.transpose(), np.ascontiguousarray(x.T)), x)
    x = sc.values((5,), dtype, 5)
    same(on_device(lambda d: d.T, x), x)
    same(on_device(lambda d: d.T, x.reshape(5, 1)), x.reshape(1, 5))
    assert oa.to_device(np.zeros((0, 3), dtype=dtype)).T.shape == (3, 0)


def test_transpose_of_a_codeword_block():
    x = sc.values((648, 30), np.uint8, 648)
    same(on_device(lambda d: d.T, x), np.ascontiguousarray(x.T))
    x = sc.values((1025, 3), np.float64, 3)
    same(on_device(lambda d: d.T, x), np.ascontiguousarray(x.T))


@pytest.mark.parametrize("dtype", sc.MOVE)
def test_concatenate_and_stack(dtype):
    shapes = {0: [(3, 2, 3), (0, 2, 3), (65, 2, 3)], 1: [(5, 1, 3), (5, 0, 3), (5, 4, 3)], 2: [(5, 2, 1), (5, 2, 0), (5, 2, 7)]}
    for axis, shp in shapes.items():
        for count in (1, 2, 3):
            xs = [sc.values(s, dtype, i + 1) for i, s in enumerate(shp[:count])]
            for ax in (axis, axis - 3):
                same(on_device(lambda *d: oa.concatenate(d, axis=ax), *xs), np.concatenate(xs, axis=ax))
    xs = [sc.values((257,), dtype, i) for i in range(3)]
    same(on_device(lambda *d: oa.concatenate(d), *xs), np.concatenate(xs))
    same(on_device(lambda *d: oa.stack(d, 0), *xs), np.stack(xs, 0))
    same(on_device(lambda *d: oa.stack(d, -1), *xs), np.stack(xs, -1))
    xs = [sc.values((33, 2), dtype, i) for i in range(2)]
    same(on_device(lambda *d: oa.stack(d, axis=-1), *xs), np.stack(xs, -1))
    same(on_device(lambda *d: oa.stack(d), *xs), np.stack(xs))
    x4 = [sc.values((2, 3, 2, 5), dtype, i) for i in range(2)]
    same(on_device(lambda *d: oa.concatenate(d, axis=3), *x4), np.concatenate(x4, axis=3))


@pytest.mark.parametrize("dtype", sc.MOVE + [np.float32, np.complex64])
def test_zeros_and_full(dtype):
    v = sc.values((1,), dtype, 5)[0]
    for shape in ((0,), (1,), (257,), (65, 3)):
        with NoDownload():
            z, f = oa.zeros(shape, dtype), oa.full(shape, v, dtype)
        same(z.get(), np.zeros(shape, dtype))
        same(f.get(), np.full(shape, v, dtype))


# ------------------------------------------------------------------ single-rounding operations: bit-equal to numpy
@pytest.mark.parametrize("dt", sc.ARITH)
@pytest.mark.parametrize("dt2", sc.ARITH)
def test_add_sub_and_real_products_are_numpys_bits(dt, dt2):
    for n in (1, 3, 5, 65, 1025):
        a, b = sc.values((n,), dt, n), sc.values((n,), dt2, n + 1)
        same_arith(on_device(lambda x, y: x + y, a, b), a + b)
        same_arith(on_device(lambda x, y: x - y, a, b), a - b)
        if np.dtype(dt).kind == "f" and np.dtype(dt2).kind == "f":
            same_arith(on_device(lambda x, y: x * y, a, b), a * b)
            same_arith(on_device(lambda x, y: x / y, a, b), a / b)
    a, b = sc.specials(dt), sc.specials(dt2, partner=True)
    with np.errstate(all="ignore"):
        same_arith(on_device(lambda x, y: x + y, a, b), a + b)
        same_arith(on_device(lambda x, y: x - y, a, b), a - b)
        if np.dtype(dt).kind == "f" and np.dtype(dt2).kind == "f":
            same_arith(on_device(lambda x, y: x * y, a, b), a * b)
            same_arith(on_device(lambda x, y: x / y, a, b), a / b)


@pytest.mark.parametrize("dt", sc.ARITH)
def test_unary_single_rounding_operations_are_numpys_bits(dt):
    for x in [sc.values((n,), dt, n) for n in sc.LENGTHS] + [sc.specials(dt), sc.values((65, 2, 3), dt, 1)]:
        same(on_device(lambda d: -d, x), -x)
        same(on_device(lambda d: +d, x), +x)
        same(on_device(lambda d: d.conj(), x), np.conj(x))
        same(on_device(lambda d: d.real, x), np.ascontiguousarray(x.real))
        same(on_device(lambda d: d.imag, x), np.ascontiguousarray(x.imag) if x.dtype.kind == "c" else np.zeros_like(x))
        if x.dtype.kind == "f":
            same(on_device(lambda d: abs(d), x), np.abs(x))
            same(on_device(lambda d: d.abs(), x), np.abs(x))
        for to in sc.ARITH:
            if x.dtype.kind == "c" and np.dtype(to).kind == "f":
                continue
            with np.errstate(all="ignore"):
                same(on_device(lambda d: d.astype(to), x), x.astype(to))


SCALARS = [2, 2.5, 0.1, -3, np.float32(0.1), np.float64(0.1)]


@pytest.mark.parametrize("dt", sc.ARITH)
def test_real_scalars_are_numpys_bits_on_both_sides(dt):
    """Python scalar (weak), numpy scalar (strong) on the left and on the right of every operator; a real scalar times a complex array
    included.  Quotients with a complex side are Smith's form: multi-rounding, held to their bound below."""
    x = np.concatenate([sc.values((257,), dt, 7), np.array([0.0, -0.0, 1.0], dtype=dt)])
    real = x.dtype.kind == "f"
    for s in SCALARS:
        for got, want in [(lambda d: d + s, x + s), (lambda d: s + d, s + x), (lambda d: d - s, x - s), (lambda d: s - d, s - x), (lambda d: d * s, x * s),
                          (lambda d: s * d, s * x)]:
            same_arith(on_device(got, x), want)
        if real:
            with np.errstate(all="ignore"):
                same_arith(on_device(lambda d: d / s, x), x / s)
                same_arith(on_device(lambda d: s / d, x), s / x)
    if real:
        same_arith(on_device(lambda d: d ** 2, x), x ** 2)


@pytest.mark.parametrize("make", sc.SHAPES)
@pytest.mark.parametrize("dt", [np.float32, np.complex128])
def test_every_broadcast_kind_against_every_shape(make, dt):
    """same, scalar, row and column against 1-D, (n, 1), (n, 2), (n, 3), (n, 5), (n, 2, 3); a numpy array on the left reaches the reflected
    operator (no download) and gives a DeviceArray."""
    for n in (1, 4, 65, 257):
        shape = make(n)
        x = sc.values(shape, dt, n)
        row = sc.values((shape[-1],), dt, 3)
        for op in (lambda p, q: p + q, lambda p, q: p - q, lambda p, q: q - p):
            same_arith(on_device(lambda d, e: op(d, e), x, x[::-1].copy()), op(x, x[::-1].copy()))                  # same
            same_arith(on_device(lambda d: op(d, np.float64(1.5)), x), op(x, np.float64(1.5)))                      # scalar
            same_arith(on_device(lambda d: op(d, row), x), op(x, row))                                              # row from the host
            same_arith(on_device(lambda d: op(d, list(row)), x), op(x, np.array(list(row))))
            same_arith(on_device(lambda d, r: op(d, r), x, row), op(x, row))                                        # row on the device
            if len(shape) >= 2:
                col = sc.values((n,) + (1,) * (len(shape) - 1), dt, 4)
                same_arith(on_device(lambda d, c: op(d, c), x, col), op(x, col))                                    # column


def test_numpy_on_the_left_reaches_the_reflected_operator():
    x = sc.values((65, 3), np.float64, 0)
    row = np.array([1.0, 2.0, 4.0])
    d = oa.to_device(x)
    with NoDownload():
        rs = [np.float64(2) * d, row - d, np.float64(1) / d, row * d, row + d, row / d, 2 - d, 2j * d, np.complex64(1j) + d, np.float32(3) - d]
    with np.errstate(all="ignore"):
        want = [np.float64(2) * x, row - x, np.float64(1) / x, row * x, row + x, row / x, 2 - x, 2j * x, np.complex64(1j) + x, np.float32(3) - x]
    for r, w in zip(rs, want):
        assert isinstance(r, oa.DeviceArray)
        same_arith(r.get(), w)
    before = dev.transfer_counts()["d2h"]
    assert isinstance(np.abs(d), np.ndarray) and isinstance(np.asarray(d), np.ndarray)         # these keep downloading, as before
    assert dev.transfer_counts()["d2h"] == before + 2


def test_element_wise_across_the_grid_cap():
    """One element either side of what a capped grid covers in one walk, at 4 float32 per lane and at 1 complex128 per lane."""
    for dt in (np.float32, np.complex128):
        V = sc.vec_width(dt)
        for n in (sc.SPAN * V - 1, sc.SPAN * V + 1):
            a, b = sc.values((n,), dt, 1), sc.values((n,), dt, 2)
            same_arith(on_device(lambda x, y: x - y, a, b), a - b)
            same(on_device(lambda x: -x, a), -a)
            same_arith(on_device(lambda x: 0.5 * x, a), 0.5 * a)


def test_x_plus_equals_rebinds():
    x = sc.values((5,), np.float64, 0)
    d = oa.to_device(x)
    keep = d
    d += 1
    assert d is not keep and np.array_equal(keep.get(), x) and np.array_equal(d.get(), x + 1)


# ------------------------------------------------------------------ multi-rounding operations: the restatement within derived bounds
@pytest.mark.parametrize("dt", [np.complex64, np.complex128])
@pytest.mark.parametrize("dt2", sc.ARITH)
def test_complex_products(dt, dt2):
    for n in (1, 5, 257, 1025):
        a, b = sc.values((n, 2), dt, n), sc.values((n, 2), dt2, n + 1)
        out = np.result_type(dt, dt2)
        got = on_device(lambda x, y: x * y, a, b)
        assert got.dtype == out
        sc.check_product(got, a, b)
        sc.check_product(on_device(lambda x, y: y * x, a, b), b, a)
        sc.check_product(on_device(lambda x: x ** 2, a), a, a)
        s = 0.3 - 1.7j
        sc.check_product(on_device(lambda x: x * s, a), a, np.asarray(s).astype(dt))
        sc.check_product(on_device(lambda x: np.complex128(s) * x, a), a.astype(np.complex128), np.complex128(s))
        row = sc.values((2,), dt2, 5)
        sc.check_product(on_device(lambda x: x * row, a), a, np.broadcast_to(row, a.shape))


@pytest.mark.parametrize("dt", sc.ARITH)
@pytest.mark.parametrize("dt2", [np.complex64, np.complex128])
def test_complex_quotients(dt, dt2):
    for n in (1, 5, 257, 1025):
        a, b = sc.values((n, 3), dt, n), sc.values((n, 3), dt2, n + 1)
        sc.check_relative(on_device(lambda x, y: x / y, a, b), ar.binary("div", a, b), 8)
        sc.check_relative(on_device(lambda x, y: y / x, a, b), ar.binary("div", b, a), 8)
        out = np.result_type(dt, dt2)
        s = np.asarray(0.3 - 1.7j).astype(out)[()]
        sc.check_relative(on_device(lambda x: x / (0.3 - 1.7j), a), ar.binary("div", a, s), 8)
        sc.check_relative(on_device(lambda x: (0.3 - 1.7j) / x, b), ar.binary("div", np.asarray(0.3 - 1.7j).astype(dt2)[()], b), 8)
        s2 = np.asarray(2.5).astype(dt2)[()]
        sc.check_relative(on_device(lambda x: x / 2.5, b), ar.binary("div", b, s2), 8)           # complex / real scalar: Smith's too
    # components of very different size on either side of Smith's branch
    b = np.array([1e-3 + 1j, 1 + 1e-3j, 1 + 1j, -1 + 1j, 1e150 + 1e-150j, 1e-150 - 1e150j], dtype=np.complex128)
    a = sc.values((6,), np.complex128, 0)
    sc.check_relative(on_device(lambda x, y: x / y, a, b), ar.binary("div", a, b), 8)


@pytest.mark.parametrize("dt", sc.ARITH)
def test_abs_and_abs2(dt):
    for n in sc.LENGTHS:
        x = sc.values((n,), dt, n)
        for got, op in ((on_device(lambda d: d.abs(), x), "abs"), (on_device(lambda d: abs(d), x), "abs"), (on_device(lambda d: d.abs2(), x), "abs2")):
            assert got.dtype == ar.REAL_OF[np.dtype(dt).name]
            sc.check_relative(got, ar.unary(op, x), 4)
    if np.dtype(dt) == np.complex128:
        big = np.array([1e200 + 1e200j, -1e200 + 1e200j, 1e200 - 1e-200j, 3e-200 + 4e-200j])
        got = on_device(lambda d: d.abs(), big)
        assert np.all(np.isfinite(got))
        sc.check_relative(got, ar.unary("abs", big), 4)


@pytest.mark.parametrize("dt", sc.ARITH)
@pytest.mark.parametrize("op", ["exp", "angle", "sqrt"])
def test_library_functions_within_four_times_numpys_own_distance(dt, op):
    n = 4099
    if op == "sqrt":
        if np.dtype(dt).kind == "c":
            return
        x = np.abs(sc.values((n,), dt, 1)) * np.float32(100)
    elif op == "angle":
        x = sc.angle_input(n, dt, 2) if np.dtype(dt).kind == "c" else sc.values((n,), dt, 2)
    else:
        x = sc.values((n,), dt, 3, scale=3.0)
    got = on_device(lambda d: getattr(d, op)(), x)
    assert got.dtype == (ar.REAL_OF[np.dtype(dt).name] if op == "angle" else np.dtype(dt))
    mine, numpys, allowed = sc.library_distance(op, x, got)
    print(f"{op} {np.dtype(dt).name}: device {mine:.3f} u, numpy {numpys:.3f} u, allowed {allowed:.3f} u")
    assert mine <= allowed
    if op == "angle" and np.dtype(dt).kind == "c":
        assert got[0] == np.angle(x[0]) == ar.REAL_OF[np.dtype(dt).name](np.pi) and got[1] == np.angle(x[1]) == -got[0]
    if op == "sqrt":
        with np.errstate(all="ignore"):
            same_arith(on_device(lambda d: d.sqrt(), np.array([-1.0, 0.0, -0.0, 4.0, np.inf], dtype=dt)), np.sqrt(np.array([-1.0, 0.0, -0.0, 4.0, np.inf], dtype=dt)))


# ------------------------------------------------------------------ reductions
def red_lengths():
    return sc.LENGTHS + [sc.RED_SPAN - 1, sc.RED_SPAN + 1, 2 * sc.RED_SPAN]         # (2^17: the largest the bounds are derived for)


def numpy_scalar(v, dtype):
    assert isinstance(v, np.generic) and v.dtype == dtype, (type(v), getattr(v, "dtype", None))


@pytest.mark.parametrize("dt", sc.ARITH)
def test_sums_means_and_variances(dt):
    real = ar.REAL_OF[np.dtype(dt).name]
    for n in red_lengths():
        x = sc.reduction_input((n,), dt, n)
        d = oa.to_device(x)
        with NoDownload():
            r = [(d.sum(), d.mean(), d.var(), d.std()) for _ in range(2)]
        assert all(np.array(a).tobytes() == np.array(b).tobytes() for a, b in zip(*r))          # repeats bit for bit
        s, m, v, sd = r[0]
        numpy_scalar(s, np.dtype(dt)), numpy_scalar(m, np.dtype(dt)), numpy_scalar(v, real), numpy_scalar(sd, real)
        sc.check_sum(s, x, None), sc.check_sum(m, x, None, mean=True), sc.check_var(v, x, None), sc.check_var(sd, x, None, std=True)
        if n > 1:                                                       # ddof only changes the divisor of the same sum
            assert abs(float(d.var(ddof=1)) * (n - 1) / n - float(v)) <= 4 * sc.u_of(dt) * float(v)
            assert abs(float(d.std(ddof=1)) ** 2 * (n - 1) / n - float(v)) <= 8 * sc.u_of(dt) * float(v)


@pytest.mark.parametrize("dt", sc.ARITH)
@pytest.mark.parametrize("cols", [1, 2, 3, 5])
def test_reductions_over_axis_0(dt, cols):
    for n in (1, 5, 257, 1025, sc.RED_SPAN + 1):
        x = sc.reduction_input((n, cols), dt, n + cols)
        d = oa.to_device(x)
        with NoDownload():
            r = [(d.sum(axis=0), d.mean(axis=0), d.var(axis=0), d.std(axis=0), d.sum(), d.std()) for _ in range(2)]
        assert all(np.array(a).tobytes() == np.array(b).tobytes() for a, b in zip(*r))
        s, m, v, sd, s_all, sd_all = r[0]
        assert s.shape == (cols,) and isinstance(s, np.ndarray) and s.dtype == dt and v.dtype == ar.REAL_OF[np.dtype(dt).name]
        sc.check_sum(s, x, 0), sc.check_sum(m, x, 0, mean=True), sc.check_var(v, x, 0), sc.check_var(sd, x, 0, std=True)
        sc.check_sum(s_all, x, None), sc.check_var(sd_all, x, None, std=True)
        if np.dtype(dt).kind == "f":
            with NoDownload():
                e = [(d.min(axis=0), d.max(axis=0), d.argmin(axis=0), d.argmax(axis=0)) for _ in range(2)]
            for got, want in zip(e[0], (x.min(axis=0), x.max(axis=0), x.argmin(axis=0), x.argmax(axis=0))):
                assert got.dtype == want.dtype and np.array_equal(got, want)
            assert all(np.array_equal(a, b) for a, b in zip(*e))
    x = sc.reduction_input((65, 2, 3), dt, 1)                               # axis=None over three dimensions
    sc.check_sum(oa.to_device(x).sum(), x, None)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(sc.extreme_rows()))
def test_extremes_are_numpys(dt, name):
    x = sc.extreme_rows()[name].astype(dt)
    d = oa.to_device(x)
    with NoDownload():
        got = [(d.min(), d.max(), d.argmin(), d.argmax()) for _ in range(2)]
    with np.errstate(all="ignore"):
        want = (x.min(), x.max(), x.argmin(), x.argmax())
    for g, g2, w in zip(got[0], got[1], want):
        assert isinstance(g, np.generic) and g.dtype == w.dtype and sc.same_bits(np.array(g), np.array(w)) and sc.same_bits(np.array(g), np.array(g2)), name


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_extremes_at_every_length(dt):
    for n in red_lengths():
        x = sc.values((n,), dt, n)
        for at in (0, n - 1, n // 2):                                   # the extreme in the first, the last and a middle element
            y = x.copy()
            y[at] = 100.0
            d = oa.to_device(y)
            assert d.argmax() == at and d.max() == 100 and d.argmin() == y.argmin() and d.min() == y.min()
            d = oa.to_device(-y)
            assert d.argmin() == at and d.min() == -100


def test_empty_arrays():
    e = oa.to_device(np.zeros((0, 3), dtype=np.complex64))
    with NoDownload():
        assert e.sum() == 0 and e.sum(axis=0).shape == (3,) and (-e).shape == (0, 3) and e[:, 1].shape == (0,) and e.T.shape == (3, 0)
        assert (e * 2).dtype == np.complex64 and e.abs().dtype == np.float32 and oa.concatenate([e, e]).shape == (0, 3)
    for name in ("mean", "var", "std"):
        with pytest.raises(ValueError):
            getattr(e, name)()
    with pytest.raises(ValueError):
        oa.to_device(np.zeros(0)).max()


def test_infinite_sums_and_no_degrees_of_freedom():
    """An infinite imaginary sum leaves the real one alone; var and std with ddof >= n are NaN with numpy's warning."""
    x = np.array([1 + 2j, 3 + np.inf * 1j, -1 - 1j])
    x[1] = complex(3.0, np.inf)
    s = oa.to_device(x).sum()
    assert s.real == 3.0 and s.imag == np.inf
    s0 = oa.to_device(np.stack([x, x.conj()], axis=1)).sum(axis=0)
    assert np.array_equal(s0.real, [3.0, 3.0]) and np.array_equal(s0.imag, [np.inf, -np.inf])
    d = oa.to_device(np.array([1.0, 2.0, 4.0]))
    with pytest.warns(RuntimeWarning, match="Degrees of freedom"):
        assert np.isnan(d.var(ddof=3)) and np.isnan(d.std(ddof=4))
    assert abs(d.var(ddof=2) - np.array([1.0, 2.0, 4.0]).var(ddof=2)) <= 4 * 2.0 ** -53 * d.var(ddof=2)


# ------------------------------------------------------------------ freqShift
def load(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


@pytest.mark.parametrize("case", ["one_dim", "two_modes", "far"])
def test_freqshift_fixture(case):
    g = load(case)
    x, c = g["x"], g["cfg"]
    a = oa.freqShift(x, c["deltaF"], c["Fs"])
    with NoDownload():
        b = oa.freqShift(oa.to_device(x), c["deltaF"], c["Fs"])
    assert isinstance(a, np.ndarray) and isinstance(b, oa.DeviceArray) and a.dtype == np.complex128 and a.shape == g["y"].shape
    assert np.array_equal(a, b.get())                                       # both kinds of argument: identical bits
    err = float(np.max(np.abs(a - g["y"])) / np.max(np.abs(g["y"])))
    rest = float(np.max(np.abs(a - ar.freq_shift(x, c["deltaF"], c["Fs"]))) / np.max(np.abs(g["y"])))
    print(f"freqShift {case}: {err:.2e} of the largest sample from the reference, {rest:.2e} from the restatement")
    assert err <= 1e-12
    assert abs(2 * np.pi * c["deltaF"] * (len(x) - 1) / c["Fs"]) > (1e6 if case == "far" else 1.0)
    assert np.max(np.abs(g["y"] - x)) > 1e-3 * np.max(np.abs(x))           # the shift is not the identity


@pytest.mark.parametrize("dt", sc.ARITH)
def test_freqshift_at_every_length_and_type(dt):
    for n in sc.LENGTHS + [sc.SPAN + 1]:
        for shape in ((n,), (n, 3)) if n < 2000 else ((n,),):
            x = sc.values(shape, dt, n)
            got = on_device(lambda d: oa.freqShift(d, -3.3e9, 64e9), x)
            want = ar.freq_shift(x, -3.3e9, 64e9)
            assert got.dtype == np.complex128 and got.shape == shape
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
