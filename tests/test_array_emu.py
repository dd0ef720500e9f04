"""The array layer's kernels without a GPU: tests/emu/emu_array.cpp includes opticommpy_amd/csrc/array_kernels.h -- the bodies the
gfx950 kernels of engine_array.hip call -- and walks them with g++ over the device's grids and in the device's order of summation.
The descriptors, operand kinds and result types are the package's own (device.normalize_key, device.plan_binary), the inputs and
bounds those of tests/test_gpu_array.py (tests/array_shape_cases.py).  The rows one element either side of the capped grids run on
the GPU only.  The same walk is also built as a program under -fsanitize=address,undefined and run, never loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import array_restatement as ar
import array_shape_cases as sc
from opticommpy_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = _lib.METRICS_DTYPES


def build_emu(exe, flags=("-O2",)):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I",
                           os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_array.cpp"), "-o", str(exe)])
    return str(exe)


class FakeDevice:
    """What device.plan_binary needs of a DeviceArray, with the values on the host."""

    def __new__(cls, x):
        d = object.__new__(device.DeviceArray)
        x = np.ascontiguousarray(x)
        d.shape, d.dtype, d.device, d._ptr, d._owner, d.host = x.shape, x.dtype, 0, None, None, x
        d._owner = d
        return d


class Emu:
    def __init__(self, exe, tmp):
        self.exe, self.tmp = exe, str(tmp)

    def _run(self, head, *arrays):
        hd = np.zeros(32, dtype=np.int64)
        hd[:len(head)] = head
        src, dst = os.path.join(self.tmp, "in.bin"), os.path.join(self.tmp, "out.bin")
        with open(src, "wb") as f:
            f.write(hd.tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([self.exe, src, dst])
        return np.fromfile(dst, dtype=np.uint8)

    def getitem(self, x, key):
        axes, index = device.normalize_key(x.shape, key)
        st = device._c_strides(x.shape)
        counts = [c for _, c, _, _ in axes]
        pad = lambda v, fill: list(v) + [fill] * (4 - len(v))                                   # noqa: E731
        out = x
        if index is None or any((s, c, t) != (0, n, 1) for (s, c, t, _), n in zip(axes, x.shape)):
            n_out = int(np.prod(counts))
            raw = self._run([0, x.dtype.itemsize, x.ndim, sum(s * a[0] for s, a in zip(st, axes)), 0, n_out] + pad(counts, 1) +
                            pad([s * a[2] for s, a in zip(st, axes)], 0) + pad(device._c_strides(counts), 0), x) if n_out else np.zeros(0, np.uint8)
            out = raw.view(x.dtype).reshape([c for (_, c, _, keep) in axes if keep or index is not None])
        if index is None:
            return out
        kept = [c for _, c, _, keep in axes[1:] if keep]
        inner = int(np.prod(kept))
        if len(index) * inner == 0:
            return np.zeros([len(index)] + kept, dtype=x.dtype)
        raw = self._run([1, x.dtype.itemsize, x.shape[0], len(index), inner], index.astype(np.int64), out)
        return raw.view(x.dtype).reshape([len(index)] + kept)

    def transpose(self, x):
        return self._run([6, x.dtype.itemsize, x.shape[0], x.shape[1]], x).view(x.dtype).reshape(x.shape[::-1])

    def binary(self, op, x, other, swap=False):
        a, b, kind, inner, out_dtype, scalar, swap = device.plan_binary(FakeDevice(x), FakeDevice(other) if isinstance(other, np.ndarray) and other.ndim else other, swap)
        bh = np.zeros(0) if b is None else b.host
        head = [2, _lib.ARRAY_BINARY[op], int(swap), DT[a.dtype.name], DT[(out_dtype if b is None else b.dtype).name], DT[out_dtype.name], kind, a.size, inner]
        return self._run(head, np.array([scalar.real, scalar.imag]), a.host, bh).view(out_dtype).reshape(a.shape)

    def unary(self, op, x, out_dtype):
        return self._run([3, _lib.ARRAY_UNARY[op], DT[x.dtype.name], DT[np.dtype(out_dtype).name], x.size], x).view(out_dtype).reshape(x.shape)

    def reduce(self, op, x, center=None):
        rows, cols = (x.size, 1) if x.ndim == 1 else x.shape
        c = np.zeros((cols, 2)) if center is None else np.stack([np.real(center), np.imag(center)], -1).astype(np.float64).reshape(cols, 2)
        raw = self._run([4, op, DT[x.dtype.name], rows, cols], c, x)
        return raw[:cols * 16].view(np.float64).reshape(cols, 2), raw[cols * 16:].view(np.int64)

    def freq_shift(self, x, deltaF, Fs):
        return self._run([5, DT[x.dtype.name], x.shape[0], int(np.prod(x.shape[1:]))], np.array([deltaF, Fs]), x).view(np.complex128).reshape(x.shape)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_array") / "emu_array")


@pytest.fixture
def emu(exe, tmp_path):
    return Emu(exe, tmp_path)


def same(got, want, generates_nan=False):
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert sc.same_bits(got, want, generates_nan)


def same_arith(got, want):
    """+ - x / and sqrt: a NaN they generate has the hardware's sign (tests/array_shape_cases.py)."""
    same(got, want, generates_nan=True)


@pytest.mark.parametrize("dtype", sc.MOVE)
def test_movement_is_numpys(emu, dtype):
    for n in (1, 5, 65, 257):
        x = sc.values((n,), dtype, n)
        for k in (slice(None, None, -1), slice(None, None, 2), slice(1, None, 3), slice(None, None, 16), slice(-3, None), slice(None, None, -5000)):
            same(emu.getitem(x, k), x[k])
        y = sc.values((n, 2, 3), dtype, n)
        for k in ((slice(None), slice(None), 2), (slice(None, None, -2), 1), (0,), (-1, Ellipsis, 1), (slice(None), slice(None, None, -1), slice(1, None))):
            same(emu.getitem(y, k), y[k])
        z = sc.values((n, 5), dtype, n + 1)
        for k in ((slice(None), 4), (slice(None, None, -1), slice(None, None, 2)), (-1,), (slice(1, None, 3), slice(-2, None)), (Ellipsis, 0)):
            same(emu.getitem(z, k), z[k])
        for ind in ([0], list(range(n))[::-1], [-1, 0, -1], []):
            same(emu.getitem(y, ind), y[np.asarray(ind, dtype=np.int64)])
            same(emu.getitem(y, (ind, 1)), y[np.asarray(ind, dtype=np.int64), 1])
            same(emu.getitem(z, ind), z[np.asarray(ind, dtype=np.int64)])
            same(emu.getitem(z, (ind, slice(None, None, -2))), z[np.asarray(ind, dtype=np.int64), ::-2])
    for r, c in ((31, 1), (32, 2), (33, 65), (65, 33), (648, 30)):
        x = sc.values((r, c), dtype, r)
        same(emu.transpose(x), np.ascontiguousarray(x.T))


@pytest.mark.parametrize("dt", sc.ARITH)
@pytest.mark.parametrize("dt2", sc.ARITH)
def test_arithmetic(emu, dt, dt2):
    cplx = np.dtype(dt).kind == "c" or np.dtype(dt2).kind == "c"
    for n, cols in ((1, 3), (5, 5), (257, 3), (65, 5)):
        a, b = sc.values((n, cols), dt, n), sc.values((n, cols), dt2, n + 1)
        row, col = sc.values((cols,), dt2, 2), sc.values((n, 1), dt2, 3)
        for other in (b, row, col, 2.5, np.float32(0.1)):
            same_arith(emu.binary("add", a, other), a + other)
            same_arith(emu.binary("sub", a, other, swap=True), other - a)
            if not cplx:
                same_arith(emu.binary("mul", a, other), a * other)
                same_arith(emu.binary("div", a, other, swap=True), other / a)
        if cplx:
            sc.check_product(emu.binary("mul", a, b), a, b)
            sc.check_relative(emu.binary("div", a, b), ar.binary("div", a, b), 8)
            sc.check_relative(emu.binary("div", a, b, swap=True), ar.binary("div", b, a), 8)
    with np.errstate(all="ignore"):
        a, b = sc.specials(dt), sc.specials(dt2, partner=True)
        same_arith(emu.binary("add", a, b), a + b)
        same_arith(emu.binary("sub", a, b), a - b)
        if not cplx:
            same_arith(emu.binary("mul", a, b), a * b)
            same_arith(emu.binary("div", a, b), a / b)


@pytest.mark.parametrize("dt", sc.ARITH)
def test_unary(emu, dt):
    real = ar.REAL_OF[np.dtype(dt).name]
    for x in (sc.values((257,), dt, 1), sc.specials(dt)):
        same(emu.unary("neg", x, dt), -x)
        same(emu.unary("conj", x, dt), np.conj(x))
        same(emu.unary("real", x, real), np.ascontiguousarray(x.real))
        same(emu.unary("imag", x, real), np.ascontiguousarray(x.imag) if x.dtype.kind == "c" else np.zeros_like(x))
        for to in sc.ARITH:
            if not (x.dtype.kind == "c" and np.dtype(to).kind == "f"):
                with np.errstate(all="ignore"):
                    same(emu.unary("convert", x, to), x.astype(to))
    x = sc.values((1025,), dt, 2)
    sc.check_relative(emu.unary("abs", x, real), ar.unary("abs", x), 4)
    sc.check_relative(emu.unary("abs2", x, real), ar.unary("abs2", x), 4)
    for op, inp in (("exp", sc.values((1025,), dt, 3, scale=3.0)), ("angle", sc.angle_input(1025, dt, 4) if np.dtype(dt).kind == "c" else x),
                    ("sqrt", np.abs(x) if np.dtype(dt).kind == "f" else None)):
        if inp is not None:
            mine, numpys, allowed = sc.library_distance(op, inp, emu.unary(op, inp, real if op == "angle" else dt))
            assert mine <= allowed, (op, mine, numpys)
    if np.dtype(dt) == np.complex128:
        big = np.array([1e200 + 1e200j, -1e200 - 1e200j])
        assert np.all(np.isfinite(emu.unary("abs", big, np.float64)))


@pytest.mark.parametrize("dt", sc.ARITH)
def test_reductions(emu, dt):
    for shape in ((1,), (5,), (257,), (1025,), (300, 3), (sc.RED_SPAN + 1,)):
        x = sc.reduction_input(shape, dt, sum(shape))
        axis = 0 if len(shape) == 2 else None
        n = shape[0]
        s, _ = emu.reduce(_lib.ARRAY_SUM, x)
        total = s[:, 0] + 1j * s[:, 1] if x.dtype.kind == "c" else s[:, 0]
        got = total.astype(dt) if axis == 0 else total.astype(dt)[0]
        sc.check_sum(got, x, axis)
        v, _ = emu.reduce(_lib.ARRAY_SUMSQDEV, x, total / n)
        var = (v[:, 0] / n).astype(ar.REAL_OF[np.dtype(dt).name])
        sc.check_var(var if axis == 0 else var[0], x, axis)


@pytest.mark.parametrize("name", list(sc.extreme_rows()))
def test_extremes(emu, name):
    for dt in (np.float32, np.float64):
        x = sc.extreme_rows()[name].astype(dt)
        with np.errstate(all="ignore"):
            for op, val, arg in ((_lib.ARRAY_MIN, x.min(), x.argmin()), (_lib.ARRAY_MAX, x.max(), x.argmax())):
                v, a = emu.reduce(op, x)
                assert a[0] == arg and sc.same_bits(np.array(v[0, 0]).astype(dt), np.array(val))


def test_freq_shift(emu):
    for dt in sc.ARITH:
        for shape in ((1,), (257,), (1025, 2)):
            x = sc.values(shape, dt, 5)
            got, want = emu.freq_shift(x, -3.3e9, 64e9), ar.freq_shift(x, -3.3e9, 64e9)
            assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_the_walk_is_clean_under_the_sanitizers(tmp_path):
    """Built and run as a program with its own main: one call of every kind."""
    exe = build_emu(tmp_path / "emu_array_san", flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    e = Emu(exe, tmp_path)
    y = sc.values((65, 2, 3), np.complex128, 1)
    same(e.getitem(y, (slice(None, None, -2), 1, slice(1, None))), y[::-2, 1, 1:])
    same(e.getitem(y, ([-1, 0, 64], slice(None), 0)), y[[-1, 0, 64], :, 0])
    b = sc.values((33, 65), np.uint8, 2)
    same(e.transpose(b), np.ascontiguousarray(b.T))
    a = sc.values((257, 3), np.float32, 3)
    same_arith(e.binary("sub", a, sc.values((3,), np.float32, 4), swap=True), sc.values((3,), np.float32, 4) - a)
    same_arith(e.binary("add", a, sc.values((257, 1), np.float64, 5)), a + sc.values((257, 1), np.float64, 5))
    same(e.unary("convert", a, np.complex128), a.astype(np.complex128))
    x = sc.reduction_input((1025, 2), np.complex64, 6)
    s, _ = e.reduce(_lib.ARRAY_SUM, x)
    sc.check_sum((s[:, 0] + 1j * s[:, 1]).astype(np.complex64), x, 0)
    v, arg = e.reduce(_lib.ARRAY_MAX, a[:, 0].copy())
    assert arg[0] == a[:, 0].argmax()
    z = sc.values((257, 2), np.complex64, 7)
    assert np.max(np.abs(e.freq_shift(z, 1e9, 64e9) - ar.freq_shift(z, 1e9, 64e9))) <= 1e-12 * np.max(np.abs(z))
