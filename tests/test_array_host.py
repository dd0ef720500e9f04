"""Host side of the array layer of DeviceArray (opticommpy_amd/device.py) without a GPU: the key normalisation is numpy's over every
small slice and tuple, what is out of scope is refused before the library is even loaded, result types are np.result_type's over
the whole table, operand shapes are classified as the kernels take them, the structs are packed as include/ssf.h lays them out
and the C ABI refuses bad arguments before it needs a device."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import array_restatement as ar
import opticommpy_amd as oa
from opticommpy_amd import _lib, device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITH = (np.float32, np.float64, np.complex64, np.complex128)


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the checks under test come before it."""
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def fake_device(shape, dtype, dev=0):
    d = object.__new__(oa.DeviceArray)                      # (no GPU needed: the checks are on type and shape)
    d.shape, d.dtype, d.device, d._ptr, d._owner = tuple(shape), np.dtype(dtype), dev, None, d
    return d


def test_public_names():
    for name in ("concatenate", "stack", "zeros", "full", "freqShift"):
        assert getattr(oa, name) is getattr(device, name) and name in oa.__all__
    from opticommpy_amd import core
    assert core.freqShift is device.freqShift
    assert oa.DeviceArray.__array_priority__ > 0 and not hasattr(oa.DeviceArray, "__array_ufunc__")
    assert not hasattr(oa.DeviceArray, "__setitem__") and not hasattr(oa.DeviceArray, "__iadd__")


def test_every_slice_is_numpys():
    vals = [None] + list(range(-7, 8))
    n_checked = 0
    for n in range(7):
        x = np.arange(n) + 100
        for start, stop, step in itertools.product(vals, vals, vals):
            key = slice(start, stop, step)
            if step == 0:
                with pytest.raises(ValueError):
                    device.normalize_key(x.shape, key)
                continue
            (s, c, st, keep), = device.normalize_key(x.shape, key)[0]
            want = x[key]
            assert keep and c == len(want) and np.array_equal(x[s + st * np.arange(c)] if c else want, want), (n, key)
            n_checked += 1
    assert n_checked == 7 * 16 * 16 * 15


def test_every_integer_is_numpys():
    for n in range(7):
        x = np.arange(n)
        for i in range(-8, 9):
            if -n <= i < n:
                assert device.normalize_key((n,), i) == ([(x[i], 1, 1, False)], None)
                assert device.normalize_key((n,), np.int64(i)) == ([(x[i], 1, 1, False)], None)
            else:
                with pytest.raises(IndexError):
                    device.normalize_key((n,), i)


PER_AXIS = [0, -1, 1, slice(None), slice(1, None, 2), slice(None, None, -1), slice(-1, 0, -2), slice(5, 1), slice(-100, 100, 3), Ellipsis]


@pytest.mark.parametrize("shape", [(4,), (3, 4), (2, 3, 4), (0, 3), (3, 0, 2), (1, 1, 1), (2, 2, 2, 3)])
def test_tuples_are_numpys(shape):
    x = np.arange(int(np.prod(shape))).reshape(shape)
    n_checked = 0
    for r in range(0, min(len(shape), 3) + 1):
        for key in itertools.product(PER_AXIS, repeat=r):
            if sum(k is Ellipsis for k in key) > 1:
                continue
            try:
                want = x[key]
            except IndexError:
                with pytest.raises(IndexError):
                    device.normalize_key(shape, key)
                continue
            got = ar.apply_normalized(x, key)
            assert got.shape == want.shape and np.array_equal(got, want), key
            n_checked += 1
    assert n_checked > 10


@pytest.mark.parametrize("ind", [[0, 2, 3], [3, 3, 0, 0], [4, 3, 2, 1, 0], [-1, -5, 0], np.array([1, 2], dtype=np.int32), np.array([], dtype=np.int64),
                                 []])
def test_index_sequences_are_numpys(ind):
    x = np.arange(30).reshape(5, 3, 2)
    for key in (ind, (ind,), (ind, slice(None)), (ind, 1), (ind, slice(None, None, -1), 0), (ind, Ellipsis, 1), (ind, Ellipsis)):
        want = x[tuple(np.asarray(k, dtype=np.int64) if k is ind else k for k in key)] if isinstance(key, tuple) else x[np.asarray(ind, dtype=np.int64)]
        got = ar.apply_normalized(x, key)
        assert got.shape == want.shape and np.array_equal(got, want), key
    axes, index = device.normalize_key((5,), ind)
    assert index.dtype == np.int64 and (index >= 0).all()


def test_indexing_refusals_come_before_the_library(no_library):
    d = fake_device((6, 3), np.complex128)
    for key, exc, word in [(None, IndexError, "None"), ((slice(None), None), IndexError, "reshape"), (np.array([True] * 6), IndexError, "boolean"),
                           ([True, False], IndexError, "boolean"), (True, IndexError, "boolean"),
                           (([0, 1], [0, 1]), IndexError, "more than one"), ((slice(None), [0, 1]), IndexError, "first position"),
                           ((0, np.array([1])), IndexError, "first position"), ([6], IndexError, "out of bounds"), ([-7], IndexError, "out of bounds"),
                           ([[0, 1]], IndexError, "1-D"), ([0.5], IndexError, "integers"), (1.5, IndexError, "supported"), ("a", IndexError, "supported"),
                           ((0, 0, 0), IndexError, "too many"), ((Ellipsis, Ellipsis), IndexError, "ellipsis"), (6, IndexError, "out of bounds"),
                           (fake_device((2,), np.float64), IndexError, "int32 or int64"), (fake_device((2, 1), np.int64), IndexError, "1-D")]:
        with pytest.raises(exc, match=word):
            d[key]
    with pytest.raises(ValueError, match="zero"):
        d[::0]
    with pytest.raises(IndexError, match="ndim <= 4"):
        fake_device((1, 1, 1, 1, 1), np.float64)[0]
    with pytest.raises(TypeError, match="1, 2, 4, 8 or 16"):
        fake_device((4,), np.dtype([("a", np.uint8, 3)]))[1:]
    with pytest.raises(ValueError, match="different GPUs"):
        d[fake_device((2,), np.int64, dev=1)]
    with pytest.raises(ValueError, match="selected device"):
        fake_device((6,), np.float64, dev=3)[1:]
    with pytest.raises(TypeError):
        d[0] = 1                                                    # no __setitem__


def test_movement_refusals_come_before_the_library(no_library):
    with pytest.raises(ValueError, match="ndim <= 2"):
        fake_device((2, 2, 2), np.float64).T
    with pytest.raises(ValueError, match="ndim <= 2"):
        fake_device((2, 2, 2), np.float64).transpose()
    a, b = fake_device((4, 2), np.float64), fake_device((4, 3), np.float64)
    with pytest.raises(ValueError, match="must match"):
        oa.concatenate([a, b], axis=0)
    with pytest.raises(ValueError, match="out of bounds"):
        oa.concatenate([a, a], axis=2)
    with pytest.raises(TypeError, match="one dtype"):
        oa.concatenate([a, fake_device((4, 2), np.float32)])
    with pytest.raises(TypeError, match="to_device"):
        oa.concatenate([a, np.zeros((4, 2))])
    with pytest.raises(TypeError):
        oa.concatenate([])
    with pytest.raises(ValueError, match="different GPUs"):
        oa.concatenate([a, fake_device((4, 2), np.float64, dev=1)])
    with pytest.raises(ValueError, match="ndim"):
        oa.concatenate([fake_device((1,) * 5, np.float64)])
    with pytest.raises(ValueError, match="axis=0 and axis=-1"):
        oa.stack([a, a], axis=1)
    with pytest.raises(ValueError, match="same shape"):
        oa.stack([a, b])
    with pytest.raises(ValueError, match="ndim"):
        oa.stack([fake_device((1, 1, 1, 1), np.float64)])
    with pytest.raises(TypeError, match="1, 2, 4, 8 or 16"):
        oa.full((3,), 0, np.dtype([("a", np.uint8, 3)]))


def test_arithmetic_refusals_come_before_the_library(no_library):
    d = fake_device((6, 3), np.complex128)
    r = fake_device((6, 3), np.float64)
    i = fake_device((6, 3), np.int32)
    for call in (lambda: i + 1, lambda: 1 + i, lambda: -i, lambda: abs(i), lambda: i.conj(), lambda: i.real, lambda: i.astype(np.float64), lambda: i.sum(),
                 lambda: d + i, lambda: i.exp(), lambda: +i, lambda: i ** 2, lambda: i.abs2(), lambda: i.angle(), lambda: i.imag, lambda: i.sqrt()):
        with pytest.raises(TypeError, match="float32, float64, complex64, complex128"):
            call()
    for call in (lambda: d + np.zeros((6, 3)), lambda: np.zeros((6, 3)) * d, lambda: d - np.zeros((6, 1)), lambda: d / np.zeros(6),
                 lambda: fake_device((5000,), np.float64) + np.zeros(5000), lambda: d * [[1, 2, 3]]):
        with pytest.raises(TypeError, match="to_device"):
            call()
    with pytest.raises(ValueError, match="do not combine"):
        d + fake_device((6, 2), np.complex128)
    with pytest.raises(ValueError, match="do not combine"):
        d * fake_device((1, 3), np.complex128)
    with pytest.raises(ValueError, match="different GPUs"):
        d + fake_device((6, 3), np.complex128, dev=1)
    for p in (3, 2.0, np.int64(2), 0.5, -1, d):
        with pytest.raises(TypeError, match="integer 2"):
            d ** p
    with pytest.raises(TypeError, match="real arrays"):
        d.sqrt()
    with pytest.raises(TypeError, match=r"\.real"):
        d.astype(np.float64)
    with pytest.raises(TypeError, match=r"\.real"):
        fake_device((3,), np.complex64).astype(np.float32)
    with pytest.raises(TypeError, match="converts among"):
        r.astype(np.int32)
    with pytest.raises(TypeError):
        d + "a"
    with pytest.raises(TypeError, match="not supported"):
        d + np.array(["a", "b", "c"])
    with pytest.raises(TypeError, match="float128|longdouble|not supported"):
        r * np.longdouble(2)


def test_reduction_refusals_come_before_the_library(no_library):
    d = fake_device((6, 3), np.complex128)
    for name in ("min", "max", "argmin", "argmax"):
        with pytest.raises(TypeError, match="real arrays"):
            getattr(d, name)()
    r = fake_device((6, 3, 2), np.float64)
    with pytest.raises(ValueError, match="axis=None and axis=0"):
        r.sum(axis=1)
    with pytest.raises(ValueError, match="1-D and 2-D"):
        r.sum(axis=0)
    e = fake_device((0,), np.float32)
    for name in ("mean", "var", "std", "min", "max", "argmin", "argmax"):
        with pytest.raises(ValueError, match="empty"):
            getattr(e, name)()
    assert e.sum() == 0 and e.sum().dtype == np.float32
    s = fake_device((0, 3), np.complex64).sum(axis=0)
    assert s.shape == (3,) and s.dtype == np.complex64 and not s.any()
    with pytest.raises(ValueError, match="empty"):
        fake_device((0, 3), np.float64).mean(axis=0)


def test_further_refusals_come_before_the_library(no_library):
    with pytest.raises(ValueError, match="selected device"):
        oa.full((3,), 1.0, np.float64, device=5)                        # before the result is allocated
    with pytest.raises(ValueError, match="selected device"):
        +fake_device((3,), np.float64, dev=2)
    with pytest.raises(ValueError, match="selected device"):
        fake_device((3,), np.float64, dev=2).T
    with pytest.raises(IndexError, match="size 0"):
        fake_device((0, 2), np.float64)[fake_device((3,), np.int64)]    # as a host index: IndexError, not the C ABI's refusal
    with pytest.raises(IndexError, match="out of bounds"):
        fake_device((0, 2), np.float64)[[0]]
    with pytest.warns(RuntimeWarning, match="Degrees of freedom"):
        assert np.isnan(device._dof(3, 3)) and np.isnan(device._dof(3, 4))
    assert device._dof(3, 1) == 2


def test_freqshift_refusals_come_before_the_library(no_library):
    with pytest.raises(ValueError, match="1-D or"):
        oa.freqShift(np.zeros((2, 2, 2)), 1.0, 2.0)
    with pytest.raises(ValueError, match="finite"):
        oa.freqShift(np.zeros(4), np.inf, 2.0)
    with pytest.raises(ValueError, match="non-zero"):
        oa.freqShift(np.zeros(4), 1.0, 0.0)
    with pytest.raises(TypeError):
        oa.freqShift(fake_device((4,), np.int32), 1.0, 2.0)
    with pytest.raises(TypeError):
        oa.freqShift(np.array(["a"]), 1.0, 2.0)
    assert oa.freqShift(np.zeros(0), 1.0, 2.0).shape == (0,) and oa.freqShift(np.zeros((0, 2)), 1.0, 2.0).dtype == np.complex128


SCALARS = [2, -3, 2.5, 0.1, 1j, 2 - 0.1j, True, np.float32(0.1), np.float64(0.1), np.complex64(0.1 + 2j), np.complex128(0.1 - 1j), np.array(0.1),
           np.array(0.1, dtype=np.float32)]


def test_promotion_is_numpys_over_the_whole_table(no_library):
    for dt in ARITH:
        x = fake_device((4, 3), dt)
        host = np.ones((4, 3), dtype=dt)
        for dt2 in ARITH:
            for other, shape in ((fake_device((4, 3), dt2), (4, 3)), (fake_device((3,), dt2), (3,)), (fake_device((4, 1), dt2), (4, 1))):
                want = (host * np.ones(shape, dtype=dt2)).dtype
                for swap in (False, True):
                    assert device.plan_binary(x, other, swap)[4] == want, (dt, dt2, shape)
            row = np.arange(3).astype(dt2)
            plan = device.plan_binary(x, row, False)
            assert plan[4] == (host * row).dtype and plan[1].dtype == plan[4] and np.array_equal(plan[1], row.astype(plan[4]))
        for s in SCALARS:
            want = host * s
            plan = device.plan_binary(x, s, False)
            assert plan[4] == want.dtype and plan[2] == _lib.ARRAY_SCALAR and plan[1] is None, (dt, s)
            # the scalar goes in the result type, as numpy converts it before the loop
            assert plan[5] == complex(np.asarray(s).astype(want.dtype)[()])
            assert np.array_equal(want, host * want.dtype.type(plan[5] if want.dtype.kind == "c" else plan[5].real))
        assert device.plan_binary(x, [1, 2, 3], False)[4] == (host * [1, 2, 3]).dtype           # a list is an array: strong
        assert device.plan_binary(x, (1.5, 2, 3), True)[4] == (host * np.array((1.5, 2, 3))).dtype
    assert device.plan_binary(fake_device((3,), np.float32), np.int64(2), False)[4] == np.float64   # numpy's rule for a strong integer


def test_operand_shapes_are_classified_as_the_kernels_take_them():
    cb = device.classify_broadcast
    S, R, K = _lib.ARRAY_SAME, _lib.ARRAY_ROW, _lib.ARRAY_COLUMN
    assert cb((7,), (7,)) == (S, 1) and cb((7, 2), (7, 2)) == (S, 1) and cb((), ()) == (S, 1)
    assert cb((7, 2), (2,)) == (R, 2) and cb((7, 2, 3), (3,)) == (R, 3) and cb((7, 1), (1,)) == (R, 1) and cb((2, 2, 2, 5), (5,)) == (R, 5)
    assert cb((7, 2), (7, 1)) == (K, 2) and cb((7, 2, 3), (7, 1, 1)) == (K, 6) and cb((7, 1), (7, 1)) == (S, 1)
    for a, b in (((7, 2), (7,)), ((7, 2), (1, 2)), ((7, 2, 3), (7, 1)), ((7, 2, 3), (7, 2, 1)), ((7,), (1,)), ((7, 2), ()), ((2, 2, 2, 2), (2, 1, 1, 1))):
        assert cb(a, b) is None
    # the smaller operand on the left: the roles swap, and with them the operator's direction
    big, row, col = fake_device((7, 2), np.float64), fake_device((2,), np.float64), fake_device((7, 1), np.float64)
    for small, kind in ((row, R), (col, K)):
        a, b, k, inner, _, _, swap = device.plan_binary(small, big, False)
        assert a is big and b is small and k == kind and inner == 2 and swap is True
        assert device.plan_binary(small, big, True)[6] is False


def test_struct_layouts_match_header(tmp_path):
    structs = {"ssf_array_desc": _lib.ArrayDesc, "ssf_array_binary_params": _lib.ArrayBinaryParams}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    consts = ["SSF_ARRAY_MAX_DIM", "SSF_ARRAY_ADD", "SSF_ARRAY_SUB", "SSF_ARRAY_MUL", "SSF_ARRAY_DIV", "SSF_ARRAY_SAME", "SSF_ARRAY_SCALAR", "SSF_ARRAY_ROW",
              "SSF_ARRAY_COLUMN", "SSF_ARRAY_NEG", "SSF_ARRAY_CONJ", "SSF_ARRAY_REAL", "SSF_ARRAY_IMAG", "SSF_ARRAY_ABS", "SSF_ARRAY_ABS2", "SSF_ARRAY_ANGLE",
              "SSF_ARRAY_EXP", "SSF_ARRAY_SQRT", "SSF_ARRAY_CONVERT", "SSF_ARRAY_SUM", "SSF_ARRAY_SUMSQDEV", "SSF_ARRAY_MIN", "SSF_ARRAY_MAX"]
    lines += [f'printf("{c} %d\\n", (int){c});' for c in consts]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    want = dict(SSF_ARRAY_MAX_DIM=_lib.ARRAY_MAX_DIM, SSF_ARRAY_SAME=_lib.ARRAY_SAME, SSF_ARRAY_SCALAR=_lib.ARRAY_SCALAR, SSF_ARRAY_ROW=_lib.ARRAY_ROW,
                SSF_ARRAY_COLUMN=_lib.ARRAY_COLUMN, SSF_ARRAY_SUM=_lib.ARRAY_SUM, SSF_ARRAY_SUMSQDEV=_lib.ARRAY_SUMSQDEV, SSF_ARRAY_MIN=_lib.ARRAY_MIN,
                SSF_ARRAY_MAX=_lib.ARRAY_MAX)
    want.update({"SSF_ARRAY_" + k.upper(): v for k, v in _lib.ARRAY_BINARY.items()})
    want.update({"SSF_ARRAY_" + k.upper(): v for k, v in _lib.ARRAY_UNARY.items()})
    assert {k: int(got[k]) for k in consts} == want


def test_kernel_constants_match_the_binding():
    text = open(os.path.join(ROOT, "opticommpy_amd", "csrc", "array_kernels.h")).read()
    for name, val in (("kBlock", _lib.ARRAY_BLOCK), ("kMaxBlocks", _lib.ARRAY_MAX_BLOCKS), ("kRedBlocks", _lib.ARRAY_RED_BLOCKS), ("kTile", _lib.ARRAY_TILE),
                      ("kMaxDim", _lib.ARRAY_MAX_DIM)):
        assert f"constexpr int {name} = {val};" in text, name


def desc(shape, stride, offset=0, extent=64, itemsize=8):
    d = _lib.ArrayDesc(ndim=len(shape), itemsize=itemsize, offset=offset, extent=extent)
    for a, (n, s) in enumerate(zip(shape, stride)):
        d.shape[a], d.stride[a] = n, s
    return d


def test_library_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    buf, buf2 = (C.c_double * 64)(), (C.c_double * 64)()
    good = desc((4, 4), (4, 1))

    def copy(s, d, a=buf, b=buf2):
        return lib.ssf_array_copy(0, C.byref(s), a, C.byref(d), b)
    assert copy(good, good, buf, buf) == -1                                              # in place
    assert copy(good, desc((4, 4), (4, 1), itemsize=4)) == -1 and copy(good, desc((4, 4), (4, 1), itemsize=3)) == -1
    assert copy(good, desc((4, 2), (4, 1))) == -1 and copy(good, desc((16,), (1,))) == -1      # another shape, another ndim
    assert copy(desc((4, 4), (20, 1), offset=4), good) == -1                             # the last row ends at element 67 of 64
    assert copy(desc((4, 4), (-4, 1)), good) == -1 and copy(good, desc((4, 4), (4, -1))) == -1     # a negative stride from offset 0
    # ... but not from the last row: the descriptors pass, and the call ends for another reason -- no device, or, with one, these
    # host buffers (the refusal's text tells the two apart on either kind of machine)
    assert b"descriptor" in lib.ssf_last_error(None)
    copy(desc((4, 4), (-4, 1), offset=12), good)
    assert b"descriptor" not in lib.ssf_last_error(None)
    copy(desc((4, 4), (0, 1)), good)                                                     # a source may repeat its elements
    assert b"descriptor" not in lib.ssf_last_error(None)
    for d in (desc((4, 4), (0, 1)), desc((4, 4), (1, 1)), desc((4, 4), (3, 1)), desc((2, 2, 2), (4, 2, 2))):      # a destination may not
        assert copy(good if d.ndim == 2 else desc((2, 2, 2), (4, 2, 1)), d) == -1 and b"twice" in lib.ssf_last_error(None)
    assert copy(good, desc((4, 4), (1, 4))) != -1 or b"descriptor" not in lib.ssf_last_error(None)     # a transposed destination is fine
    big = 1 << 40                                                                        # spans that overflow 64 bits if multiplied there
    for d in (desc((big, 2), (big, 1)), desc((big,), (-big,), offset=3, extent=big), desc((1 << 20, 1 << 20), (1 << 39, 1 << 39), extent=big),
              desc((big,), (big - 1,), extent=big), desc((3,), (-(1 << 39),), offset=5, extent=big), desc((4, 4), (64, 1)),
              desc((4, 4), (4, 1), offset=64), desc((1 << 41, 1), (1, 1))):
        assert copy(d, good) == -1 and b"descriptor is malformed" in lib.ssf_last_error(None)
    assert copy(desc((4, 4), (4, 1), offset=-1), good) == -1 and copy(desc((4, -4), (4, 1)), good) == -1
    bad = desc((4, 4), (4, 1))
    bad.ndim = 5
    assert copy(bad, good) == -1
    assert lib.ssf_array_copy(0, None, buf, C.byref(good), buf2) == -1 and copy(good, good, None, buf2) == -1
    assert copy(desc((0, 4), (4, 1)), desc((0, 4), (4, 1))) == 0                          # nothing to move: no device needed
    idx = (C.c_int64 * 4)()
    assert lib.ssf_array_take(0, 0, 4, 1, 8, 8, idx, buf, buf2) == -1 and lib.ssf_array_take(0, 4, 4, 1, 3, 8, idx, buf, buf2) == -1
    assert lib.ssf_array_take(0, 4, 4, 1, 8, 2, idx, buf, buf2) == -1 and lib.ssf_array_take(0, 4, 4, 1, 8, 8, None, buf, buf2) == -1
    assert lib.ssf_array_take(0, 4, -1, 1, 8, 8, idx, buf, buf2) == -1 and lib.ssf_array_take(0, 4, 0, 1, 8, 8, idx, buf, buf2) == 0
    assert lib.ssf_array_transpose(0, 4, 4, 8, buf, buf) == -1 and lib.ssf_array_transpose(0, -1, 4, 8, buf, buf2) == -1
    assert lib.ssf_array_transpose(0, 4, 4, 5, buf, buf2) == -1 and lib.ssf_array_transpose(0, 0, 4, 8, buf, buf2) == 0
    assert lib.ssf_array_fill(0, 4, 8, None, buf) == -1 and lib.ssf_array_fill(0, -4, 8, buf2, buf) == -1 and lib.ssf_array_fill(0, 4, 7, buf2, buf) == -1

    def binary(**kw):
        p = _lib.ArrayBinaryParams(**dict(dict(op=0, swap=0, a_dtype=2, b_dtype=2, out_dtype=2, kind=0, count=8, inner=1), **kw))
        return lib.ssf_array_binary(0, C.byref(p), buf, buf2, (C.c_double * 64)())
    assert binary(op=4) == -1 and binary(op=-1) == -1 and binary(kind=4) == -1 and binary(swap=2) == -1 and binary(a_dtype=4) == -1
    assert binary(out_dtype=0) == -1 and binary(a_dtype=0) == -1 and binary(b_dtype=1) == -1           # complex exactly if an operand is
    assert binary(count=-1) == -1 and binary(kind=2, inner=3) == -1 and binary(kind=3, inner=0) == -1
    p = _lib.ArrayBinaryParams(op=0, a_dtype=2, b_dtype=2, out_dtype=2, kind=0, count=8, inner=1)
    assert lib.ssf_array_binary(0, C.byref(p), buf, None, buf2) == -1 and lib.ssf_array_binary(0, C.byref(p), buf, buf2, buf) == -1
    assert lib.ssf_array_binary(0, None, buf, buf2, buf2) == -1 and binary(count=0) == 0
    U = _lib.ARRAY_UNARY
    assert lib.ssf_array_unary(0, 10, 2, 2, 4, buf, buf2) == -1 and lib.ssf_array_unary(0, U["neg"], 2, 2, 4, buf, buf) == -1
    assert lib.ssf_array_unary(0, U["abs"], 0, 0, 4, buf, buf2) == -1 and lib.ssf_array_unary(0, U["neg"], 0, 2, 4, buf, buf2) == -1
    assert lib.ssf_array_unary(0, U["convert"], 0, 2, 4, buf, buf2) == -1 and lib.ssf_array_unary(0, U["sqrt"], 0, 0, 4, buf, buf2) == -6
    assert lib.ssf_array_unary(0, U["exp"], 2, 0, 4, buf, buf2) == -1 and lib.ssf_array_unary(0, U["exp"], 2, 2, 0, buf, buf2) == 0
    arg = (C.c_int64 * 4)()
    assert lib.ssf_array_reduce(0, 4, 2, 4, 1, None, buf, buf2, arg) == -1 and lib.ssf_array_reduce(0, 0, 2, 0, 1, None, buf, buf2, arg) == -1
    assert lib.ssf_array_reduce(0, _lib.ARRAY_SUMSQDEV, 2, 4, 1, None, buf, buf2, arg) == -1                  # no centre
    assert lib.ssf_array_reduce(0, _lib.ARRAY_MIN, 0, 4, 1, None, buf, buf2, arg) == -1                       # complex
    assert lib.ssf_array_reduce(0, _lib.ARRAY_MAX, 2, 4, 1, None, buf, buf2, None) == -1 and lib.ssf_array_reduce(0, 0, 2, 4, 70000, None, buf, buf2, arg) == -1
    assert lib.ssf_freq_shift(0, 4, 1, 0, 1.0, 0.0, buf, buf2) == -1 and lib.ssf_freq_shift(0, 4, 1, 0, float("nan"), 1.0, buf, buf2) == -1
    assert lib.ssf_freq_shift(0, 4, 0, 0, 1.0, 1.0, buf, buf2) == -1 and lib.ssf_freq_shift(0, 4, 1, 7, 1.0, 1.0, buf, buf2) == -1
    assert lib.ssf_freq_shift(0, 4, 1, 0, 1.0, 1.0, buf, buf) == -1 and lib.ssf_freq_shift(0, 0, 1, 0, 1.0, 1.0, buf, buf2) == 0
