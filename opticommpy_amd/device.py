"""Device-resident arrays: chain channel -> receiver -> DSP calls without crossing PCIe.

The reference's cupy twin converts back to numpy at every function boundary (``cp.asnumpy``,
optic/models/modelsGPU.py:271, 501-509; optic/dsp/coreGPU.py:72).  Here a field may stay in HBM
between calls:

    Ed = oa.to_device(E)                     # one upload
    Ed = oa.manakovSSF(Ed, paramCh)          # DeviceArray in -> DeviceArray out
    Sd = oa.pdmCoherentReceiver(Ed, Elo, paramFE, paramPD)
    Sd = oa.edc(Sd, paramEDC)
    S = oa.decimate(Sd, paramDec).get()      # one download

A DeviceArray is a typed, C-contiguous block of device memory (``ssf_device_malloc``); the C ABI
recognises device pointers wherever it takes array arguments (include/ssf.h), so the same entry
points serve both kinds of caller.  Functions return a DeviceArray when their main input is one."""
import ctypes as C
import math
import operator
import threading
import warnings

import numpy as np

from . import _lib


# Freed blocks are kept (by device and size) and handed out again: hipMalloc / hipFree of tens of MiB cost
# hundreds of microseconds and hipFree synchronises the device.  Capped; release_pool() returns everything.
_POOL = {}
_POOL_BYTES = [0]
_POOL_CAP = 4 << 30
_POOL_LOCK = threading.Lock()


# Transfers between host and device memory made through DeviceArray.set / .get (tests count them: a chain of calls on
# DeviceArrays must not go through the host in between, tests/test_chain.py, tests/test_gpu_device_arrays.py)
_COUNTS = {"h2d": 0, "d2h": 0, "h2d_bytes": 0, "d2h_bytes": 0}


def transfer_counts():
    """Copy of the counters of DeviceArray.set (h2d) / .get (d2h) calls and bytes since the package was imported."""
    return dict(_COUNTS)


def release_pool():
    """Give the cached device blocks back to the driver."""
    lib = _lib.load()
    with _POOL_LOCK:
        for (dev, _), ptrs in _POOL.items():
            for p in ptrs:
                lib.ssf_device_free(dev, p)
        _POOL.clear()
        _POOL_BYTES[0] = 0


class DeviceArray:
    """C-contiguous ndarray-like block of HBM on one GPU.  ``get()`` / ``np.asarray`` download it."""

    def __init__(self, shape, dtype, device=None):
        from .models import _state
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.device = _state["device"] if device is None else int(device)
        self._ptr = C.c_void_p()
        self._alloc = max(self.nbytes, 1)
        with _POOL_LOCK:
            cached = _POOL.get((self.device, self._alloc))
            if cached:
                self._ptr = cached.pop()
                _POOL_BYTES[0] -= self._alloc
                return
        lib = _lib.load()
        rc = lib.ssf_device_malloc(self.device, self._alloc, C.byref(self._ptr))
        if rc == -3 and _POOL:                      # out of memory: drop the cache and retry once
            release_pool()
            rc = lib.ssf_device_malloc(self.device, self._alloc, C.byref(self._ptr))
        _lib.raise_for(lib, None, rc)

    # ---- ndarray-like surface
    @property
    def size(self):
        return math.prod(self.shape)                 # (np.prod costs microseconds per call: several per receiver-side call)

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def ndim(self):
        return len(self.shape)

    def __len__(self):
        return self.shape[0]

    @property
    def ptr(self):
        return self._ptr

    def reshape(self, *shape):
        """Same memory, another C-contiguous shape (a view: keeps the owner alive)."""
        shape = shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
        known = math.prod(int(s) for s in shape if s != -1)
        shape = tuple(self.size // known if s == -1 else int(s) for s in shape)
        if math.prod(shape) != self.size:
            raise ValueError(f"cannot reshape array of size {self.size} into shape {shape}")
        v = object.__new__(DeviceArray)
        v.shape, v.dtype, v.device, v._ptr, v._owner = shape, self.dtype, self.device, self._ptr, self
        return v

    # ---- transfers
    def set(self, x):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        if x.shape != self.shape:
            raise ValueError(f"shape mismatch: {x.shape} vs {self.shape}")
        if self.nbytes:                              # (an empty array has nothing to move, and numpy may hand out no address for it)
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_device_memcpy(self.device, self._ptr, x.ctypes.data_as(C.c_void_p), self.nbytes))
        _COUNTS["h2d"] += 1
        _COUNTS["h2d_bytes"] += self.nbytes
        return self

    def get(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_device_memcpy(self.device, out.ctypes.data_as(C.c_void_p), self._ptr, self.nbytes))
        _COUNTS["d2h"] += 1
        _COUNTS["d2h_bytes"] += self.nbytes
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.get()
        return a if dtype is None else a.astype(dtype)

    def copy(self):
        out = DeviceArray(self.shape, self.dtype, self.device)
        if self.nbytes:
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_device_memcpy(self.device, out._ptr, self._ptr, self.nbytes))
        return out

    # ---- the array layer (engine_array.hip): what a notebook writes between two stages.  Every result is a fresh C-contiguous
    # allocation (no views: kernels across the package assume allocation alignment), nothing writes its operands, a result of
    # zero elements is returned without a launch, and nothing crosses to the host except the few values of a reduction.
    __array_priority__ = 1000          # ndarray o d and np.float64 o d reach the reflected method instead of downloading d

    def __getitem__(self, key):
        """Basic indexing for ndim <= 4: integers, slices, Ellipsis and tuples of these, or one 1-D integer index sequence (list,
        numpy array, int32 / int64 DeviceArray) in first position.  A copy, never a view.  A host index out of range raises
        IndexError; the entries of a device index wrap if negative and are then CLAMPED to the first or last row by the kernel."""
        axes, index = normalize_key(self.shape, key)
        _movable(self)
        if isinstance(index, DeviceArray):
            _on_selected_device(self, index)
        else:
            _on_selected_device(self)
        if index is not None and len(index) and self.shape[0] == 0:      # (a host index was refused by normalize_key already)
            raise IndexError("an index into axis 0 with size 0 is out of bounds")
        src = self
        if any((start, count, step) != (0, n, 1) for (start, count, step, _), n in zip(axes, self.shape)) or index is None:
            src = _strided_gather(self, axes, drop=index is None)
        if index is None:
            return src
        kept = tuple(c for _, c, _, keep in axes[1:] if keep)
        out = DeviceArray((len(index),) + kept, self.dtype, self.device)
        inner = math.prod(kept)
        if out.size:
            lib = _lib.load()
            ip, _keep = (index.ptr, index) if isinstance(index, DeviceArray) else (index.ctypes.data_as(C.c_void_p), index)
            _lib.raise_for(lib, None, lib.ssf_array_take(self.device, self.shape[0], len(index), inner, self.dtype.itemsize,
                                                         index.dtype.itemsize, ip, src.ptr, out.ptr))
        return out

    @property
    def T(self):
        return self.transpose()

    def transpose(self):
        """The transpose of a 2-D array (through a padded LDS tile); of a 0-D or 1-D array, a copy."""
        if self.ndim > 2:
            raise ValueError(f"transpose supports ndim <= 2, this array has {self.ndim} dimensions")
        _movable(self)
        _on_selected_device(self)
        if self.ndim < 2:
            return self.copy()
        out = DeviceArray(self.shape[::-1], self.dtype, self.device)
        if out.size:
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_array_transpose(self.device, self.shape[0], self.shape[1], self.dtype.itemsize, self.ptr, out.ptr))
        return out

    def _binary(self, other, op, swap):
        plan = plan_binary(self, other, swap)
        if plan is NotImplemented:
            return plan
        a, b, kind, inner, out_dtype, scalar, swap = plan
        _on_selected_device(*(x for x in (a, b) if isinstance(x, DeviceArray)))
        out = DeviceArray(a.shape, out_dtype, a.device)
        if out.size:
            p = _lib.ArrayBinaryParams(op=_lib.ARRAY_BINARY[op], swap=int(swap), a_dtype=_lib.METRICS_DTYPES[a.dtype.name],
                                       b_dtype=_lib.METRICS_DTYPES[(out_dtype if b is None else b.dtype).name],
                                       out_dtype=_lib.METRICS_DTYPES[out_dtype.name], kind=kind, count=a.size, inner=inner,
                                       scalar_re=scalar.real, scalar_im=scalar.imag)
            bp = None if b is None else out_ptr(b)
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_array_binary(a.device, C.byref(p), a.ptr, bp, out.ptr))
        return out

    def __add__(self, other):
        return self._binary(other, "add", False)

    def __radd__(self, other):
        return self._binary(other, "add", True)

    def __sub__(self, other):
        return self._binary(other, "sub", False)

    def __rsub__(self, other):
        return self._binary(other, "sub", True)

    def __mul__(self, other):
        return self._binary(other, "mul", False)

    def __rmul__(self, other):
        return self._binary(other, "mul", True)

    def __truediv__(self, other):
        return self._binary(other, "div", False)

    def __rtruediv__(self, other):
        return self._binary(other, "div", True)

    def __pow__(self, p):
        if type(p) is not int or p != 2:
            raise TypeError("** is supported with the Python integer 2 only (x ** 2 is x * x, as numpy's square)")
        return self._binary(self, "mul", False)

    def __neg__(self):
        return self._unary("neg", self.dtype)

    def __pos__(self):
        _arithmetic(self)
        _on_selected_device(self)
        return self.copy()

    def __abs__(self):
        return self.abs()

    def _unary(self, op, out_dtype):
        _arithmetic(self)
        _on_selected_device(self)
        out = DeviceArray(self.shape, out_dtype, self.device)
        if out.size:
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_array_unary(self.device, _lib.ARRAY_UNARY[op], _lib.METRICS_DTYPES[self.dtype.name],
                                                          _lib.METRICS_DTYPES[out.dtype.name], self.size, self.ptr, out.ptr))
        return out

    def conj(self):
        return self._unary("conj", self.dtype)

    @property
    def real(self):
        """The real parts (of a real array: a copy)."""
        return self._unary("real", _real_dtype(self.dtype))

    @property
    def imag(self):
        """The imaginary parts (of a real array: zeros)."""
        return self._unary("imag", _real_dtype(self.dtype))

    def abs(self):
        """|x|: of a complex value by hypot, finite wherever the true value is."""
        return self._unary("abs", _real_dtype(self.dtype))

    def abs2(self):
        """re^2 + im^2: np.abs(x) ** 2 without the square root."""
        return self._unary("abs2", _real_dtype(self.dtype))

    def angle(self):
        return self._unary("angle", _real_dtype(self.dtype))

    def exp(self):
        return self._unary("exp", self.dtype)

    def sqrt(self):
        """Square root of a real array (a negative value gives NaN, as numpy)."""
        _arithmetic(self)
        if self.dtype.kind == "c":
            raise TypeError("sqrt is for real arrays (float32, float64)")
        return self._unary("sqrt", self.dtype)

    def astype(self, dtype):
        """Conversion among float32, float64, complex64 and complex128 (to the same dtype: a copy)."""
        _arithmetic(self)
        dtype = np.dtype(dtype)
        if dtype.name not in _ARITH:
            raise TypeError(f"astype converts among {', '.join(_ARITH)}, not to {dtype.name}")
        if self.dtype.kind == "c" and dtype.kind != "c":
            raise TypeError("astype from complex to real would drop the imaginary parts: take .real (or .imag, .abs()) first")
        return self._unary("convert", dtype)

    def _reduce(self, op, axis, need_values=True, real_only=False):
        """-> (out, arg, cols, rows): per column the engine's doubles and (min / max) indices; out is None for an empty array."""
        _arithmetic(self)
        if real_only and self.dtype.kind == "c":
            raise TypeError("min, max, argmin and argmax are for real arrays (float32, float64)")
        if axis not in (None, 0):
            raise ValueError("reductions support axis=None and axis=0")
        if axis == 0 and not 1 <= self.ndim <= 2:
            raise ValueError(f"axis=0 is supported for 1-D and 2-D arrays, this array has {self.ndim} dimensions")
        rows, cols = (self.size, 1) if axis is None else (self.shape[0], math.prod(self.shape[1:]))
        if rows == 0 and need_values:
            raise ValueError("this reduction of an empty array has no value")
        if rows == 0 or cols == 0:
            return None, None, cols, rows
        _on_selected_device(self)
        out, arg = (C.c_double * (2 * cols))(), (C.c_int64 * cols)()
        center = None
        if op == _lib.ARRAY_SUMSQDEV:
            s, _, _, _ = self._reduce(_lib.ARRAY_SUM, axis)
            center = (C.c_double * (2 * cols))(*(v / rows for v in s))
        lib = _lib.load()
        _lib.raise_for(lib, None, lib.ssf_array_reduce(self.device, op, _lib.METRICS_DTYPES[self.dtype.name], rows, cols, center, self.ptr, out, arg))
        return out, arg, cols, rows

    def _shaped(self, values, axis, dtype):
        a = np.asarray(values).astype(dtype)
        return a.reshape(())[()] if axis is None or self.ndim == 1 else a.reshape(self.shape[1:])

    def _sums(self, out, cols):
        v = np.frombuffer(out, dtype=np.float64).reshape(cols, 2)
        if self.dtype.kind != "c":
            return v[:, 0].copy()
        z = np.empty(cols, dtype=np.complex128)          # (re + 1j im would turn an infinite imaginary sum into a NaN real part)
        z.real, z.imag = v[:, 0], v[:, 1]
        return z

    def sum(self, axis=None):
        """Sum over the whole array (a numpy scalar) or over axis 0 of a 1-D or 2-D array (a numpy array of shape[1:]).  Accumulated
        in double whatever the dtype, partial sums added in a fixed order; rounded to numpy's result dtype at the end."""
        out, _, cols, _ = self._reduce(_lib.ARRAY_SUM, axis, need_values=False)
        return self._shaped(np.zeros(cols) if out is None else self._sums(out, cols), axis, self.dtype)

    def mean(self, axis=None):
        out, _, cols, rows = self._reduce(_lib.ARRAY_SUM, axis)
        return self._shaped(np.zeros(0) if out is None else self._sums(out, cols) / rows, axis, self.dtype)

    def var(self, axis=None, ddof=0):
        """Two passes, as numpy: the mean, then the sum of |x - mean|^2 over rows - ddof.  With ddof >= rows the result is NaN and
        a RuntimeWarning is given, as numpy does."""
        out, _, cols, rows = self._reduce(_lib.ARRAY_SUMSQDEV, axis)
        v = np.zeros(0) if out is None else np.frombuffer(out, dtype=np.float64).reshape(cols, 2)[:, 0] / _dof(rows, ddof)
        return self._shaped(v, axis, _real_dtype(self.dtype))

    def std(self, axis=None, ddof=0):
        out, _, cols, rows = self._reduce(_lib.ARRAY_SUMSQDEV, axis)
        v = np.zeros(0) if out is None else np.sqrt(np.frombuffer(out, dtype=np.float64).reshape(cols, 2)[:, 0] / _dof(rows, ddof))
        return self._shaped(v, axis, _real_dtype(self.dtype))

    def _extreme(self, op, axis, want_arg):
        out, arg, cols, _ = self._reduce(op, axis, real_only=True)
        if out is None:
            return self._shaped(np.zeros(0), axis, np.int64 if want_arg else self.dtype)
        if want_arg:
            return self._shaped(np.frombuffer(arg, dtype=np.int64), axis, np.int64)
        return self._shaped(np.frombuffer(out, dtype=np.float64)[:cols], axis, self.dtype)

    def min(self, axis=None):
        """numpy's rule: a NaN wins."""
        return self._extreme(_lib.ARRAY_MIN, axis, False)

    def max(self, axis=None):
        return self._extreme(_lib.ARRAY_MAX, axis, False)

    def argmin(self, axis=None):
        """numpy's rule: the lowest index among equals, the first NaN's if there is one."""
        return self._extreme(_lib.ARRAY_MIN, axis, True)

    def argmax(self, axis=None):
        return self._extreme(_lib.ARRAY_MAX, axis, True)

    def __del__(self):
        if getattr(self, "_owner", None) is None and getattr(self, "_ptr", None):
            try:
                with _POOL_LOCK:
                    keep = _POOL_BYTES[0] + self._alloc <= _POOL_CAP
                    if keep:
                        _POOL.setdefault((self.device, self._alloc), []).append(self._ptr)
                        _POOL_BYTES[0] += self._alloc
                if not keep:
                    _lib.load().ssf_device_free(self.device, self._ptr)
            except Exception:
                pass

    def __repr__(self):
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype.name}, device={self.device})"


# ---- the array layer's host side: everything here is decided before the library is loaded
_ARITH = ("float32", "float64", "complex64", "complex128")
_ITEMSIZES = (1, 2, 4, 8, 16)
_MAX_DIM = _lib.ARRAY_MAX_DIM
_ROW_MAX = 4096            # values of a host row operand: beyond it the operand is an array to upload, not a handful of coefficients
_INDEXING = ("supported: integers, slices, Ellipsis and tuples of these, or one 1-D integer index sequence (list, numpy array, "
             "int32 / int64 DeviceArray) in first position")


def _dof(rows, ddof):
    """The divisor of var and std; numpy's answer to none left: a RuntimeWarning and NaN."""
    if rows - ddof <= 0:
        warnings.warn("Degrees of freedom <= 0 for slice", RuntimeWarning, stacklevel=3)
        return float("nan")
    return rows - ddof


def _real_dtype(dtype):
    return np.dtype({"complex64": np.float32, "complex128": np.float64}.get(dtype.name, dtype))


def _arithmetic(x):
    if x.dtype.name not in _ARITH:
        raise TypeError(f"arithmetic, conversion and reductions are for {', '.join(_ARITH)}; this array is {x.dtype.name}")


def _movable(x):
    if x.dtype.itemsize not in _ITEMSIZES:
        raise TypeError(f"indexing, transposes and concatenation move items of 1, 2, 4, 8 or 16 bytes; {x.dtype.name} has {x.dtype.itemsize}")


def _on_selected_device(*arrays):
    from .models import _state
    for x in arrays:
        if x.device != arrays[0].device:
            raise ValueError(f"operands live on different GPUs ({arrays[0].device} and {x.device})")
        if x.device != _state["device"]:
            raise ValueError(f"device array lives on GPU {x.device}, the selected device is {_state['device']} (set_device)")


def _c_strides(shape):
    s, acc = [], 1
    for n in reversed(shape):
        s.append(acc)
        acc *= n
    return tuple(reversed(s))


def _is_index_sequence(k):
    return isinstance(k, (list, np.ndarray, DeviceArray))


def normalize_key(shape, key):
    """An indexing key against `shape` -> (axes, index): per axis of the array (start, count, step, keep) -- the elements
    start, start + step, .. (count of them), and whether the axis stays in the result (an integer drops it) -- and the 1-D index
    sequence of axis 0 (an int64 numpy array with negative entries wrapped, or the int32 / int64 DeviceArray) or None.  The rules are
    numpy's for basic indexing; everything else raises IndexError or TypeError naming what is supported."""
    if len(shape) > _MAX_DIM:
        raise IndexError(f"indexing supports ndim <= {_MAX_DIM}, this array has {len(shape)} dimensions")
    key = key if isinstance(key, tuple) else (key,)
    for k in key:
        if k is None:
            raise IndexError("None (np.newaxis) is not supported: reshape instead; " + _INDEXING)
        if isinstance(k, (bool, np.bool_)) or (isinstance(k, (np.ndarray, DeviceArray)) and k.dtype.kind == "b") or \
                (isinstance(k, list) and any(isinstance(v, (bool, np.bool_)) for v in k)):
            raise IndexError("boolean masks are not supported; " + _INDEXING)
    if sum(_is_index_sequence(k) for k in key) > 1:
        raise IndexError("more than one index array is not supported; " + _INDEXING)
    if any(_is_index_sequence(k) for k in key[1:]):
        raise IndexError("an index array is supported in first position only; " + _INDEXING)
    if sum(k is Ellipsis for k in key) > 1:
        raise IndexError("an index can only have a single ellipsis ('...')")
    if Ellipsis in [k for k in key if not _is_index_sequence(k)]:
        at = next(i for i, k in enumerate(key) if k is Ellipsis)
        fill = len(shape) - (len(key) - 1)
        if fill < 0:
            raise IndexError(f"too many indices for array: array is {len(shape)}-dimensional, but {len(key) - 1} were indexed")
        key = key[:at] + (slice(None),) * fill + key[at + 1:]
    if len(key) > len(shape):
        raise IndexError(f"too many indices for array: array is {len(shape)}-dimensional, but {len(key)} were indexed")
    key = key + (slice(None),) * (len(shape) - len(key))
    axes, index = [], None
    for ax, (k, n) in enumerate(zip(key, shape)):
        if _is_index_sequence(k):
            index = _index_sequence(k, n)
            axes.append((0, n, 1, True))
        elif isinstance(k, slice):
            start, stop, step = k.indices(n)                        # (a zero step: ValueError, as numpy)
            axes.append((start, len(range(start, stop, step)), step, True))
        else:
            try:
                i = operator.index(k)
            except TypeError:
                raise IndexError(f"{type(k).__name__} is not a valid index; " + _INDEXING) from None
            if not -n <= i < n:
                raise IndexError(f"index {i} is out of bounds for axis {ax} with size {n}")
            axes.append((i + n if i < 0 else i, 1, 1, False))
    return axes, index


def _index_sequence(k, n):
    if isinstance(k, DeviceArray):
        if k.dtype.name not in ("int32", "int64") or k.ndim != 1:
            raise IndexError("a device index is a 1-D int32 or int64 DeviceArray; " + _INDEXING)
        return k
    a = np.asarray(k)
    if a.size == 0 and a.ndim == 1:
        a = a.astype(np.int64)
    if a.dtype.kind not in "iu" or a.ndim != 1:
        raise IndexError("an index sequence is 1-D and of integers; " + _INDEXING)
    a = a.astype(np.int64)
    if a.size and (a.min() < -n or a.max() >= n):
        bad = a[(a < -n) | (a >= n)][0]
        raise IndexError(f"index {bad} is out of bounds for axis 0 with size {n}")
    return np.ascontiguousarray(np.where(a < 0, a + n, a))


def _desc(shape, strides, offset, itemsize, extent):
    d = _lib.ArrayDesc(ndim=len(shape), itemsize=itemsize, offset=offset, extent=extent)
    for a, (n, s) in enumerate(zip(shape, strides)):
        d.shape[a], d.stride[a] = n, s
    return d


def _strided_gather(x, axes, drop=True):
    """The elements `axes` (normalize_key) selects of x, as a new array; drop: leave out the axes an integer indexed."""
    _movable(x)
    counts = tuple(c for _, c, _, _ in axes)
    out = DeviceArray(tuple(c for _, c, _, keep in axes if keep or not drop), x.dtype, x.device)
    if out.size:
        st = _c_strides(x.shape)
        src = _desc(counts, [s * step for s, (_, _, step, _) in zip(st, axes)], sum(s * start for s, (start, _, _, _) in zip(st, axes)),
                    x.dtype.itemsize, x.size)
        dst = _desc(counts, _c_strides(counts), 0, x.dtype.itemsize, out.size)
        lib = _lib.load()
        _lib.raise_for(lib, None, lib.ssf_array_copy(x.device, C.byref(src), x.ptr, C.byref(dst), out.ptr))
    return out


def classify_broadcast(shape, other):
    """How an operand of shape `other` meets an array of `shape`: (kind, inner) with kind one of _lib.ARRAY_SAME, ARRAY_ROW (varying
    along the last axis only: inner its length), ARRAY_COLUMN ((n, 1) against (n, m), (n, 1, 1) against 3-D: inner the elements per
    value), or None where the pair is not one of these."""
    shape, other = tuple(shape), tuple(other)
    if shape == other:
        return _lib.ARRAY_SAME, 1
    if len(shape) >= 1 and other == (shape[-1],):
        return _lib.ARRAY_ROW, shape[-1]
    if len(shape) in (2, 3) and other == (shape[0],) + (1,) * (len(shape) - 1):
        return _lib.ARRAY_COLUMN, math.prod(shape[1:])
    return None


def promote(dtype, other):
    """numpy's result dtype of an operation between an array of `dtype` and `other` (a dtype, a numpy scalar or array: strong; a
    Python scalar: weak); TypeError if it is not one of the four arithmetic types."""
    r = np.result_type(dtype, other)
    if r.name not in _ARITH:
        raise TypeError(f"the result type {r.name} is not supported: arithmetic is for {', '.join(_ARITH)}")
    return r


def plan_binary(x, other, swap):
    """What `x o other` launches: (a, b, kind, inner, out_dtype, scalar, swap) with a the array that gives the result its shape, b
    the other array (a DeviceArray, a host row already in the result dtype, or None for a scalar).  Raises before anything is loaded."""
    _arithmetic(x)
    if isinstance(other, DeviceArray):
        _arithmetic(other)
        out_dtype = promote(x.dtype, other.dtype)
        c = classify_broadcast(x.shape, other.shape)
        if c is not None:
            return x, other, c[0], c[1], out_dtype, 0j, swap
        c = classify_broadcast(other.shape, x.shape)
        if c is not None:
            return other, x, c[0], c[1], out_dtype, 0j, not swap
        raise ValueError(f"operands of shapes {x.shape} and {other.shape} do not combine: the second operand has the same shape, is a "
                         "row along the last axis, a column (n, 1) / (n, 1, 1), or a scalar")
    if isinstance(other, (bool, int, float, complex, np.generic)) or (isinstance(other, np.ndarray) and other.ndim == 0):
        if isinstance(other, np.ndarray):
            other = other[()]
        out_dtype = promote(x.dtype, other)
        s = complex(np.asarray(other).astype(out_dtype)[()])         # the scalar in the result type, as numpy converts it
        return x, None, _lib.ARRAY_SCALAR, 1, out_dtype, s, swap
    if isinstance(other, (list, tuple, np.ndarray)):
        row = np.asarray(other)
        if row.dtype.kind not in "biufc":
            raise TypeError(f"an operand of dtype {row.dtype} is not supported")
        if row.ndim != 1 or x.ndim < 1 or row.shape[0] != x.shape[-1] or row.size > _ROW_MAX:
            raise TypeError(f"a host array of shape {row.shape} beside a DeviceArray of shape {x.shape}: only a row of shape[-1] <= "
                            f"{_ROW_MAX} values is taken from the host; to_device it (there are no hidden uploads)")
        out_dtype = promote(x.dtype, row.dtype)
        return x, np.ascontiguousarray(row.astype(out_dtype)), _lib.ARRAY_ROW, x.shape[-1], out_dtype, 0j, swap
    return NotImplemented


def concatenate(arrays, axis=0):
    """np.concatenate of DeviceArrays of one dtype (ndim <= 4, any valid axis): a new array, one strided copy per operand."""
    arrays = list(arrays)
    if not arrays or not all(isinstance(a, DeviceArray) for a in arrays):
        raise TypeError("concatenate takes a non-empty sequence of DeviceArrays (to_device a host array first: no hidden uploads)")
    first = arrays[0]
    nd = first.ndim
    if nd == 0 or nd > _MAX_DIM:
        raise ValueError(f"concatenate supports 1 <= ndim <= {_MAX_DIM}")
    if not -nd <= axis < nd:
        raise ValueError(f"axis {axis} is out of bounds for arrays of dimension {nd}")
    axis %= nd
    for a in arrays:
        if a.dtype != first.dtype:
            raise TypeError(f"concatenate needs one dtype, got {first.dtype.name} and {a.dtype.name} (astype is the explicit conversion)")
        if a.ndim != nd or a.shape[:axis] != first.shape[:axis] or a.shape[axis + 1:] != first.shape[axis + 1:]:
            raise ValueError(f"all the input array dimensions except for the concatenation axis must match: {first.shape} and {a.shape}")
    _movable(first)
    _on_selected_device(*arrays)
    shape = first.shape[:axis] + (sum(a.shape[axis] for a in arrays),) + first.shape[axis + 1:]
    out = DeviceArray(shape, first.dtype, first.device)
    st, at = _c_strides(shape), 0
    for a in arrays:
        if a.size:
            src = _desc(a.shape, _c_strides(a.shape), 0, a.dtype.itemsize, a.size)
            dst = _desc(a.shape, st, at * st[axis], a.dtype.itemsize, out.size)
            lib = _lib.load()
            _lib.raise_for(lib, None, lib.ssf_array_copy(first.device, C.byref(src), a.ptr, C.byref(dst), out.ptr))
        at += a.shape[axis]
    return out


def stack(arrays, axis=0):
    """np.stack of DeviceArrays of one shape along a new first (axis=0) or last (axis=-1) axis."""
    arrays = list(arrays)
    if not arrays or not all(isinstance(a, DeviceArray) for a in arrays):
        raise TypeError("stack takes a non-empty sequence of DeviceArrays (to_device a host array first: no hidden uploads)")
    if axis not in (0, -1):
        raise ValueError("stack supports axis=0 and axis=-1")
    if any(a.shape != arrays[0].shape for a in arrays):
        raise ValueError("all input arrays must have the same shape")
    if arrays[0].ndim >= _MAX_DIM:
        raise ValueError(f"stack supports results of ndim <= {_MAX_DIM}")
    if axis == 0:
        return concatenate([a.reshape((1,) + a.shape) for a in arrays], 0)
    return concatenate([a.reshape(a.shape + (1,)) for a in arrays], -1)


def full(shape, value, dtype, device=None):
    """A new DeviceArray with every element `value` (any dtype of 1, 2, 4, 8 or 16 bytes)."""
    dtype = np.dtype(dtype)
    if dtype.itemsize not in _ITEMSIZES:
        raise TypeError(f"full fills items of 1, 2, 4, 8 or 16 bytes; {dtype.name} has {dtype.itemsize}")
    v = np.asarray(value).astype(dtype).reshape(1)
    from .models import _state
    if device is not None and int(device) != _state["device"]:
        raise ValueError(f"device {int(device)} was asked for, the selected device is {_state['device']} (set_device)")
    out = DeviceArray(shape, dtype, device)
    if out.size:
        lib = _lib.load()
        _lib.raise_for(lib, None, lib.ssf_array_fill(out.device, out.size, dtype.itemsize, v.ctypes.data_as(C.c_void_p), out.ptr))
    return out


def zeros(shape, dtype=np.float64, device=None):
    return full(shape, 0, dtype, device)


def freqShift(x, deltaF, Fs):
    """Frequency shift of a signal (optic/dsp/core.py:1050-1072): x exp(1j 2 pi deltaF t) with t = arange(len(x)) (1 / Fs), the phasor
    formed in the kernel from the sample index.  x: 1-D or (n, m), a numpy array or a DeviceArray of float32, float64, complex64 or
    complex128 (each column of (n, m) is shifted; the reference's own broadcasting only allows 1-D); returns complex128 of the
    same kind as x."""
    dev = isinstance(x, DeviceArray)
    if not dev:
        x = np.asarray(x)
        if x.dtype.kind not in "biufc":
            raise TypeError(f"freqShift of dtype {x.dtype} is not supported")
        if x.dtype.name not in _ARITH:
            x = x.astype(np.float64)
        x = np.ascontiguousarray(x)
    else:
        _arithmetic(x)
        _on_selected_device(x)
    if x.ndim not in (1, 2):
        raise ValueError("freqShift takes a 1-D or (n, m) signal")
    deltaF, Fs = float(deltaF), float(Fs)
    if not (math.isfinite(deltaF) and math.isfinite(Fs)) or Fs == 0:
        raise ValueError("freqShift needs a finite deltaF and a finite, non-zero Fs")
    from .models import _state
    out = empty(dev, x.shape, np.complex128, x.device if dev else None)
    if math.prod(x.shape):
        lib = _lib.load()
        xp = x.ptr if dev else x.ctypes.data_as(C.c_void_p)
        _lib.raise_for(lib, None, lib.ssf_freq_shift(_state["device"], x.shape[0], math.prod(x.shape[1:]), _lib.METRICS_DTYPES[x.dtype.name],
                                                     deltaF, Fs, xp, out_ptr(out)))
    return out


def to_device(x, device=None):
    """Upload a numpy array (made C-contiguous) and return the DeviceArray."""
    x = np.ascontiguousarray(x)
    return DeviceArray(x.shape, x.dtype, device).set(x)


def is_device(x):
    return isinstance(x, DeviceArray)


def arg(x, dtype):
    """(pointer, keepalive) of an array argument of the C ABI: numpy arrays are made contiguous in
    ``dtype``; a DeviceArray must already have it (converting would be a hidden device round trip)."""
    if isinstance(x, DeviceArray):
        from .models import _state
        if x.dtype != np.dtype(dtype):
            raise TypeError(f"device array has dtype {x.dtype.name}, this call needs {np.dtype(dtype).name}")
        if x.device != _state["device"]:
            raise ValueError(f"device array lives on GPU {x.device}, the selected device is {_state['device']} (set_device)")
        return x.ptr, x
    a = np.ascontiguousarray(x, dtype=dtype)
    return a.ctypes.data_as(C.c_void_p), a


def empty(like_device, shape, dtype, device=None):
    """Output buffer of the kind the caller works with."""
    return DeviceArray(shape, dtype, device) if like_device else np.empty(shape, dtype=dtype)


def out_ptr(x):
    return x.ptr if isinstance(x, DeviceArray) else x.ctypes.data_as(C.c_void_p)
