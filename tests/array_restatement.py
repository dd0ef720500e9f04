"""Restatement of the array layer of DeviceArray (opticommpy_amd/device.py, engine_array.hip) for the tests: the index
normalisation -- the package's own pure-Python function, held to numpy exhaustively in tests/test_array_host.py -- turned back into
numpy indexing, and every arithmetic operation and reduction evaluated in extended precision (np.longdouble: 64 bits of mantissa
against the 53 and 24 of the types under test), with the terms the derived error bounds are written in.  numpy is the definition of
these operations; nothing here comes from the reference except the order of operations of freqShift."""
import numpy as np

from opticommpy_amd.device import normalize_key  # noqa: F401

LD, CLD = np.longdouble, np.clongdouble
U = {"float64": 2.0 ** -53, "complex128": 2.0 ** -53, "float32": 2.0 ** -24, "complex64": 2.0 ** -24}
REAL_OF = {"complex64": np.float32, "complex128": np.float64, "float32": np.float32, "float64": np.float64}


def apply_normalized(x, key):
    """x[key] rebuilt from normalize_key's (start, count, step, keep) per axis and index sequence: what the kernels are handed."""
    axes, index = normalize_key(x.shape, key)
    out = x
    for ax, (start, count, step, keep) in enumerate(axes):
        idx = start + step * np.arange(count)
        out = np.take(out, idx, axis=ax)
    if index is not None:
        out = np.take(out, np.asarray(index), axis=0)
    kept = [c for _, c, _, keep in axes if keep]
    if index is not None:
        kept[0] = len(index)                  # (the axis an index sequence takes is whole and stays)
    return out.reshape(kept)


def widen(x):
    x = np.asarray(x)
    return x.astype(CLD) if x.dtype.kind == "c" else x.astype(LD)


def binary(op, a, b):
    """a op b in extended precision (the operands as given: a caller rounds a scalar to the result type first, as numpy does)."""
    a, b = widen(a), widen(b)
    return {"add": a + b, "sub": a - b, "mul": a * b, "div": a / b}[op]


def product_terms(a, b):
    """|p1| + |p2| per component of a complex product: (|ar br| + |ai bi|, |ar bi| + |ai br|)."""
    a, b = widen(a).astype(CLD), widen(b).astype(CLD)
    return np.abs(a.real * b.real) + np.abs(a.imag * b.imag), np.abs(a.real * b.imag) + np.abs(a.imag * b.real)


def unary(op, x):
    x = widen(x)
    c = x.dtype.kind == "c"
    if op == "abs":
        return np.hypot(x.real, x.imag) if c else np.abs(x)
    if op == "abs2":
        return x.real * x.real + x.imag * x.imag if c else x * x
    if op == "angle":
        return np.arctan2(x.imag, x.real) if c else np.arctan2(np.zeros_like(x), x)
    if op == "exp":
        return np.exp(x.real) * (np.cos(x.imag) + 1j * np.sin(x.imag)) if c else np.exp(x)
    if op == "sqrt":
        return np.sqrt(x)
    raise KeyError(op)


def total(x, axis=None):
    """(sum, sum of |x_i|) in extended precision."""
    w = widen(x)
    return w.sum(axis=axis), np.abs(w).sum(axis=axis)


def variance(x, axis=None):
    """(var, sum of the squared deviations) in extended precision, two passes."""
    w = widen(x)
    n = w.shape[0] if axis == 0 else w.size
    d = w - w.sum(axis=axis) / n
    s = (d.real * d.real + d.imag * d.imag).sum(axis=axis) if w.dtype.kind == "c" else (d * d).sum(axis=axis)
    return s / n, s


def freq_shift(x, deltaF, Fs):
    """x exp(1j ((2 pi) deltaF) (k (1 / Fs))): the argument in double as the reference forms it, the phasor and product widened."""
    x = np.asarray(x)
    theta = ((2 * np.pi) * deltaF) * (np.arange(x.shape[0]) * (1 / Fs))
    ph = np.cos(theta.astype(LD)) + 1j * np.sin(theta.astype(LD))
    return widen(x).astype(CLD) * (ph if x.ndim == 1 else ph[:, None])
