"""firFilter, blockwiseFFTConv's result, delaySignal and decimate (optic/dsp/core.py:87-125, 435-491, 880-922, 973-1046) restated
with every convolution taken directly in the time domain in ``np.longdouble`` over the zero-extended signal -- no transform, so no
transform's rounding and no block size -- and decimate's variances in two passes in ``np.longdouble``.  Plain numpy, no project
code.  decimate also returns the chosen phases and ``margin``, the smallest relative gap between the largest variance and the
next one over the columns: a case whose margin is far above the rounding of a double-precision sum has one right answer."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble


def _full(h, x):
    """The full linear convolution of two 1-D sequences (len(h) + len(x) - 1 values), from real extended-precision sums."""
    h, x = np.asarray(h), np.asarray(x)
    hr, hi, xr, xi = h.real.astype(LD), h.imag.astype(LD), x.real.astype(LD), x.imag.astype(LD)
    zero = np.zeros(len(h) + len(x) - 1, dtype=LD)
    c = lambda a, b: np.convolve(a, b) if np.any(a) and np.any(b) else zero    # noqa: E731
    out = np.empty(len(zero), dtype=CLD)
    out.real = c(hr, xr) - c(hi, xi)
    out.imag = c(hr, xi) + c(hi, xr)
    return out


def conv_shift(h, x, shift, outLen):
    """out[n, m] = sum_t h[t] x[n + shift - t, m] for n in [0, outLen), x extended with zeros on both sides (clongdouble)."""
    x = np.asarray(x)
    x2 = x.reshape(len(x), -1)
    out = np.zeros((outLen, x2.shape[1]), dtype=CLD)
    for m in range(x2.shape[1]):
        full = _full(h, x2[:, m])
        lo, hi = max(0, -shift), min(outLen, len(full) - shift)
        if hi > lo:
            out[lo:hi, m] = full[lo + shift:hi + shift]
    return out.reshape((outLen,) + x.shape[1:])


def convolve_same(h, x):
    """firFilter / blockwiseFFTConv: the convolution with the delay (len(h) - 1) // 2 taken off, len(x) samples per column."""
    return conv_shift(h, x, (len(h) - 1) // 2, len(x))


def delay_signal(x, delay, Fs=1, NFFT=1024):
    """delaySignal (core.py:880-922): the NFFT // 2 frequency samples exp(-j 2 pi f delay) become the centred impulse response
    (core.py:1015-1016), the signal is extended by padLen zeros, filtered, rolled by -1 and cut to its length."""
    x = np.asarray(x)
    N = len(x)
    padLen = int(np.ceil(np.abs(delay * Fs)))
    if NFFT is None:
        NFFT = 2 ** int(np.ceil(np.log2(N + padLen)))
    freq = np.fft.fftfreq(NFFT // 2, d=1 / Fs)
    H = np.exp(-1j * 2 * np.pi * freq * delay)
    h = np.fft.fftshift(np.fft.ifft(H))
    y = conv_shift(h, x, (len(h) - 1) // 2, N + padLen)
    return np.roll(y, -1)[:N]


def decimate(x, SpSin, SpSout):
    """decimate (core.py:435-491) -> (out, sampDelay, margin).  Per column the first phase of the largest two-pass variance, then
    every int(SpSin / SpSout)-th sample of the column rolled by that phase.  margin: the smallest (best - runner-up) / best over
    the columns; where the best is tied exactly, the runner-up is the largest strictly smaller variance (inf when there is none)."""
    x = np.asarray(x)
    x2 = x.reshape(len(x), -1)
    dec = int(SpSin / SpSout)
    sampDelay = np.zeros(x2.shape[1], dtype=np.int64)
    margin = np.inf
    out = x2[::dec].copy()
    for k in range(x2.shape[1]):
        var = np.var(x2[:, k].astype(CLD if x2.dtype.kind == "c" else LD).reshape(-1, SpSin), axis=0)
        best = np.max(var)
        sampDelay[k] = np.flatnonzero(var == best)[0]
        below = var[var < best]
        if len(below) and best > 0:
            margin = min(margin, float((best - np.max(below)) / best))
        out[:, k] = np.roll(x2[:, k], -int(sampDelay[k]))[::dec]
    return out.reshape((len(out),) + x.shape[1:]), sampDelay, margin
