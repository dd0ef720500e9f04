"""numpy complex128 restatement of the reference's ``modulateOFDM`` and ``demodulateOFDM`` (optic/comm/ofdm.py), written from their
description: the yardstick of the OFDM shape tests, itself held to the reference-generated fixtures by
tests/test_ofdm_restatement.py.  Plain loops over frames, every array materialised, nothing shared with the package; at the end
the same two functions with the frames as an array axis, byte-equal to the loops, for the one row of 10^5 frames.

Two deliberate differences from the reference, both stated in the fixtures' bounds: the transforms run in double whatever the
input type (numpy >= 2 transforms a complex64 frame in single precision), and a signal is never written."""
import numpy as np


def layout(Nfft, hermitSymmetry, pilotCarriers, nullCarriers):
    """(Ns, data carriers) of a parameter set."""
    Ns = Nfft // 2 - 1 if hermitSymmetry else Nfft
    taken = np.union1d(np.asarray(pilotCarriers, dtype=np.int64), np.asarray(nullCarriers, dtype=np.int64))
    return Ns, np.setdiff1d(np.arange(Ns), taken)


def modulate(symb, Nfft=512, G=4, hermitSymmetry=False, pilot=0.25 + 0.25j, SpS=2, pilotCarriers=(), nullCarriers=()):
    """The transmit signal in complex128, not yet rounded to the reference's complex64."""
    pilots = np.asarray(pilotCarriers, dtype=np.int64)
    nulls = np.asarray(nullCarriers, dtype=np.int64)
    Ns, data = layout(Nfft, hermitSymmetry, pilots, nulls)
    Ni = len(data)
    symb = np.asarray(symb)
    assert len(symb) % Ni == 0
    F = len(symb) // Ni
    L = SpS * Nfft
    out = np.zeros((F, SpS * (Nfft + G)), dtype=np.complex128)
    for f in range(F):
        V = np.zeros(Ns, dtype=np.complex64)                 # the frame's values are single precision
        V[data] = symb[f * Ni:(f + 1) * Ni]
        V[pilots] = pilot
        V[nulls] = 0
        V = V.astype(np.complex128)
        if hermitSymmetry:
            V = np.concatenate(([0], V, [0], np.conj(V[::-1])))
        pad = (Nfft * (SpS - 1)) // 2
        X = np.fft.fftshift(np.concatenate((np.zeros(pad), V, np.zeros(pad))))
        assert len(X) == L
        x = np.fft.ifft(X) * np.sqrt(L)
        out[f, SpS * G:] = x
        out[f, :SpS * G] = x[L - SpS * G:]
    return out.ravel()


def line_through(x, y, at):
    """Piecewise-linear interpolation of (x, y) at ``at`` with the end segments running on; x in any order."""
    order = np.argsort(x)
    x, y = np.asarray(x, dtype=np.float64)[order], np.asarray(y, dtype=np.float64)[order]
    hi = np.clip(np.searchsorted(x, at, side="left"), 1, len(x) - 1)
    lo = hi - 1
    return (y[hi] - y[lo]) / (x[hi] - x[lo]) * (at - x[lo]) + y[lo]


def demodulate(sig, Nfft=512, G=4, hermitSymmetry=False, pilot=0.25 + 0.25j, pilotCarriers=(), nullCarriers=(), **_):
    """(symbols, H) in complex128; H is 0j without pilots."""
    pilots = np.asarray(pilotCarriers, dtype=np.int64)
    Ns, data = layout(Nfft, hermitSymmetry, pilots, nullCarriers)
    sig = np.asarray(sig).astype(np.complex128)
    assert len(sig) % (Nfft + G) == 0
    F = len(sig) // (Nfft + G)
    Y = np.zeros((F, Ns), dtype=np.complex128)
    for f in range(F):
        frame = sig[f * (Nfft + G) + G:(f + 1) * (Nfft + G)]
        S = np.fft.fftshift(np.fft.fft(frame)) / np.sqrt(Nfft)
        Y[f] = S[1:1 + Ns] if hermitSymmetry else S
    H = 0j
    if len(pilots):
        carriers = np.arange(Ns, dtype=np.float64)
        mag, ang = np.zeros(Ns), np.zeros(Ns)
        for f in range(F):
            est = Y[f, pilots] / pilot
            mag += line_through(pilots, np.abs(est), carriers)
            ang += line_through(pilots, np.angle(est), carriers)
        H = (mag / F) * np.exp(1j * (ang / F))
        Y = Y / H
    return Y[:, data].ravel(), H


# ---- the same two functions with the frames as an array axis, for signals of 10^5 frames where the loops above take minutes.  Every
# frame goes through the same operations in the same order, and the sums over the frames stay loops in frame order, so the output
# is byte-equal to the loops' (tests/test_ofdm_restatement.py asserts that on every shape row).
def modulate_frames(symb, Nfft=512, G=4, hermitSymmetry=False, pilot=0.25 + 0.25j, SpS=2, pilotCarriers=(), nullCarriers=()):
    pilots = np.asarray(pilotCarriers, dtype=np.int64)
    nulls = np.asarray(nullCarriers, dtype=np.int64)
    Ns, data = layout(Nfft, hermitSymmetry, pilots, nulls)
    Ni = len(data)
    symb = np.asarray(symb)
    assert len(symb) % Ni == 0
    F = len(symb) // Ni
    L = SpS * Nfft
    V = np.zeros((F, Ns), dtype=np.complex64)
    V[:, data] = symb.reshape(F, Ni)
    V[:, pilots] = pilot
    V[:, nulls] = 0
    V = V.astype(np.complex128)
    if hermitSymmetry:
        V = np.concatenate((np.zeros((F, 1)), V, np.zeros((F, 1)), np.conj(V[:, ::-1])), axis=1)
    pad = (Nfft * (SpS - 1)) // 2
    X = np.fft.fftshift(np.concatenate((np.zeros((F, pad)), V, np.zeros((F, pad))), axis=1), axes=1)
    assert X.shape == (F, L)
    x = np.fft.ifft(X, axis=1) * np.sqrt(L)
    out = np.zeros((F, SpS * (Nfft + G)), dtype=np.complex128)
    out[:, SpS * G:] = x
    out[:, :SpS * G] = x[:, L - SpS * G:]
    return out.ravel()


def lines_through(x, y, at):
    """``line_through`` for every row of ``y``."""
    order = np.argsort(x)
    x, y = np.asarray(x, dtype=np.float64)[order], np.asarray(y, dtype=np.float64)[:, order]
    hi = np.clip(np.searchsorted(x, at, side="left"), 1, len(x) - 1)
    lo = hi - 1
    return (y[:, hi] - y[:, lo]) / (x[hi] - x[lo]) * (at - x[lo]) + y[:, lo]


def demodulate_frames(sig, Nfft=512, G=4, hermitSymmetry=False, pilot=0.25 + 0.25j, pilotCarriers=(), nullCarriers=(), **_):
    pilots = np.asarray(pilotCarriers, dtype=np.int64)
    Ns, data = layout(Nfft, hermitSymmetry, pilots, nullCarriers)
    sig = np.asarray(sig).astype(np.complex128)
    assert len(sig) % (Nfft + G) == 0
    F = len(sig) // (Nfft + G)
    S = np.fft.fftshift(np.fft.fft(sig.reshape(F, Nfft + G)[:, G:], axis=1), axes=1) / np.sqrt(Nfft)
    Y = S[:, 1:1 + Ns] if hermitSymmetry else S
    H = 0j
    if len(pilots):
        carriers = np.arange(Ns, dtype=np.float64)
        est = Y[:, pilots] / pilot
        mags, angs = lines_through(pilots, np.abs(est), carriers), lines_through(pilots, np.angle(est), carriers)
        mag, ang = np.zeros(Ns), np.zeros(Ns)
        for f in range(F):                                   # the sums in frame order, as above
            mag += mags[f]
            ang += angs[f]
        H = (mag / F) * np.exp(1j * (ang / F))
        Y = Y / H
    return Y[:, data].ravel(), H
