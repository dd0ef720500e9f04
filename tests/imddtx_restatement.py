"""An extended-precision (np.longdouble) restatement of the IM/DD transmitter's and the AWGN channel's signal paths, written from
the reference's formulas (optic/models/tx.py:317-342, optic/dsp/core.py:1076-1139, 701-717, optic/models/devices.py:214-218,
optic/models/channels.py:556-565): the PAM path from given symbols and taps, the modulators from given drives, awgn from given unit
normals.  It shares one thing with the reference on purpose: pi is the double np.pi, as in ``(u / Vpi) * np.pi``.  Held to the
reference's fixtures at 1e-12 of the peak (tests/test_imddtx_restatement.py), then used for the shape rows, where no fixture
exists."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
PI = LD(np.pi)


def shaped(symbols, taps, SpS):
    """firFilter(taps, upsample(symbols, SpS)): the 'same' part of the full convolution, first sample (len(taps) - 1) // 2."""
    symbols, taps = np.asarray(symbols, dtype=LD), np.asarray(taps, dtype=LD)
    N = len(symbols) * SpS
    full = np.zeros(N + len(taps) - 1, dtype=LD)
    for k, s in enumerate(symbols):                      # only the stuffed samples are non-zero
        full[k * SpS:k * SpS + len(taps)] += s * taps
    start = (len(taps) - 1) // 2
    return full[start:start + N]


def peak_margin(sig):
    """1 - (largest |sample| that is not the peak) / peak.  Samples within 1e-12 of the peak are the peak: the flat top of an NRZ
    pulse under equal symbols is one value to rounding."""
    a = np.abs(np.asarray(sig, dtype=LD))
    peak = np.max(a)
    rest = a[a < peak * (1 - LD(1e-12))]
    return float(1 - np.max(rest) / peak) if len(rest) else 1.0


def _pm_factor(z, Vpi):
    z = np.asarray(z)
    zr, zi = (z.real.astype(LD), z.imag.astype(LD)) if np.iscomplexobj(z) else (z.astype(LD), np.zeros(z.shape, dtype=LD))
    ar, ai = (zr / LD(Vpi)) * PI, (zi / LD(Vpi)) * PI
    m = np.exp(-ai)
    return (m * np.cos(ar)).astype(CLD) + CLD(1j) * (m * np.sin(ar)).astype(CLD)


def _arms(ER):
    erLin = 10 ** (ER / 10)                                # double, as calcMZM and the library derive it
    gamma = 2 * np.sqrt(erLin) / (erLin + 1)
    return LD(np.sqrt(1 + gamma)), LD(np.sqrt(1 - gamma))


def _wide(x):
    x = np.asarray(x)
    return x.astype(CLD) if np.iscomplexobj(x) else x.astype(LD)


def pm(Ei, u, Vpi):
    return _wide(Ei) * _pm_factor(_wide(u), Vpi)


def mzm(Ei, u, Vpi=2, Vb=-1, ER=60):
    sp, sm = _arms(ER)
    v = (_wide(u) + LD(Vb)) / 2
    h = _wide(Ei) / 2
    return sp * (h * _pm_factor(v, Vpi)) + sm * (h * _pm_factor(-v, Vpi))


def iqm(Ei, u, Vpi=2, VbI=-2, VbQ=-2, Vphi=1, ERI=60, ERQ=60):
    u = _wide(u)
    ur, ui = (u.real, u.imag) if np.iscomplexobj(u) else (u, np.zeros(u.shape, dtype=LD))
    h = _wide(Ei) / LD(np.sqrt(2))
    return mzm(h, ur, Vpi, VbI, ERI) + pm(mzm(h, ui, Vpi, VbQ, ERQ), np.full(u.shape, LD(Vphi)), Vpi)


def pam_field(symbols, taps, SpS, mzmScale=0.25, mzmVpi=3, mzmVb=1.5, mzmER=80, power=-3):
    """One mode of pamTransmitter from its symbols and taps: (field, shaped signal)."""
    sig = shaped(symbols, taps, SpS)
    u = LD(mzmScale) * (LD(mzmVpi) * sig / np.max(np.abs(sig)))
    E = mzm(LD(1), u, mzmVpi, -mzmVb, mzmER)
    mean = np.mean(E.real ** 2 + E.imag ** 2)
    return np.sqrt(LD(1e-3 * 10 ** (power / 10))) * (E / np.sqrt(mean)), sig


def awgn(sig, zr, zi, FsB, snr_lin):
    """sig + sqrt(sigma2 / 2) (zr + 1j zi), zi None for real noise; sigma2 = FsB * mean(|sig|^2) / snr_lin."""
    x = _wide(sig)
    pw = np.mean(x.real ** 2 + x.imag ** 2) if np.iscomplexobj(x) else np.mean(x ** 2)
    s = np.sqrt(LD(FsB) * (pw / LD(snr_lin)) / 2)
    nr = s * np.asarray(zr, dtype=LD).reshape(x.shape)
    if zi is None:
        return x + nr
    return x + (nr.astype(CLD) + CLD(1j) * (s * np.asarray(zi, dtype=LD).reshape(x.shape)).astype(CLD))


def upsample(x, factor):
    x = np.asarray(x)
    out = np.zeros((x.shape[0] * factor,) + x.shape[1:], dtype=x.dtype)
    out[::factor] = x
    return out


def narrow(x):
    """The restated values in the dtype the functions return."""
    x = np.asarray(x)
    return x.astype(np.complex128) if np.iscomplexobj(x) else x.astype(np.float64)
