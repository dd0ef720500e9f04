"""The lines the reference's notebooks write between two stages, on DeviceArrays at 2^16 samples: ``symbTx_[:, :, chIndex]``,
``np.sqrt(P) * pnorm(x)``, ``y[discard:-discard]``, ``y[ind, :]``, ``I - I.mean()``, ``x / np.std(x)``, ``.real``, ``.T``.  Each chain
keeps ``transfer_counts()["d2h"]`` unchanged until its final ``.get()`` and is compared with the same lines on numpy arrays through
the package's host-array path."""
import numpy as np
import pytest

import cpr_cases as cc
import fec_cases as fc
import opticommpy_amd as oa
import siso_cases as sc
from opticommpy_amd import device

pytestmark = pytest.mark.gpu
N = 1 << 16


def downloads():
    return device.transfer_counts()["d2h"]


def test_coherent_chain():
    """One channel of a WDM symbol block (sent, and received with a phase walk and noise) -> launch power -> pnorm -> cpr -> the
    edges discarded by a slice and by an index array -> fastBERcalc: equal to what ``discard=k`` gives, and to the same lines on
    numpy arrays."""
    rng = np.random.default_rng(21)
    nCh, ch, P, discard = 3, 1, 0.5e-3, 700
    table = oa.grayMapping(16, "qam")
    table = (table / np.sqrt(np.mean(np.abs(table) ** 2))).astype(np.complex128)
    symb = table[rng.integers(0, 16, size=(N, 2, nCh))]
    walk = np.exp(1j * np.cumsum(rng.normal(size=(N, 2, 1)) * 0.01, axis=0))
    field = symb * walk + (rng.normal(size=symb.shape) + 1j * rng.normal(size=symb.shape)) * np.sqrt(10 ** (-1.6) / 2)      # the channel
    prm = dict(M=16, constType="qam", N=35, B=64, runFOE=False)
    ind = np.arange(discard, N - discard)

    def chain(symb_, field_):
        tx = symb_[:, :, ch]
        sig = np.sqrt(P) * oa.pnorm(field_[:, :, ch])
        y = oa.cpr(oa.pnorm(sig), cc.Param(**prm))
        by_slice = oa.fastBERcalc(y[discard:-discard], tx[discard:-discard], 16, "qam")
        by_index = oa.fastBERcalc(y[ind, :], tx[ind, :], 16, "qam")
        by_param = oa.fastBERcalc(y, tx, 16, "qam", discard=discard)
        return y, tx, by_slice, by_index, by_param, oa.metrics(y, tx, 16, "qam", discard=discard)

    sd, fd = oa.to_device(symb), oa.to_device(field)
    before = downloads()
    yd, txd, a, b, c, m = chain(sd, fd)
    assert downloads() == before and isinstance(yd, oa.DeviceArray) and isinstance(txd, oa.DeviceArray) and txd.shape == (N, 2)
    for got in (a, b):
        assert all(np.array_equal(g, w) for g, w in zip(got, c))                 # BER, SER, SNR: what discard=k gives
    assert np.array_equal(a[0], m["BER"]) and np.array_equal(a[2], m["SNR"])
    yh, txh, ah, bh, _, _ = chain(symb, field)
    assert np.array_equal(txd.get(), txh) and np.array_equal(yd.get(), yh)
    assert all(np.array_equal(g, w) for g, w in zip(a, ah)) and all(np.array_equal(g, w) for g, w in zip(b, bh))
    print(f"coherent chain: BER {a[0]}, SNR {a[2]} dB")
    assert np.all(a[0] < 0.02) and np.all(a[0] > 0)


def test_imdd_chain():
    """photodiode -> ``I - I.mean()`` -> ``(I / I.std()).astype(complex128)`` -> resample -> ``.real`` -> pnorm -> ffe -> fastBERcalc:
    the chain that could not be run on the device, because the photodiode's float64 current is not what resample takes and nothing
    converted it.  Within 1e-9 of the run on host arrays (the device's mean and deviation are sums in another order than numpy's)."""
    rng = np.random.default_rng(11)
    sps, Rs = 4, 10e9
    nsym = N // sps
    table = sc.pam_table(4)
    tx = table[rng.integers(0, 4, size=nsym)]
    drive = np.repeat(tx, sps)
    drive = np.convolve(drive, [0.1, 0.2, 0.4, 0.2, 0.1], mode="same") + 0.15 * np.roll(drive, sps)
    E = np.sqrt(1e-3 * (1.0 + 0.45 * drive / np.max(np.abs(drive)))).astype(np.complex128)
    pd = dict(Fs=sps * Rs, B=0.9 * Rs, ideal=False, shotNoise=False, thermalNoise=False, seed=1, N=65)
    rs = dict(inFs=sps * Rs, outFs=2 * Rs, N=201)
    eq = dict(nTaps=11, SpS=2, mu=5e-3, nTrain=2000, M=4, constType="pam", prec=np.float64)
    discard = 2500

    def chain(E_, tx_):
        I = oa.photodiode(E_, sc.Param(**pd))
        I = I - I.mean()
        x = (I / I.std()).astype(np.complex128)
        x = oa.resample(x, sc.Param(**rs))
        y = oa.ffe(oa.pnorm(x.real), tx_, sc.Param(**eq))[0]
        y = oa.pnorm(y)
        return I, x, y, oa.fastBERcalc(y, tx_, 4, "pam", discard=discard)

    Ed, txd = oa.to_device(E), oa.to_device(tx)
    before = downloads()
    Id, xd, yd, (ber_d, ser_d, snr_d) = chain(Ed, txd)
    assert downloads() == before and all(isinstance(v, oa.DeviceArray) for v in (Id, xd, yd))
    assert Id.dtype == np.float64 and xd.dtype == np.complex128 and xd.ndim == 1
    Ih, xh, yh, (ber_h, ser_h, snr_h) = chain(E, tx)
    for name, got, want in (("current", Id.get(), Ih), ("resampled", xd.get(), xh), ("equalized", yd.get(), yh)):
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"IM/DD chain, {name}: {err:.2e} of the largest sample from the host-array run")
        assert got.shape == want.shape and err <= 1e-9
    print(f"IM/DD chain: BER {float(ber_d[0]):.3e} on the device, {float(ber_h[0]):.3e} on host arrays, SNR {float(snr_d[0]):.1f} dB")
    assert np.array_equal(ber_d, ber_h) and abs(snr_d[0] - snr_h[0]) <= 1e-6 and ber_d[0] <= 1e-2


def test_coded_link():
    """calcLLR(...).reshape(nwords, -1) into decodeLDPC(transposed=True) against .reshape(nwords, -1).T into decodeLDPC: the
    reference's own line, now that a DeviceArray has a .T.  The bits are equal."""
    g = fc.load("msa_648_mixed")
    rng = np.random.default_rng(8)
    M, nwords, n = 16, 400, 648                                             # 64 800 symbols
    raw = oa.grayMapping(M, "qam")
    bitMap = oa.demodulateGray(raw, M, "qam").reshape(-1, 4)
    const = (raw / np.sqrt(np.mean(np.abs(raw) ** 2))).astype(np.complex128)
    px = np.ones(M) / M
    zero = const[np.flatnonzero(~bitMap.any(axis=1))[0]]                    # the symbol that carries 0000: the all-zero codeword
    s2 = 10 ** (-7.0 / 10)
    nsym = nwords * n // 4
    rx = zero + np.sqrt(s2 / 2) * (rng.normal(size=nsym) + 1j * rng.normal(size=nsym))
    prm = dict(H=fc.H_of(g), alg="SPA", maxIter=20, prec=np.float32)

    rxd = oa.to_device(rx)
    before = downloads()
    llr = oa.calcLLR(rxd, s2, const, bitMap, px)
    bits_t, post_t, fail_t = oa.decodeLDPC(llr.reshape(nwords, -1), fc.Param(**prm), transposed=True)
    bits, post, fail = oa.decodeLDPC(llr.reshape(nwords, -1).T, fc.Param(**prm))
    back = bits.T
    assert downloads() == before and isinstance(bits, oa.DeviceArray) and bits.shape == (n, nwords) and bits_t.shape == (nwords, n)
    assert np.array_equal(back.get(), bits_t.get()) and np.array_equal(post.T.get(), post_t.get()) and np.array_equal(fail, fail_t)
    llr_h = oa.calcLLR(rx, s2, const, bitMap, px)
    bits_h, _, fail_h = oa.decodeLDPC(llr_h.reshape(nwords, -1).T, fc.Param(**prm))
    assert np.array_equal(bits.get(), bits_h) and np.array_equal(fail, fail_h)
    print(f"coded link: {int(fail.sum())} of {nwords} frames in error, pre-FEC bit errors {int(np.sum(llr_h < 0))} of {llr_h.size}")
    assert np.sum(llr_h < 0) > 0 and fail.sum() < nwords
