"""The IM/DD transmitter and the AWGN channel on the GPU.  Every fixture of tests/golden/imddtx goes through numpy arguments and
through DeviceArray arguments (identical bits where no device noise is involved), every shape row of tests/imddtx_cases.py against
the extended-precision restatement.  Bound: 1e-12 of the largest sample of the reference, the bound of the WDM transmitter's tests.

Device-generated noise is held to what the estimators' own spread allows at n = 2^18 (6 standard deviations, nothing tuned):
the noise power within 6 / sqrt(n) relative of sigma^2 (6 sqrt(2 / n) for real noise), the mean of each part within
6 sigma / sqrt(2 n), the correlation coefficients between parts, columns and lag-1 neighbours below 6 / sqrt(n).

The chains keep ``device.transfer_counts()`` unchanged between their first and last call."""
import numpy as np
import pytest

import imddtx_cases as ic
import imddtx_restatement as ir
import opticommpy_amd as oa
from opticommpy_amd import device as dev
from opticommpy_amd.wdm_tx import pulseShape

pytestmark = pytest.mark.gpu


def pam_taps(p):
    return pulseShape(ic.make_param(dict(pulseType=p.pulseType, nFilterTaps=p.nFilterTaps, rollOff=p.pulseRollOff, SpS=p.SpS)))


# ------------------------------------------------------------------ fixtures, both routes
@pytest.mark.parametrize("case", ic.PAM_CASES)
def test_pam_fixture(case):
    g = ic.load("pam_" + case)
    d = g["cfg"]["param"]
    res = oa.pamTransmitter(ic.make_param(d))
    resd = oa.pamTransmitter(ic.make_param(d), device_output=True)
    assert len(res) == len(resd) == (3 if d.get("returnParam") else 2)
    assert isinstance(resd[0], oa.DeviceArray) and isinstance(resd[1], np.ndarray) and resd[0].shape == g["sigTxo"].shape
    assert np.array_equal(res[1], g["symbTx"]) and np.array_equal(resd[1], g["symbTx"])
    assert np.array_equal(res[0], resd[0].get())
    err = ic.rel_peak(res[0], g["sigTxo"])
    print(f"pam_{case}: {err:.2e}")
    assert err <= ic.BOUND


@pytest.mark.parametrize("case", ic.MOD_CASES)
def test_modulator_fixture(case):
    g = ic.load("mod_" + case)
    a = ic.mod_call(g)
    b = ic.mod_call(g, convert=oa.to_device)
    assert isinstance(a, np.ndarray) and isinstance(b, oa.DeviceArray) and b.shape == g["out"].shape and b.dtype == np.complex128
    assert np.array_equal(a, b.get())
    err = ic.rel_peak(a, g["out"])
    print(f"mod_{case}: {err:.2e}")
    assert err <= ic.BOUND


def test_modulator_with_one_argument_on_the_device():
    g = ic.load("mod_mzm_er80_array")
    want = ic.mod_call(g)
    prm = ic.make_param(g["cfg"]["param"])
    for Ei, u in ((oa.to_device(g["Ei"]), g["u"]), (g["Ei"], oa.to_device(g["u"]))):
        out = oa.mzm(Ei, u, prm)
        assert isinstance(out, oa.DeviceArray) and np.array_equal(out.get(), want)
    # firFilter's complex128 result as the drive, its imaginary part zero: the real case
    u = g["u"].astype(np.complex128)
    assert ic.rel_peak(oa.mzm(1.0, oa.to_device(u), prm).get(), oa.mzm(1.0, g["u"], prm)) <= 1e-15


@pytest.mark.parametrize("case", ic.AWGN_CASES)
def test_awgn_fixture_from_numpy(case):
    g = ic.load("awgn_" + case)
    ic.awgn_seed_global(g)
    out = oa.awgn(g["sig"], ic.make_param(g["cfg"]["param"]))
    ic.awgn_seed_global(g)
    again = oa.awgn(g["sig"], ic.make_param(g["cfg"]["param"]))
    assert out.dtype == g["out"].dtype and out.shape == g["out"].shape and np.array_equal(out, again)
    err = ic.rel_peak(out, g["out"])
    print(f"awgn_{case}: {err:.2e}")
    assert err <= ic.BOUND


@pytest.mark.parametrize("case", ic.AWGN_CASES)
def test_awgn_fixture_from_a_device_array(case):
    """Device noise: the fixture's signal, the fixture's sigma^2 -- statistical parity at the fixture's small n."""
    g = ic.load("awgn_" + case)
    d = dict(g["cfg"]["param"], seed=41)
    cplx = d.get("complexNoise", True)
    out = oa.awgn(oa.to_device(g["sig"]), ic.make_param(d))
    assert isinstance(out, oa.DeviceArray) and out.dtype == g["out"].dtype and out.shape == g["out"].shape
    noise = out.get() - g["sig"]
    n = noise.size
    want = float(g["sigma2"]) * (1 if cplx else 0.5)
    assert abs(np.mean(np.abs(noise) ** 2) / want - 1) <= 6 * np.sqrt((1 if cplx else 2) / n)
    if not cplx:
        assert np.all(noise.imag == 0)


def test_sources_upsample_and_voa():
    g = ic.load("sources")
    for name, factor in g["cfg"]["rows"]["upsample"].items():
        x = g[name + "_in"]
        a, b = oa.upsample(x, factor), oa.upsample(oa.to_device(x), factor)
        assert a.dtype == g[name].dtype and np.array_equal(a, g[name]), name
        assert isinstance(b, oa.DeviceArray) and b.dtype == x.dtype and np.array_equal(b.get(), g[name]), name
    x = g["up_2d_5_in"]
    for arr in (x, x.real.copy(), x[:, 0].copy()):
        want = arr * 10 ** (-2.5 / 20)
        assert np.array_equal(oa.voa(arr, 2.5), want) and np.array_equal(oa.voa(oa.to_device(arr), 2.5).get(), want)
    assert np.array_equal(oa.upsample(np.array([-0.0, np.nan, 1e-310]), 2).view(np.uint64),
                          ir.upsample(np.array([-0.0, np.nan, 1e-310]), 2).view(np.uint64))        # the bits are copied


# ------------------------------------------------------------------ shape rows
@pytest.mark.parametrize("rid", list(ic.PAM_ROWS))
def test_pam_shape_row(rid):
    p = ic.make_param(ic.PAM_ROWS[rid])
    sig, symb = oa.pamTransmitter(p)
    sigd, _ = oa.pamTransmitter(ic.make_param(ic.PAM_ROWS[rid]), device_output=True)
    want = ic.pam_restated(symb, pam_taps(p), vars(p))
    assert sig.shape == want.shape and np.array_equal(sig, sigd.get())
    assert ic.rel_peak(sig, want) <= ic.BOUND


@pytest.mark.parametrize("rid", list(ic.PEAK_ROWS))
def test_peak_row(rid):
    got, want = ic.run_peak_row(rid)
    gotd, _ = ic.run_peak_row(rid, device_output=True)
    assert np.array_equal(got, gotd) and ic.rel_peak(got, want) <= ic.BOUND


@pytest.mark.parametrize("kind", ["pm", "mzm", "iqm"])
@pytest.mark.parametrize("n", ic.MOD_ROW_SIZES)
def test_modulator_shape_row(kind, n):
    Ei, u = ic.mod_row_inputs(n, kind)
    if kind == "pm":
        got, want = oa.pm(oa.to_device(Ei), oa.to_device(u), 2.5), ir.pm(Ei, u, 2.5)
    elif kind == "mzm":
        got, want = oa.mzm(oa.to_device(Ei), oa.to_device(u), ic.make_param(dict(Vpi=2, Vb=-0.6, ER=25))), ir.mzm(Ei, u, 2, -0.6, 25)
    else:
        prm = dict(Vpi=2, VbI=-1.7, VbQ=-2.2, Vphi=0.9, ERI=10, ERQ=80)
        got, want = oa.iqm(oa.to_device(Ei), oa.to_device(u), ic.make_param(prm)), ir.iqm(Ei, u, **prm)
    assert ic.rel_peak(got.get(), ir.narrow(want)) <= ic.BOUND


@pytest.mark.parametrize("n", [ic.EW_SPAN - 1, ic.EW_SPAN + 1])
def test_either_side_of_the_grid_stride_span(n):
    Ei, u, want = ic.span_row(n)
    got = oa.mzm(oa.to_device(Ei), oa.to_device(u), ic.make_param(dict(Vpi=2, Vb=-0.6, ER=25))).get()
    assert ic.rel_peak(got, want) <= ic.BOUND
    assert np.array_equal(oa.upsample(oa.to_device(u), 1).get(), u)            # the copy launch at the same edge
    assert np.array_equal(oa.voa(oa.to_device(u), 1.0).get(), u * 10 ** (-1.0 / 20))


@pytest.mark.parametrize("shape,real", [((1,), False), ((2,), True), ((255,), False), ((256,), True), ((257, 1), False), ((300, 3), False),
                                        ((513,), True), ((700, 3), True)])
def test_awgn_shape_row(shape, real):
    rng = np.random.default_rng(sum(shape))
    sig = rng.standard_normal(shape) if real else rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    out = oa.awgn(sig, ic.make_param(dict(snr=11, Fs=3.0, B=2.0, complexNoise=not real, seed=77)))
    np.random.seed(77)
    zr = np.random.standard_normal(shape)
    zi = None if real else np.random.standard_normal(shape)
    want = ir.narrow(ir.awgn(sig, zr, zi, 1.5, 10 ** 1.1))
    assert out.dtype == want.dtype and ic.rel_peak(out, want) <= ic.BOUND
    outd = oa.awgn(oa.to_device(sig), ic.make_param(dict(snr=11, Fs=3.0, B=2.0, complexNoise=not real, seed=77)))
    assert outd.shape == shape and outd.dtype == out.dtype and np.all(np.isfinite(outd.get()))


# ------------------------------------------------------------------ device noise
N_NOISE = 1 << 18


def corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float(np.sum(a * b) / np.sqrt(np.sum(a * a) * np.sum(b * b)))


@pytest.fixture(scope="module")
def noise_runs():
    n = N_NOISE
    t = np.arange(n)
    sig = np.stack([np.exp(2j * np.pi * 0.01 * t), 0.5 * np.exp(-2j * np.pi * 0.003 * t)], axis=1)      # mean |sig|^2 = 0.625
    sd = oa.to_device(sig)
    prm = dict(snr=7, Fs=2.0, B=1.0)
    sigma2 = 2.0 * 0.625 / 10 ** 0.7
    runs = {"sig": sig, "sigma2": sigma2}
    runs["a"] = oa.awgn(sd, ic.make_param(dict(prm, seed=3))).get() - sig
    runs["a2"] = oa.awgn(sd, ic.make_param(dict(prm, seed=3))).get() - sig
    runs["b"] = oa.awgn(sd, ic.make_param(dict(prm, seed=4))).get() - sig
    runs["u1"] = oa.awgn(sd, ic.make_param(prm)).get() - sig
    runs["u2"] = oa.awgn(sd, ic.make_param(prm)).get() - sig
    runs["real"] = oa.awgn(oa.to_device(sig.real.copy()), ic.make_param(dict(prm, complexNoise=False, seed=3))).get() - sig.real
    runs["real_sigma2"] = 2.0 * np.mean(sig.real ** 2) / 10 ** 0.7
    return runs


def test_device_noise_has_the_asked_power_and_no_structure(noise_runs):
    z, sigma2 = noise_runs["a"], noise_runs["sigma2"]
    n = z.size                                                     # 2^19 complex samples over the two columns
    bound = 6 / np.sqrt(n)
    assert abs(np.mean(np.abs(z) ** 2) / sigma2 - 1) <= bound
    s = np.sqrt(sigma2 / 2)
    assert abs(z.real.mean()) <= 6 * s / np.sqrt(n) and abs(z.imag.mean()) <= 6 * s / np.sqrt(n)        # s = sigma / sqrt 2
    for col in range(2):
        c = z[:, col]
        m = len(c)
        assert abs(np.mean(np.abs(c) ** 2) / sigma2 - 1) <= 6 / np.sqrt(m)
        assert abs(c.real.mean()) <= 6 * np.sqrt(sigma2) / np.sqrt(2 * m) and abs(c.imag.mean()) <= 6 * np.sqrt(sigma2) / np.sqrt(2 * m)
        assert abs(corr(c.real, c.imag)) <= 6 / np.sqrt(m)
        assert abs(corr(c.real[1:], c.real[:-1])) <= 6 / np.sqrt(m) and abs(corr(c.imag[1:], c.imag[:-1])) <= 6 / np.sqrt(m)
        assert abs(corr(c.real[1:], c.imag[:-1])) <= 6 / np.sqrt(m)
    m = len(z)
    assert abs(corr(z[:, 0].real, z[:, 1].real)) <= 6 / np.sqrt(m) and abs(corr(z[:, 0].imag, z[:, 1].imag)) <= 6 / np.sqrt(m)
    assert abs(corr(z[:, 0].real, z[:, 1].imag)) <= 6 / np.sqrt(m)
    r = noise_runs["real"]
    assert r.dtype == np.float64
    m = r.size
    assert abs(np.mean(r ** 2) / (noise_runs["real_sigma2"] / 2) - 1) <= 6 * np.sqrt(2 / m)
    assert abs(r.mean()) <= 6 * np.sqrt(noise_runs["real_sigma2"] / 2) / np.sqrt(m)
    assert abs(corr(r[:, 0], r[:, 1])) <= 6 / np.sqrt(len(r)) and abs(corr(r[1:, 0], r[:-1, 0])) <= 6 / np.sqrt(len(r))


def test_device_noise_repeats_per_seed_and_only_per_seed(noise_runs):
    assert np.array_equal(noise_runs["a"], noise_runs["a2"])
    for other in ("b", "u1"):
        assert not np.array_equal(noise_runs["a"], noise_runs[other])
        assert abs(corr(noise_runs["a"].real.ravel(), noise_runs[other].real.ravel())) <= 6 / np.sqrt(noise_runs["a"].size)
    assert not np.array_equal(noise_runs["u1"], noise_runs["u2"])


def test_device_noise_shares_no_stream_with_edfa(noise_runs):
    sig = noise_runs["sig"]
    amp = oa.edfa(oa.to_device(sig), ic.make_param(dict(G=20, NF=5, Fs=64e9, seed=3))).get() - sig * np.sqrt(10 ** (20 / 10))
    a = noise_runs["a"]
    m = a.size
    za, ze = a / np.sqrt(np.mean(np.abs(a) ** 2)), amp / np.sqrt(np.mean(np.abs(amp) ** 2))
    assert not np.allclose(za, ze, atol=1e-3)
    assert abs(corr(za.real.ravel(), ze.real.ravel())) <= 6 / np.sqrt(m) and abs(corr(za.imag.ravel(), ze.imag.ravel())) <= 6 / np.sqrt(m)


# ------------------------------------------------------------------ chains
def test_pam_transmitter_to_photodiode_stays_on_the_device():
    g = ic.load("pam_rrc")
    before = dev.transfer_counts()
    sig, symb = oa.pamTransmitter(ic.make_param(g["cfg"]["param"]), device_output=True)
    ipd = oa.photodiode(sig, ic.make_param(dict(ideal=True)))
    assert dev.transfer_counts() == before and isinstance(ipd, oa.DeviceArray)
    err = ic.rel_peak(ipd.get(), g["ipd"])
    print(f"pam -> photodiode: {err:.2e}")
    assert err <= ic.BOUND


def theory_ber_qam(M, snr_db):
    """theoryBER(M, EbN0, 'qam') of optic/comm/metrics.py:640-686 in closed form, EbN0 = SNR / log2 M:
    2 (1 - 1 / L) / log2 L * Q(sqrt(3 log2 L / (L^2 - 1) * 2 EbN0)), L = sqrt M, Q(x) = erfc(x / sqrt 2) / 2."""
    from math import erfc, log2, sqrt
    L = sqrt(M)
    EbN0 = 10 ** (snr_db / 10) / log2(M)
    x = sqrt(3 * log2(L) / (L ** 2 - 1) * (2 * EbN0))
    return 2 * (1 - 1 / L) / log2(L) * 0.5 * erfc(x / sqrt(2))


def test_modulate_awgn_metrics_chain():
    n, M, snr = 1 << 16, 16, 15
    bits = oa.bitSource(ic.make_param(dict(nBits=4 * n, seed=12))).astype(np.uint8)
    bd = oa.to_device(bits)
    before = dev.transfer_counts()
    tx = oa.pnorm(oa.modulateGray(bd, M, "qam"))
    rx = oa.awgn(tx, ic.make_param(dict(snr=snr, seed=21)))
    BER, SER, SNR = oa.fastBERcalc(rx, tx, M, "qam")
    m = oa.metrics(rx, tx, M, "qam")
    assert dev.transfer_counts() == before
    lo, hi = 10 * np.log10(1 - 6 / np.sqrt(n)), 10 * np.log10(1 + 6 / np.sqrt(n))
    print(f"SNR {float(SNR[0]):.4f} dB, BER {float(BER[0]):.3e}, theory {theory_ber_qam(M, snr):.3e}")
    assert snr + lo <= float(SNR[0]) <= snr + hi and snr + lo <= float(m["SNR"][0]) <= snr + hi
    # fastBERcalc normalises the received symbols to unit power before it subtracts (optic/comm/metrics.py:183-187), so what it
    # estimates is not 1 / s2 but 1 / ((1 - 1 / sqrt(1 + s2))^2 + s2 / (1 + s2)): 15.1015 dB at 15 dB, 0.1015 dB above the channel's
    # SNR and a hair outside the window above, which this seeded run (15.0924 dB on an MI355X) meets with 0.008 dB to spare.  The
    # same window around the estimator's own expectation is the check with room on both sides:
    s2 = 10 ** (-snr / 10)
    expect = -10 * np.log10((1 - 1 / np.sqrt(1 + s2)) ** 2 + s2 / (1 + s2))
    assert expect + lo <= float(SNR[0]) <= expect + hi
    pb = theory_ber_qam(M, snr)
    nbits = 4 * n
    assert abs(float(BER[0]) - pb) <= 6 * np.sqrt(pb * (1 - pb) / nbits)
    assert float(m["BER"][0]) == float(BER[0])


def test_notebook_cell():
    """bitSource -> modulateGray -> upsample -> firFilter -> mzm -> linearFiberChannel -> photodiode with oa. names only, on numpy
    arrays and kept on the device."""
    c = ic.load("cell_ook")
    k = c["cfg"]["param"]
    bits = oa.bitSource(ic.make_param(dict(nBits=256, mode="random", seed=123)))
    assert np.array_equal(bits, c["bits"])
    pulse = oa.pulseShape(ic.make_param(dict(pulseType="nrz", SpS=k["SpS"])))
    Ai = np.sqrt(1e-3 * 10 ** (k["Pi_dBm"] / 10))
    for on_device in (False, True):
        b = oa.to_device(bits.astype(np.uint8)) if on_device else bits
        before = dev.transfer_counts()
        symb = oa.modulateGray(b, k["M"], "pam")
        up = oa.upsample(symb, k["SpS"])
        sigTx = oa.firFilter(pulse, up)
        sigTxo = oa.mzm(Ai, sigTx, ic.make_param(dict(Vpi=k["Vpi"], Vb=k["Vb"])))
        sigCh = oa.linearFiberChannel(sigTxo, ic.make_param(k["ch"]))
        ipd = oa.photodiode(sigCh, ic.make_param(dict(ideal=True)))
        if on_device:
            assert dev.transfer_counts() == before and isinstance(ipd, oa.DeviceArray)
        assert np.array_equal(ic.host(up), c["symbolsUp"])
        for name, got in (("sigTx", sigTx), ("sigTxo", sigTxo), ("sigCh", sigCh), ("ipd", ipd)):
            err = ic.rel_peak(ic.host(got), c[name])
            print(f"cell[{'device' if on_device else 'numpy'}] {name}: {err:.2e}")
            assert err <= ic.BOUND, name
