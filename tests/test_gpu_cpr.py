"""Carrier phase recovery on the GPU against the reference's recorded results (tests/golden/cpr/cpr_*.npz, tools/gen_golden_cpr.py),
through numpy arguments and through DeviceArrays, and against numpy restatements at sizes no fixture covers (run with -m gpu).

Bounds (tests/cpr_cases.py): raw test phases within 1e-12 rad at every symbol (grid values; the fixtures' margin conditions rule
out a flipped decision), unwrapped phases within 1e-9 rad, sigOut and the frequency-compensated signal within 1e-9 rel-L2 and
1e-9 max |ref| per element (the project's bound for double-precision receiver functions against reference fixtures), fo within
1e-12 relative."""
import numpy as np
import pytest

import cpr_cases as cc
import opticommpy_amd as oa
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


@pytest.mark.parametrize("name", cc.EXPECTED_CASES)
def test_cpr_matches_the_reference(name):
    g = cc.load(name)
    cc.check_conditions(g)
    cfg = g["cfg"]
    x0 = g["sigIn"].copy()
    results = {}
    for kind in ("numpy", "device"):
        x = oa.to_device(x0) if kind == "device" else x0.copy()
        bx0 = np.ascontiguousarray(cc.bps_input(g))
        bx = oa.to_device(bx0) if kind == "device" else bx0.copy()
        before = device.transfer_counts()
        sig, phase = oa.cpr(x, cc.param(g, returnPhases=True))
        again, phase2 = oa.cpr(x, cc.param(g, returnPhases=True))
        alone = oa.cpr(x, cc.param(g, returnPhases=False))
        gpu_alg = oa.cpr(x, cc.param(g, returnPhases=False, alg="bpsGPU"))
        raw = oa.bps(bx, cfg["N"] // 2, g["table"], cfg["B"])
        raw_gpu = oa.bpsGPU(bx, cfg["N"] // 2, g["table"], cfg["B"])
        foe = oa.fourthPowerFOE(x, 1 / cfg["Ts"], cfg["P"]) if cfg["foe"] else None
        after = device.transfer_counts()
        want_type = oa.DeviceArray if kind == "device" else np.ndarray
        for a in (sig, phase, alone, raw) + ((foe[0],) if foe else ()):
            assert type(a) is want_type and a.shape == x0.shape, (name, kind, type(a), a.shape)
        if kind == "device":
            assert after == before, (name, before, after)                   # no DeviceArray.get / .set inside the calls
            assert np.array_equal(x.get(), x0) and np.array_equal(bx.get(), bx0)
        else:
            assert np.array_equal(x, x0) and np.array_equal(bx, bx0)        # inputs are never written
        label = f"{name} [{kind}]"
        r = dict(sig=host(sig), phase=host(phase), raw=host(raw))
        cc.compare_phases(r["raw"], g["raw"], cc.RAW_ABS, f"{label} raw bps")
        cc.compare_phases(r["phase"], g["phaseEst"], cc.PHASE_ABS, f"{label} phaseEst")
        cc.compare_signal(r["sig"], g["sigOut"], f"{label} sigOut")
        assert np.array_equal(host(raw_gpu), r["raw"])
        # a repeated call, the call without phases and alg = 'bpsGPU' give the same bits
        assert np.array_equal(host(again), r["sig"]) and np.array_equal(host(phase2), r["phase"]), label
        assert np.array_equal(host(alone), r["sig"]) and np.array_equal(host(gpu_alg), r["sig"]), label
        if foe:
            assert isinstance(foe[1], np.ndarray) and foe[1].dtype == np.float64
            cc.compare_fo(foe[1], g["fo"], f"{label} fo")
            cc.compare_signal(host(foe[0]), g["sig_foe"], f"{label} fourthPowerFOE")
            r["foe"], r["fo"] = host(foe[0]), foe[1]
        results[kind] = r
    for k, v in results["numpy"].items():
        assert np.array_equal(v, results["device"][k]), (name, k)            # numpy and device calls: the same bits


@pytest.fixture(scope="module")
def qam16_8192():
    """n = 8192, 16-QAM at 20 dB with a phase walk; the search over the whole signal and its margins in numpy."""
    x, table = cc.noisy_qam16(8192, 1, 20, 0.02, seed=11)
    idx, margin = cc.numpy_bps(x, 17, table, 64)
    return x, table, idx, margin


def test_decisions_do_not_depend_on_the_tile_geometry(qam16_8192):
    x, table, idx, margin = qam16_8192
    Nh, B = 17, 64
    print(f"smallest numpy argmin margin: {margin.min():.2e}")
    assert margin.min() >= 1e-9
    phases = np.arange(0, B) * (np.pi / 2) / B
    whole = oa.bps(x, Nh, table, B)
    assert np.array_equal(whole, phases[idx])
    for a, b in ((3, 5001), (1237, 8190), (4099, 4099 + 777)):
        assert all((a % p) and (b % p) for p in (8, 16, 32, 64, 128, 256))
        part = oa.bps(np.ascontiguousarray(x[a:b]), Nh, table, B)
        assert np.array_equal(whole[a + Nh:b - Nh], part[Nh:-Nh]), (a, b)


def test_many_workgroups_against_a_numpy_restatement():
    """n = 2^16 + 37 symbols x 2 modes, a phase walk that wraps past pi / 2 many times: raw index, np.unwrap and pnorm in numpy."""
    n, N, B = 65573, 35, 64
    x, table = cc.noisy_qam16(n, 2, 20, 0.02, seed=12)
    x = x * np.exp(1j * 2e-3 * np.arange(n))[:, None]                        # ... and a drift of about 80 quarter turns
    idx, margin = cc.numpy_bps(x, N // 2, table, B)
    phases = np.arange(0, B) * (np.pi / 2) / B
    prm = cc.Param(M=16, constType="qam", N=N, B=B, runFOE=False, returnPhases=True)
    xd = oa.to_device(x)
    sig, phase = oa.cpr(xd, prm)
    raw = oa.bps(xd, N // 2, table, B).get()
    sig, phase = sig.get(), phase.get()

    sure = margin >= 1e-9
    left_out = 1 - np.count_nonzero(sure) / sure.size
    print(f"smallest numpy margin {margin.min():.2e}; share of symbols left out {left_out:.2e}")
    assert left_out <= 1e-4
    assert np.array_equal(raw[sure], phases[idx][sure])
    steps = np.abs(np.diff(raw, axis=0))
    assert np.count_nonzero(steps > np.pi / 4) >= 40                         # the walk does wrap many times
    # phases and signal from the GPU's own raw decisions where numpy's are not sure, numpy's elsewhere
    ref_raw = np.where(sure, phases[idx], raw)
    ref_phase = np.unwrap(4 * ref_raw, axis=0) / 4
    cc.compare_phases(phase, ref_phase, cc.PHASE_ABS, "65573 x 2 phaseEst")
    y = x * np.exp(1j * ref_phase)
    y = y / np.sqrt(np.mean(y * np.conj(y)).real)
    e = cc.rel_l2(sig, y)
    print(f"65573 x 2 sigOut: rel-L2 {e:.2e}")
    assert e <= cc.REL


def test_limits_of_the_kernel():
    """The largest table (1024 scattered points: no product of levels, so the full search) with 128 test phases; the longest
    window, longer than the signal; the shortest signal with 64 modes."""
    rng = np.random.default_rng(13)
    table = rng.normal(size=1024) + 1j * rng.normal(size=1024)
    x = table[rng.integers(0, 1024, size=(200, 1))] * np.exp(-0.2j) + 0.001 * (rng.normal(size=(200, 1)) + 1j * rng.normal(size=(200, 1)))
    idx, margin = cc.numpy_bps(x, 100, table, 128)
    raw = oa.bps(x, 100, table, 128)
    sure = margin >= 1e-9
    assert sure.mean() > 0.99 and np.array_equal(raw[sure], (np.arange(128) * (np.pi / 2) / 128)[idx][sure])
    assert abs(np.median(raw) - 0.2) < 0.02
    for t in (table[::16], table):                                            # (three and two test phases per LDS chunk)
        big = oa.bps(x, 1023, t, 3)
        idx, margin = cc.numpy_bps(x, 1023, t, 3)
        sure = margin >= 1e-9
        assert sure.mean() > 0.99 and np.array_equal(big[sure], (np.arange(3) * (np.pi / 2) / 3)[idx][sure])

    x2, t16 = cc.noisy_qam16(2, 64, 25, 0.0, seed=14)
    sig, phase = oa.cpr(x2, cc.Param(M=16, N=1023, B=128, runFOE=False, returnPhases=True))
    idx, margin = cc.numpy_bps(x2, 511, t16, 128)
    want = np.unwrap(4 * (np.arange(128) * (np.pi / 2) / 128)[idx], axis=0) / 4
    sure = np.all(margin >= 1e-9, axis=0)
    assert sure.sum() >= 32
    cc.compare_phases(phase[:, sure], want[:, sure], cc.PHASE_ABS, "2 x 64 phaseEst")
    assert sig.shape == (2, 64) and abs(np.mean(np.abs(sig) ** 2) - 1) <= 1e-12


def test_derotation_at_large_angles():
    """fourthPowerFOE with P = 1 on a tone near a third of the sampling rate over 400 000 symbols: the derotation's angle reaches
    8e5 rad; fo and the compensated signal against numpy."""
    n, Fs = 400000, 32e9
    k = np.arange(n)
    x = np.exp(1j * 2 * np.pi * 0.3217 * k) * (1 + 0.1 * np.cos(0.001 * k))
    y, fo = oa.fourthPowerFOE(x, Fs, 1)
    f = np.fft.fftshift(Fs * np.fft.fftfreq(n))
    want_fo = f[np.argmax(np.abs(np.fft.fftshift(np.fft.fft(x))))] / 1
    assert y.shape == (n,) and fo.shape == (1,) and fo[0] == want_fo
    t = k * 1 / Fs
    assert abs(2 * np.pi * fo[0] * t[-1]) > 8e5
    cc.compare_signal(y, x * np.exp(-1j * 2 * np.pi * fo[0] * t), "derotation up to 8e5 rad")


def test_chain_stays_on_the_device():
    """to_device -> cpr -> metrics with no host copy in between; the BER of the same symbols through numpy arguments."""
    rng = np.random.default_rng(15)
    n = 4096
    table = oa.grayMapping(16, "qam")
    table = (table / np.sqrt(np.mean(np.abs(table) ** 2))).astype(np.complex128)
    tx = table[rng.integers(0, 16, size=(n, 2))]
    walk = np.cumsum(rng.normal(size=(n, 2)) * 0.01, axis=0)
    rx = (tx + (rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))) * np.sqrt(10 ** (-1.6) / 2)) * np.exp(1j * walk)
    prm = cc.Param(M=16, constType="qam", N=35, B=64, runFOE=False)
    rxd, txd = oa.to_device(rx), oa.to_device(tx)
    before = device.transfer_counts()
    out = oa.cpr(rxd, prm)
    BERd, SERd, SNRd = oa.fastBERcalc(out, txd, 16, "qam", discard=100)
    assert device.transfer_counts() == before and isinstance(out, oa.DeviceArray)
    BER, SER, SNR = oa.fastBERcalc(oa.cpr(rx, prm), tx, 16, "qam", discard=100)
    print(f"BER {BERd} (device chain), {BER} (numpy arguments)")
    assert np.array_equal(BERd, BER) and np.array_equal(SERd, SER) and np.array_equal(SNRd, SNR)
    assert np.all(BER < 0.02)
