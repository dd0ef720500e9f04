"""symbolSync and finddelay on the GPU against the reference's recorded results (tests/golden/sync/sync_*.npz,
tools/gen_golden_sync.py), through numpy arguments and through DeviceArrays (run with -m gpu).

Bounds (tests/sync_cases.py): the output equal to the reference's, delay, swap, rot and conj equal, corrMatrix within 1e-9 of its
largest entry.  Every fixture's smallest decision margin is above 1e-6 (the rounding of the transforms is about 1e-13)."""
import numpy as np
import pytest

import eq_cases as ec
import opticommpy_amd as oa
import sync_cases as sc
import sync_restatement as sr
from helpers import load_golden, make_param
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


@pytest.mark.parametrize("name", sc.EXPECTED_CASES)
def test_symbol_sync_matches_the_reference(name):
    g = sc.load(name)
    sc.check_conditions(g)
    cfg = g["cfg"]
    rx0, tx0 = g["rx"].copy(), g["tx"].copy()
    results = {}
    for kind in ("numpy", "device"):
        rx = oa.to_device(rx0) if kind == "device" else rx0.copy()
        tx = oa.to_device(tx0) if kind == "device" else tx0.copy()
        before = device.transfer_counts()
        out, info = oa.symbolSync(rx, tx, cfg["SpS"], cfg["mode"], return_info=True)
        out2, info2 = oa.symbolSync(rx, tx, cfg["SpS"], cfg["mode"], return_info=True)
        alone = oa.symbolSync(rx, tx, cfg["SpS"], cfg["mode"])
        after = device.transfer_counts()
        label = f"{name} [{kind}]"
        assert type(out) is (oa.DeviceArray if kind == "device" else np.ndarray) and type(alone) is type(out), label
        assert out.shape == tx0.shape and out.dtype == tx0.dtype, label
        if kind == "device":
            assert after == before, (name, before, after)                   # no DeviceArray.get / .set inside the calls
            assert np.array_equal(rx.get(), rx0) and np.array_equal(tx.get(), tx0)
        else:
            assert np.array_equal(rx, rx0) and np.array_equal(tx, tx0)      # inputs are never written
        sc.compare(host(out), info, g["out"], g, label)
        # a second call and the call without the record give the same bits
        assert host(out2).tobytes() == host(out).tobytes() == host(alone).tobytes(), label
        assert np.array_equal(info2.corrMatrix, info.corrMatrix) and np.array_equal(info2.delay, info.delay), label
        results[kind] = (host(out), info)
    assert results["numpy"][0].tobytes() == results["device"][0].tobytes(), name    # numpy and device calls: the same bits
    assert np.array_equal(results["numpy"][1].corrMatrix, results["device"][1].corrMatrix), name
    # one side on the device is enough for a DeviceArray
    mixed = oa.symbolSync(oa.to_device(rx0), tx0, cfg["SpS"], cfg["mode"])
    assert isinstance(mixed, oa.DeviceArray) and mixed.get().tobytes() == results["numpy"][0].tobytes()


@pytest.mark.parametrize("name", sc.EXPECTED_CASES)
def test_finddelay_on_the_fixtures_own_pairs(name):
    """The sequences the reference's finddelay saw: |tx[:, swap[k]]| - mean against |rx_k| - mean in 'amp', the real parts of the
    rotated column and of rx_k in 'real'."""
    g = sc.load(name)
    cfg = g["cfg"]
    cols = len(g["delay"])
    rx = g["rx"].reshape(len(g["rx"]), cols)
    rx = sr.decimate(rx, cfg["SpS"]) if cfg["SpS"] > 1 else rx
    tx = g["tx"].reshape(len(g["tx"]), cols)
    for k in range(cols):
        if cfg["mode"] == "amp":
            a, b = np.abs(tx[:, g["swap"][k]]), np.abs(rx[:, k])
            a, b = a - np.mean(a), b - np.mean(b)
        else:
            a, b = np.real(g["rot"][k] * tx[:, g["swap"][k]]), np.real(rx[:, k])
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        before = device.transfer_counts()
        on_device = oa.finddelay(oa.to_device(a), oa.to_device(b))
        counts = device.transfer_counts()
        assert counts["d2h"] == before["d2h"] and counts["h2d"] == before["h2d"] + 2
        got = oa.finddelay(a, b)
        assert type(got) is int and got == on_device == int(g["delay"][k]), (name, k, got, on_device, g["delay"][k])
    # complex sequences of unequal length: y is conjugated, the offset is len(x) - 1
    x, y = tx[:, 0], rx[: len(rx) // 2 + 1, 0]
    assert oa.finddelay(x, y) == sr.finddelay(x, y) == oa.finddelay(oa.to_device(x), y)


def _disperse(x, L, Fs, D=16.0, Fc=193.1e12):
    """Chromatic dispersion of L km on every column: the response edc compensates, applied circularly."""
    c_kms = 299792458.0 / 1e3
    lam = c_kms / Fc
    b2 = -(D * lam ** 2) / (2 * np.pi * c_kms)
    w = 2 * np.pi * Fs * np.fft.fftfreq(len(x))
    return np.fft.ifft(np.fft.fft(x, axis=0) * np.exp(1j * (b2 / 2) * w ** 2 * L)[:, None], axis=0)


def _shape(tx, sps, rolloff=0.35):
    """The symbols at sps samples per symbol under a raised-cosine pulse of 16 symbols, applied circularly."""
    up = np.zeros((len(tx) * sps, tx.shape[1]), dtype=np.complex128)
    up[::sps] = tx
    t = np.arange(-8 * sps, 8 * sps + 1) / sps + 1e-9
    pulse = np.sinc(t) * np.cos(np.pi * rolloff * t) / (1 - (2 * rolloff * t) ** 2)
    h = np.fft.fft(np.roll(np.pad(pulse, (0, len(up) - len(pulse))), -8 * sps))
    return np.fft.ifft(np.fft.fft(up, axis=0) * h[:, None], axis=0)


def test_chain_stays_on_the_device():
    """decimate -> edc -> symbolSync -> pnorm -> mimoAdaptEqualizer(..., d) -> cpr -> fastBERcalc on DeviceArrays with no host copy
    in between, equal to the same calls fed host copies.  The signal is that of tests/test_gpu_eq.py's chain (16-QAM, two modes
    turned into each other by 0.5 rad, a carrier phase, noise at 22 dB) under a band-limited pulse and the dispersion of 100 km,
    so that edc has something to undo.  The transmitted symbols handed over are circularly shifted by 37 and their two modes
    swapped: without symbolSync the equalizer trains on the wrong symbols.  (The tests' numpy restatements of these stages give
    BER 0 and 19 dB on this input, 0.5 without the synchronisation.)"""
    rng = np.random.default_rng(21)
    nsym, sps_in, modes, Rs = 2048, 4, 2, 32e9
    table = oa.grayMapping(16, "qam")
    table = (table / np.sqrt(np.mean(np.abs(table) ** 2))).astype(np.complex128)
    tx = table[rng.integers(0, 16, size=(nsym, modes))]
    up = _shape(tx, sps_in)
    th = 0.5
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    rx = _disperse((up @ rot.T) * np.exp(1j * 0.2), 100.0, sps_in * Rs)
    rx = rx + (rng.normal(size=up.shape) + 1j * rng.normal(size=up.shape)) * np.sqrt(10 ** (-2.2) / 2)
    symb = np.ascontiguousarray(np.roll(tx, 37, axis=0)[:, ::-1])
    dec = ec.Param(SpSin=sps_in, SpSout=2)
    edc = ec.Param(L=100.0, D=16.0, Fc=193.1e12, Rs=Rs, Fs=2 * Rs)
    eq = ec.Param(alg=["nlms", "dd-lms"], mu=[2e-2, 1e-3], L=[600, nsym - 600], nTaps=15, SpS=2, M=16, numIter=3, prec=np.complex128)
    cp = ec.Param(M=16, constType="qam", N=35, B=64, runFOE=False)

    def chain(sig, symb, sync=True):
        x = oa.edc(oa.decimate(sig, dec), edc)
        d = oa.symbolSync(x, symb, 2) if sync else symb
        y = oa.mimoAdaptEqualizer(oa.pnorm(x), eq, d)
        z = oa.cpr(y, cp)
        return d, y, oa.fastBERcalc(z, d, 16, "qam", discard=700)

    rxd, symbd = oa.to_device(rx), oa.to_device(symb)
    before = device.transfer_counts()
    dd, yd, (BERd, SERd, SNRd) = chain(rxd, symbd)
    assert device.transfer_counts() == before and isinstance(dd, oa.DeviceArray) and isinstance(yd, oa.DeviceArray)
    d, y, (BER, SER, SNR) = chain(rx, symb)
    _, _, (BER0, _, _) = chain(rx, symb, sync=False)
    print(f"BER {BERd} (device chain), {BER} (numpy arguments), {BER0} without symbolSync; SNR {SNR} dB")
    assert np.array_equal(dd.get(), d) and np.array_equal(yd.get(), y)
    assert np.array_equal(BERd, BER) and np.array_equal(SERd, SER) and np.array_equal(SNRd, SNR)
    assert np.all(BER < 0.02)
    assert np.all(BER0 > 0.3)


def test_notebook_chain():
    """The `out` of tests/golden/chain_wdm_240k.npz and the selected channel's symbols from simpleWDMTx with that fixture's
    transmitter settings, against the reference's symbolSync on the same (tests/golden/sync/sync_chain_wdm.npz)."""
    d, cfg = load_golden("chain_wdm_240k")
    g = sc.load(sc.CHAIN_CASE)
    sc.check_conditions(g)
    _, symbTx, _ = oa.simpleWDMTx(make_param(oa.parameters, cfg["tx"]))
    assert np.array_equal(symbTx[:64], d["symb_head"])
    tx = np.ascontiguousarray(symbTx[:, :, cfg["chIndex"]]).astype(g["cfg"]["tx_dtype"])
    outd, info = oa.symbolSync(oa.to_device(d["out"]), oa.to_device(tx), 2, return_info=True)
    out = outd.get()
    assert out.shape == tx.shape and out.dtype == tx.dtype
    for k in ("delay", "swap", "rot", "conj"):
        assert np.array_equal(getattr(info, k), g[k]), (k, getattr(info, k), g[k])
    err = float(np.max(np.abs(info.corrMatrix - g["corrMatrix"])) / np.max(g["corrMatrix"]))
    print(f"notebook chain: delay {info.delay.tolist()}, swap {info.swap.tolist()}, corrMatrix error / largest entry {err:.2e}")
    assert err <= sc.CORR_REL
    assert np.array_equal(out[:64], g["out_head"])
    assert np.max(np.abs(sc.projection(out) - g["out_proj"])) <= 1e-12 * np.sqrt(np.sum(np.abs(out) ** 2))


def test_transform_timing_aid():
    """ssf_sync_transform_time (tools/bench_sync.py's floor) runs the engine's plans and returns a device time."""
    import ctypes as C
    from opticommpy_amd import _lib
    lib = _lib.load()
    s = C.c_double(-1.0)
    assert lib.ssf_sync_transform_time(0, 4096, 6, 4, 2, 3, C.byref(s)) == 0
    assert 0.0 < s.value < 1.0
