"""The adaptive MIMO equalizer on the GPU against the reference's recorded results (tests/golden/eq/eq_*.npz,
tools/gen_golden_eq.py), through numpy arguments and through DeviceArrays (run with -m gpu).

Bounds (tests/eq_cases.py): sigOut and H within 1e-9 rel-L2 and 1e-9 max |ref| per element (the project's bound for
double-precision receiver functions against reference fixtures), errSq within 1e-9 of max |ref|.  `default_prec` holds two runs
of the reference on one complex64 input.  Its complex128 run is matched with prec = complex128 at those bounds; with prec left at
complex64, as the case is named for, the constellation is the single-precision one (3e-8 away from the other), and the result is
held within twice the reference's own distance between its two runs of its complex64 run: the device is double, so that distance
is the reference's rounding, and the factor 2 allows for the two not being collinear."""
import numpy as np
import pytest

import eq_cases as ec
import opticommpy_amd as oa
from opticommpy_amd import device

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


@pytest.mark.parametrize("name", ec.EXPECTED_CASES)
def test_equalizer_matches_the_reference(name):
    g = ec.load(name)
    ec.check_conditions(g)
    x0, r0 = g["sigIn"].copy(), g["symbRef"].copy()
    results = {}
    for kind in ("numpy", "device"):
        x = oa.to_device(x0) if kind == "device" else x0.copy()
        ref = oa.to_device(r0) if kind == "device" else r0.copy()
        before = device.transfer_counts()
        sig, H, errSq, Hiter = oa.mimoAdaptEqualizer(x, ec.param128(g, returnResults=True), ref)
        sig2, H2, errSq2, _ = oa.mimoAdaptEqualizer(x, ec.param128(g, returnResults=True), ref)
        alone = oa.mimoAdaptEqualizer(x, ec.param128(g), ref)
        after = device.transfer_counts()
        label = f"{name} [{kind}]"
        # returnResults: types, shapes, dtypes
        cfg = g["cfg"]
        modes, taps, total = cfg["modes"], cfg["param"].get("nTaps", 15), cfg["total"]
        assert type(sig) is (oa.DeviceArray if kind == "device" else np.ndarray) and type(alone) is type(sig), label
        assert sig.shape == g["sigOut"].shape == alone.shape and sig.dtype == np.complex128, label
        assert sig.shape == ((total,) if cfg["input1D"] else (total, modes)), label
        assert type(H) is np.ndarray and H.shape == (modes ** 2, taps) and H.dtype == np.complex128, label
        assert type(errSq) is np.ndarray and errSq.shape == (modes, total) and errSq.dtype == np.float64, label
        assert Hiter.shape == (modes ** 2, taps, 1) and np.array_equal(Hiter[:, :, 0], H), label
        if kind == "device":
            assert after == before, (name, before, after)                   # no DeviceArray.get / .set inside the calls
            assert np.array_equal(x.get(), x0) and np.array_equal(ref.get(), r0)
        else:
            assert np.array_equal(x, x0) and np.array_equal(ref, r0)        # inputs are never written
        ec.compare_results(host(sig), H, errSq, g, label, static_from=ec.static_start(g))
        # a second call and the call without results give the same bits
        assert np.array_equal(host(sig2), host(sig)) and np.array_equal(H2, H) and np.array_equal(errSq2, errSq), label
        assert np.array_equal(host(alone), host(sig)), label
        results[kind] = (host(sig), H, errSq)
    for a, b in zip(results["numpy"], results["device"]):
        assert np.array_equal(a, b), name                                    # numpy and device calls: the same bits


def test_default_precision_is_within_the_references_own_rounding():
    g = ec.load("default_prec")
    ec.check_conditions(g)
    self_err = float(g["self_err"])
    for kind in ("numpy", "device"):
        x = oa.to_device(g["sigIn"]) if kind == "device" else g["sigIn"]
        ref = oa.to_device(g["symbRef"]) if kind == "device" else g["symbRef"]
        sig = host(oa.mimoAdaptEqualizer(x, ec.param(g), ref))                # prec left at complex64
        assert sig.dtype == np.complex128
        d64, d128 = ec.rel_l2(sig, g["sigOut64"].astype(np.complex128)), ec.rel_l2(sig, g["sigOut"])
        print(f"default_prec [{kind}]: distance to the complex64 run {d64:.2e} (the reference's own {self_err:.2e}), to the "
              f"complex128 run, whose constellation is computed in double, {d128:.2e}")
        assert d64 <= 2 * self_err, (kind, d64, self_err)


def test_chain_stays_on_the_device():
    """decimate -> mimoAdaptEqualizer -> cpr -> metrics on DeviceArrays with no host copy in between, equal to the same calls fed
    host copies."""
    rng = np.random.default_rng(21)
    nsym, sps_in, modes = 2048, 4, 2
    table = oa.grayMapping(16, "qam")
    table = (table / np.sqrt(np.mean(np.abs(table) ** 2))).astype(np.complex128)
    tx = table[rng.integers(0, 16, size=(nsym, modes))]
    up = np.repeat(tx, sps_in, axis=0)
    th = 0.5
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    rx = (up @ rot.T) * np.exp(1j * 0.2) + (rng.normal(size=up.shape) + 1j * rng.normal(size=up.shape)) * np.sqrt(10 ** (-2.2) / 2)
    dec = ec.Param(SpSin=sps_in, SpSout=2)
    eq = ec.Param(alg=["nlms", "dd-lms"], mu=[5e-3, 1e-3], L=[600, nsym - 600], nTaps=15, SpS=2, M=16, numIter=3, prec=np.complex128)
    cp = ec.Param(M=16, constType="qam", N=35, B=64, runFOE=False)

    def chain(sig, symb):
        y = oa.mimoAdaptEqualizer(oa.decimate(sig, dec), eq, symb)
        z = oa.cpr(y, cp)
        return y, oa.fastBERcalc(z, symb, 16, "qam", discard=700)

    rxd, txd = oa.to_device(rx), oa.to_device(tx)
    before = device.transfer_counts()
    yd, (BERd, SERd, SNRd) = chain(rxd, txd)
    assert device.transfer_counts() == before and isinstance(yd, oa.DeviceArray)
    y, (BER, SER, SNR) = chain(rx, tx)
    print(f"BER {BERd} (device chain), {BER} (numpy arguments); SNR {SNR} dB")
    assert np.array_equal(yd.get(), y)
    assert np.array_equal(BERd, BER) and np.array_equal(SERd, SER) and np.array_equal(SNRd, SNR)
    assert np.all(BER < 0.02)
