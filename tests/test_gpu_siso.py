"""ffe, dfe, volterra and anorm on the GPU (run with -m gpu): against the reference's recorded results
(tests/golden/siso/siso_*.npz, tools/gen_golden_siso.py) through numpy arguments and through DeviceArrays, and against the
restatement (tests/siso_restatement.py) at every shape at which the kernels take another path (tests/siso_cases.py: ROWS).

Bounds (tests/siso_cases.py): sigOut and the coefficients within 1e-9 rel-L2 and 1e-9 of max |ref| per element, mse within 1e-9 of
max |ref|.  The `*_default_prec` cases hold two runs of the reference on one single-precision input: its double run is matched at
those bounds, and with prec left unset the result is held within twice the reference's own distance between its two runs
(self_err) of its single-precision run -- the device recursion is double, so that distance is the reference's rounding, and the
factor 2 allows for the two not being collinear."""
import functools

import numpy as np
import pytest

import opticommpy_amd as oa
import siso_cases as sc
import siso_restatement as sr
from opticommpy_amd import device, sisoeq

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def expected_split(kind, x, ref, prm):
    return sisoeq.expected_split(sisoeq._prepare(kind, x, ref, prm))


@pytest.mark.parametrize("name", sc.EXPECTED_CASES)
def test_fixture_through_numpy_and_device_arguments(name):
    g = sc.load(name)
    sc.check_conditions(g)
    kind, cfg = g["cfg"]["kind"], g["cfg"]
    x0, r0 = sc.inputs(g)
    want = (g["sigOut"], sc.coefficients(g), g["mse"])
    keep_x, keep_r = x0.copy(), r0.copy()
    prm = sc.param(g)
    given = [a.copy() for a in (prm.f, prm.b)] if cfg["init"] else None
    split = expected_split(kind, x0, r0, prm)
    results = {}
    for how in ("numpy", "device"):
        x = oa.to_device(x0) if how == "device" else x0
        ref = oa.to_device(r0) if how == "device" else r0
        before = device.transfer_counts()
        got = sc.call(oa, kind, x, ref, prm)
        ran = dict(sisoeq.last_call)
        again = sc.call(oa, kind, x, ref, prm)
        after = device.transfer_counts()
        label = f"{name} [{how}]"
        kindof = oa.DeviceArray if how == "device" else np.ndarray
        assert type(got[0]) is kindof and type(got[2]) is kindof, label
        assert got[0].dtype == (np.complex128 if cfg["complex"] else np.float64) and got[2].dtype == np.float64, label
        assert all(type(c) is np.ndarray and c.dtype == got[0].dtype for c in got[1]), label
        if how == "device":
            assert after == before, (label, before, after)                  # no DeviceArray.get / .set inside the calls
            assert np.array_equal(x.get(), keep_x) and np.array_equal(ref.get(), keep_r), label
        assert np.array_equal(x0, keep_x) and np.array_equal(r0, keep_r), label                 # inputs are never written
        if given:
            assert np.array_equal(prm.f, given[0]) and np.array_equal(prm.b, given[1]), label   # nor the initial coefficients
        assert (ran["serial_symbols"], ran["parallel_symbols"]) == split and ran["R"] == 1 and ran["N"] == cfg["N"], (label, ran, split)
        got = (host(got[0]), got[1], host(got[2]))
        sc.compare_results(got, want, label)
        again = (host(again[0]), again[1], host(again[2]))
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[2], got[2]), label     # a second call: the same bits
        assert all(np.array_equal(a, b) for a, b in zip(again[1], got[1])), label
        results[how] = got
    a, b = results["numpy"], results["device"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1])), name


@pytest.mark.parametrize("name", [n for n in sc.EXPECTED_CASES if n.endswith("default_prec")])
def test_default_precision_is_within_the_references_own_rounding(name):
    g = sc.load(name)
    sc.check_conditions(g)
    self_err, kind = float(g["self_err"]), g["cfg"]["kind"]
    x0, r0 = sc.inputs(g, double=False)
    assert x0.dtype == np.float32
    for how in ("numpy", "device"):
        x = oa.to_device(x0) if how == "device" else x0
        ref = oa.to_device(r0) if how == "device" else r0
        sig = host(sc.call(oa, kind, x, ref, sc.param(g, double=False))[0])      # prec left unset
        assert sig.dtype == np.float64
        d32, d64 = sc.rel_l2(sig, g["sigOut32"].astype(np.float64)), sc.rel_l2(sig, g["sigOut"])
        print(f"{name} [{how}]: distance to the single-precision run {d32:.2e} (the reference's own {self_err:.2e}), to the double run {d64:.2e}")
        assert d32 <= 2 * self_err, (how, d32, self_err)


@functools.lru_cache(maxsize=None)
def restated(rid):
    kind, x, tx, prm = sc.row(rid)
    return sr.restate(kind, x, tx, prm)


@pytest.mark.parametrize("rid", sc.ROW_IDS)
def test_shape_row_matches_the_restatement(rid):
    kind, x, tx, prm = sc.row(rid)
    want = restated(rid)
    # no decision of the row is a near tie -- but for the one exact tie that the zeroed last sample of the one-tap row makes
    # (an output of exactly 0 between -1 and +1: |0 - c| is exact on both sides, and the first minimum is the same point)
    assert want["gap"] >= 1e-7 or (rid == "ffe_one_tap" and want["gap"] == 0.0 and want["sigOut"][-1] == 0.0), (rid, want["gap"])
    given = getattr(prm, "h", None)
    given = [a.copy() for a in given] if given is not None else None
    got = sc.call(oa, kind, x, tx, prm)
    ran = dict(sisoeq.last_call)
    sc.compare_results(got, (want["sigOut"], want["coef"], want["mse"]), rid)
    split = expected_split(kind, x, tx, prm)
    assert (ran["serial_symbols"], ran["parallel_symbols"]) == split, (rid, ran, split)
    ncoef = sisoeq._prepare(kind, x, tx, prm)["ncoef"]
    assert ran["R"] == (oa._lib.siso_slots(ncoef) if split[0] else 0), (rid, ran)
    if given is not None:                                          # order 2: h3 comes back as given, and the caller's arrays stay
        assert np.array_equal(got[1][2], given[2]) and all(np.array_equal(a, b) for a, b in zip(prm.h, given))
    xd, td = oa.to_device(x), oa.to_device(tx)
    dev = sc.call(oa, kind, xd, td, prm)
    assert np.array_equal(dev[0].get(), got[0]) and np.array_equal(dev[2].get(), got[2]), rid


def test_output_on_a_decision_threshold_takes_the_first_table_point():
    """One tap of 1 and a sample of exactly 0: the output is 0, halfway between the PAM-4 points -1 and +1 (times 1 / sqrt(5)), which
    stand at places 1 and 3 of the table (Gray-label order: -3, -1, 3, 1).  The first minimum in table order is the negative one.
    In ffe the choice shows in nothing but mse, which both points give alike; dfe feeds the chosen point back, where it shows."""
    table = sisoeq._table(4, "pam", np.float64)
    assert table[1] == -table[3] and table[1] < 0
    n = 64
    rng = np.random.default_rng(3)
    x = table[rng.integers(0, 4, size=n)].copy()
    x[10] = x[40] = 0.0
    tx = np.ones(n)
    for mode in ("data-aided", "fulltime"):                        # the frozen kernel, the serial kernel
        prm = sc.Param(nTaps=1, nTrain=0, f=np.array([1.0]), prec=np.float64, trainingMode=mode, mu=1e-3)
        out, f, mse = oa.ffe(x, tx, prm)
        assert sisoeq.last_call["parallel_symbols"] == (n if mode == "data-aided" else 0)
        assert out[10] == 0.0 and out[40] == 0.0 and mse[10] == table[1] ** 2 and mse[40] == table[1] ** 2, mode
    # dfe with a feed-forward tap of 0 and a feedback tap of 1: the first output is exactly 0, and every later output is the point
    # the symbol before chose -- the first of the two nearest in table order, then that point again
    for mode in ("data-aided", "fulltime"):
        prm = sc.Param(nTapsFF=1, nTapsFB=1, nTrain=0, f=np.array([0.0]), b=np.array([1.0]), prec=np.float64, trainingMode=mode, mu=0.0)
        out, f, b, mse = oa.dfe(x, tx, prm)
        assert out[0] == 0.0 and np.all(out[1:] == table[1]) and mse[0] == table[1] ** 2 and np.all(mse[1:] == 0.0), (mode, out[:3], table)
    want = sr.restate("dfe", x, tx, prm)
    assert np.array_equal(want["sigOut"], out) and want["gap"] == 0.0


@pytest.mark.parametrize("cx", [False, True])
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("dtype", ["wide", "narrow"])
def test_anorm(cx, where, dtype):
    rng = np.random.default_rng(5)
    n = 3001
    x = rng.normal(size=n) + (1j * rng.normal(size=n) if cx else 0)
    x = x / np.max(np.abs(x)) * 0.9
    x[0 if where == "first" else n - 1] = -1.7 + (0.4j if cx else 0)
    x = x.astype({(False, "wide"): np.float64, (False, "narrow"): np.float32, (True, "wide"): np.complex128, (True, "narrow"): np.complex64}[cx, dtype])
    wide = x.astype(np.complex128 if cx else np.float64)
    want = wide / np.max(np.abs(wide))
    keep = x.copy()
    got = oa.anorm(x)
    assert type(got) is np.ndarray and got.dtype == want.dtype and np.array_equal(x, keep)
    sc.compare(got, want, "anorm")
    assert np.max(np.abs(got)) == pytest.approx(1.0, abs=1e-15)
    xd = oa.to_device(x)
    before = device.transfer_counts()
    gd = oa.anorm(xd)
    assert device.transfer_counts() == before and isinstance(gd, oa.DeviceArray)
    assert np.array_equal(gd.get(), got) and np.array_equal(xd.get(), keep)


def _imdd_signal():
    """A PAM-4 intensity-modulated field at 2 samples per symbol with a little ISI, and its symbols."""
    rng = np.random.default_rng(11)
    nsym, sps = 3000, 2
    table = sc.pam_table(4)
    tx = table[rng.integers(0, 4, size=nsym)]
    drive = np.repeat(tx, sps)
    drive = np.convolve(drive, [0.15, 0.7, 0.15], mode="same") + 0.2 * np.roll(drive, sps)
    power = 1e-3 * (1.0 + 0.45 * drive / np.max(np.abs(drive)))
    return np.sqrt(power).astype(np.complex128), tx, sps


def test_chain_stays_on_the_device():
    """balancedPD -> pnorm -> ffe -> pnorm -> fastBERcalc on DeviceArrays with no host copy in between, equal to the same calls fed
    host copies; the BER stays under a bound that the same chain with the restatement in ffe's place meets.  (The reference's chain
    has resample between photodiode and pnorm.  This package's resample filters complex128 DeviceArrays only and refuses the
    photodiode's float64 one -- tests/test_gpu_clock.py -- so the field is made at the equalizer's two samples per symbol and the
    chain on the device goes without it.  A single photodiode's current carries the mean of the intensity, which a zero-mean PAM
    table cannot follow and nothing on the device subtracts: the second photodiode of a balanced pair, fed the unmodulated carrier,
    takes it off.)"""
    E, tx, sps = _imdd_signal()
    Rs = 10e9
    pd = sc.Param(Fs=sps * Rs, B=0.9 * Rs, ideal=False, shotNoise=False, thermalNoise=False, seed=1, N=65)
    eq = sc.Param(nTaps=11, SpS=2, mu=5e-3, nTrain=1000, M=4, constType="pam", prec=np.float64)
    discard, bound = 1100, 1e-2

    carrier = np.full(len(E), np.sqrt(1e-3), dtype=np.complex128)

    def chain(E, tx, equalize):
        # (host copies go in as one column: balancedPD then takes the two-photodiode route that DeviceArrays take, not its
        #  one-launch route for 1-D numpy fields, whose current differs in the last bits)
        i = oa.balancedPD(E, carrier_d, pd) if isinstance(E, oa.DeviceArray) else oa.balancedPD(E.reshape(-1, 1), carrier.reshape(-1, 1), pd)
        i = oa.pnorm(i)
        y = equalize(i, tx)
        y = oa.pnorm(y)
        return y, oa.fastBERcalc(y, tx, 4, "pam", discard=discard)

    Ed, txd, carrier_d = oa.to_device(E), oa.to_device(tx), oa.to_device(carrier)
    before = device.transfer_counts()
    yd, (ber_d, ser_d, snr_d) = chain(Ed, txd, lambda i, t: oa.ffe(i, t, eq)[0])
    assert device.transfer_counts() == before and isinstance(yd, oa.DeviceArray)
    yh, (ber_h, ser_h, snr_h) = chain(E, tx, lambda i, t: oa.ffe(i, t, eq)[0])
    assert np.array_equal(yd.get(), yh) and np.array_equal(ber_d, ber_h) and np.array_equal(snr_d, snr_h)
    _, (ber_r, _, _) = chain(E, tx, lambda i, t: sr.restate("ffe", i, t, eq)["sigOut"])
    print(f"IM/DD chain: BER {float(ber_d[0]):.3e} on the device, {float(ber_r[0]):.3e} with the restatement, SNR {float(snr_d[0]):.1f} dB")
    assert ber_r[0] <= bound and ber_d[0] <= bound
