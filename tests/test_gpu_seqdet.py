"""mlse, detector, autocorr and estimateWhiteningFilter on the GPU (run with -m gpu): against the reference's recorded results
(tests/golden/seqdet/*.npz, tools/gen_golden_seqdet.py) and against the restatement (tests/seqdet_restatement.py) at every shape
at which the kernels can go wrong (tests/seqdet_cases.py), each through numpy arguments and through DeviceArrays.

Bounds (tests/seqdet_cases.py): mlse's output and detector's decided / indDec equal the reference's; the final path metric within
1e-9 relative of the restatement's; autocorr within 1e-9 of r[0] and the whitening filter within 1e-9 of max |w|."""
import numpy as np
import pytest

import opticommpy_amd as oa
import seqdet_cases as sc
from opticommpy_amd import device, seqdet

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def run_mlse(y0, h, c, want_out, want_metrics, states, label):
    """Both kinds of argument, twice each: types, bits, transfer counts, last_call, the bounds.  Returns the numpy result."""
    keep = y0.copy()
    on_device = y0.dtype in (np.float64, np.complex128)             # a DeviceArray is float64 or complex128
    results = {}
    for how in ("numpy", "device") if on_device else ("numpy",):
        y = oa.to_device(y0) if how == "device" else y0
        before = device.transfer_counts()
        got = oa.mlse(y, h, c)
        ran = dict(seqdet.last_call)
        again = oa.mlse(y, h, c)
        after = device.transfer_counts()
        tag = f"{label} [{how}]"
        assert type(got) is (oa.DeviceArray if how == "device" else np.ndarray) and got.dtype == y0.dtype and got.shape == y0.shape, tag
        if how == "device":
            assert after == before, (tag, before, after)              # no DeviceArray.get / .set inside the calls
            assert np.array_equal(y.get(), keep), tag
        assert np.array_equal(y0, keep), tag
        cols = 1 if y0.ndim == 1 else y0.shape[1]
        assert ran["states"] == states and ran["kernel"] == sc.expected_kernel(states) and ran["chunk"] == seqdet.T, (tag, ran)
        assert ran["survivor_bytes"] == seqdet.survivor_bytes(len(y0), cols, states) and ran["N"] == len(y0) and ran["cols"] == cols, (tag, ran)
        got = host(got)
        assert np.array_equal(got, want_out), tag
        for k, m in enumerate(want_metrics):
            d = sc.rel(ran["final_metric"][k], m)
            print(f"{tag}: column {k} final metric within {d:.2e} relative")
            assert d <= sc.TOL, (tag, k, d)
        assert np.array_equal(host(again), got) and np.array_equal(seqdet.last_call["final_metric"], ran["final_metric"]), tag
        results[how] = (got, ran["final_metric"])
    if on_device:
        assert np.array_equal(results["numpy"][0], results["device"][0]) and np.array_equal(results["numpy"][1], results["device"][1]), label
    return results["numpy"]


@pytest.mark.parametrize("name", sc.MLSE_CASES)
def test_mlse_fixture_through_numpy_and_device_arguments(name):
    g = sc.load(f"mlse_{name}")
    sc.check_conditions(g)
    run_mlse(g["y"], g["h"], g["c"], g["out"], [float(g["metric"])], g["cfg"]["states"], name)


@pytest.mark.parametrize("rid", sc.MLSE_ROW_IDS)
def test_mlse_row_matches_the_restatement(rid):
    y, h, c, want = sc.mlse_row(rid)
    y = np.array(y)
    cols = len(want)
    out = np.stack([c[w["index"]] for w in want], axis=1) if cols > 1 else c[want[0]["index"]]
    got, metrics = run_mlse(y, h, c, out, [w["metric"] for w in want], want[0]["states"], rid)
    if cols > 1:                              # a column alone is the 1-D call, bit for bit
        one = oa.mlse(np.ascontiguousarray(y[:, 1]), h, c)
        assert one.shape == (len(y),) and np.array_equal(one, got[:, 1]) and seqdet.last_call["final_metric"][0] == metrics[1]
    tail = sc.MLSE_ROWS[rid]["tail"]
    if tail:
        assert want[0]["final_state"] == (want[0]["states"] - 1 if tail == "last" else 0)


def test_mlse_takes_device_tables_and_narrows_real_ones():
    g = sc.load("mlse_pam4_L1")
    out = oa.mlse(g["y"], oa.to_device(g["h"].astype(np.complex128)), oa.to_device(g["c"].astype(np.complex128)))
    assert out.dtype == np.float64 and np.array_equal(out, g["out"])


def run_detector(r0, sigma2, c, px, rule, want_ind, want_decided, label):
    keep = r0.copy()
    results = {}
    for how in ("numpy", "device"):
        r = oa.to_device(r0) if how == "device" else r0
        before = device.transfer_counts()
        decided, ind = oa.detector(r, sigma2, c, px=px, rule=rule)
        again = oa.detector(r, sigma2, c, px=px, rule=rule)
        after = device.transfer_counts()
        tag = f"{label} [{how}]"
        kindof = oa.DeviceArray if how == "device" else np.ndarray
        assert type(decided) is kindof and type(ind) is kindof and decided.dtype == r0.dtype and ind.dtype == np.int64, tag
        assert decided.shape == r0.shape and ind.shape == r0.shape, tag
        if how == "device":
            assert after == before and np.array_equal(r.get(), keep), tag
        assert np.array_equal(r0, keep), tag
        decided, ind = host(decided), host(ind)
        assert np.array_equal(ind, want_ind) and np.array_equal(decided, want_decided), tag
        assert np.array_equal(host(again[0]), decided) and np.array_equal(host(again[1]), ind), tag
        results[how] = (decided, ind)
    assert all(np.array_equal(a, b) for a, b in zip(results["numpy"], results["device"])), label


@pytest.mark.parametrize("name", sc.DET_CASES)
def test_detector_fixture_through_numpy_and_device_arguments(name):
    g = sc.load(f"det_{name}")
    sc.check_conditions(g)
    cfg = g["cfg"]
    run_detector(g["r"], cfg["sigma2"], g["c"], g["px"] if cfg["has_px"] else None, cfg["rule"], g["ind"], g["decided"], name)


@pytest.mark.parametrize("rid", sc.DET_ROW_IDS)
def test_detector_row_matches_the_restatement(rid):
    r, sigma2, c, px, rule, want = sc.det_row(rid)
    run_detector(np.array(r), sigma2, c, px, rule, want, c[want].astype(r.dtype), rid)


def run_autocorr(x0, nTaps, label):
    keep = x0.copy()
    results = []
    for how in ("numpy", "device"):
        x = oa.to_device(x0) if how == "device" else x0
        before = device.transfer_counts()
        r, again, w = oa.autocorr(x, nTaps), oa.autocorr(x, nTaps), oa.estimateWhiteningFilter(x, nTaps)
        after = device.transfer_counts()
        assert type(r) is np.ndarray and type(w) is np.ndarray and w.dtype == np.float64 and w.shape == (nTaps,), label
        if how == "device":
            assert after == before and np.array_equal(x.get(), keep), label
        assert np.array_equal(x0, keep) and np.array_equal(again, r) and np.array_equal(w, oa.levinson(r, nTaps)), label
        sc.check_autocorr(r, x0, nTaps, f"{label} [{how}]")
        results.append((r, w))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]), label
    return results[0]


@pytest.mark.parametrize("name", sc.WHITE_CASES)
def test_whitening_fixture_through_numpy_and_device_arguments(name):
    g = sc.load(name)
    sc.check_conditions(g)
    r, w = run_autocorr(g["x"], g["cfg"]["nTaps"], name)
    d, dw = float(np.max(np.abs(r - g["r"])) / abs(g["r"][0])), float(np.max(np.abs(w - g["w"])) / np.max(np.abs(g["w"])))
    print(f"{name}: autocorr within {d:.2e} of r[0], w within {dw:.2e} of max |w|")
    assert d <= sc.TOL and dw <= sc.TOL


@pytest.mark.parametrize("i", range(len(sc.AC_ROWS)), ids=sc.AC_ROW_IDS)
def test_autocorr_row_matches_the_restatement(i):
    x, nTaps = sc.ac_row(i)
    run_autocorr(np.array(x), nTaps, sc.AC_ROW_IDS[i])


def test_chain_stays_on_the_device():
    """to_device(y) -> mlse -> fastBERcalc next to detector -> fastBERcalc on 2^14 PAM-4 symbols through h = (1, .6, .3, .1) at
    sigma = 0.2, with no transfer inside the calls.  y is built on the host (np.convolve plus noise), as the fixtures' inputs are;
    the device stages modulateGray -> pnorm -> firFilter -> awgn are not used."""
    rng = np.random.default_rng(21)
    n, h = 1 << 14, np.array([1, .6, .3, .1])
    c = oa.grayMapping(4, "pam").astype(np.float64)
    c = c / np.sqrt(np.mean(c ** 2))
    tx = c[rng.integers(0, 4, size=n)]
    y = np.convolve(tx, h)[:n] + 0.2 * rng.normal(size=n)
    yd, txd = oa.to_device(y), oa.to_device(tx)
    before = device.transfer_counts()
    sd = oa.mlse(yd, h, c)
    ber_m, ser_m, _ = oa.fastBERcalc(sd, txd, 4, "pam")
    dd, _ = oa.detector(yd, 0.04, c, rule="ML")
    ber_d, ser_d, _ = oa.fastBERcalc(dd, txd, 4, "pam")
    assert device.transfer_counts() == before and isinstance(sd, oa.DeviceArray) and isinstance(dd, oa.DeviceArray)
    print(f"chain: mlse BER {float(ber_m[0]):.4f} SER {float(ser_m[0]):.4f}; detector BER {float(ber_d[0]):.4f} SER {float(ser_d[0]):.4f}")
    assert float(ber_m[0]) < 0.05 and float(ber_d[0]) > 0.2
    assert seqdet.last_call["states"] == 64 and seqdet.last_call["kernel"] == "forward_wave64"
