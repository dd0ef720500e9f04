"""syncDataSequences, movingAverage and bert on the GPU (run with -m gpu): every fixture of tests/golden/syncdata/ against the
reference's recorded results and every row of tests/syncdata_shape_cases.py against tests/syncdata_restatement.py, through numpy
arguments and through DeviceArrays.

Bounds (tests/syncdata_cases.py): what is only moved equals the reference bit for bit, counts are equal, everything computed is within
1e-9 of the largest magnitude of the expected array.  numpy and DeviceArray calls give the same bits, a second call repeats the first,
inputs are never written, and with DeviceArray arguments nothing goes through DeviceArray.get / .set."""
import numpy as np
import pytest

import opticommpy_amd as oa
import syncdata_cases as sc
import syncdata_restatement as rs
import syncdata_shape_cases as ssc
from opticommpy_amd import device, synchronization

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def both_ways(call, arrays, staged=False):
    """call(*arrays) with numpy arguments and with DeviceArrays, twice each: {kind: tuple of host results}.  Asserts the types, the
    transfer counts (``staged``: numpy arguments go through the library's own staging buffers, which DeviceArray's counters do not
    see), that inputs are unchanged, that a second call repeats the first and that both kinds agree bit for bit."""
    results = {}
    for kind in ("numpy", "device"):
        args = [oa.to_device(a) if kind == "device" else a.copy() for a in arrays]
        before = device.transfer_counts()
        out = call(*args)
        out2 = call(*args)
        after = device.transfer_counts()
        out, out2 = (out if isinstance(out, tuple) else (out,)), (out2 if isinstance(out2, tuple) else (out2,))
        for o in out:
            assert type(o) is (oa.DeviceArray if kind == "device" else np.ndarray), kind
        if kind == "device":
            assert after == before, (before, after)                 # no array crosses the bus inside the calls
            for a, d in zip(arrays, args):
                assert np.array_equal(d.get(), a)
        else:
            if staged:
                assert after == before
            else:                             # every input uploaded once and every output downloaded once, per call
                assert after["h2d"] == before["h2d"] + 2 * len(arrays) and after["d2h"] == before["d2h"] + 2 * len(out)
            for a, d in zip(arrays, args):
                assert np.array_equal(d, a)
        results[kind] = tuple(host(o) for o in out)
        for a, b in zip(results[kind], (host(o) for o in out2)):
            assert a.tobytes() == b.tobytes(), kind
    for a, b in zip(results["numpy"], results["device"]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return results["device"]


# ------------------------------------------------------------------ syncDataSequences
def check_sync(label, got_tx, got_symb, want_tx, want_symb, moved, reference, tol=sc.TOL):
    assert got_tx.dtype == want_tx.dtype and got_symb.dtype == want_symb.dtype, label
    e_tx, ok_tx = sc.close(got_tx, want_tx, tol)
    e_sy, ok_sy = sc.close(got_symb, want_symb, tol)
    print(f"{label}: tx_ {e_tx:.2e}  symb {e_sy:.2e}")
    assert ok_tx and ok_sy, (label, e_tx, e_sy)
    if reference == "signal":
        assert np.array_equal(got_tx, np.asarray(moved).reshape(got_tx.shape)), label                 # only moved: bit for bit (up to the sign of zeros)


@pytest.mark.parametrize("name", sc.SYNC_CASES)
def test_sync_fixtures(name):
    g = sc.load(name)
    sc.check_conditions(g)
    cfg = g["cfg"]
    p = sc.param_of(cfg)
    tx_, symb = both_ways(lambda rx, tx: oa.syncDataSequences(rx, tx, p), [g["rx"], g["tx"]])
    real = g["rx"].dtype.kind != "c" and g["tx"].dtype.kind != "c"
    wide = np.float64 if real else np.complex128
    assert tx_.shape == g["tx_"].shape and symb.shape == g["symb"].shape
    # the reference (single precision for the complex64 case: held at cfg["ref_tol"]) and the restatement in double at 1e-9
    check_sync(f"{name} vs reference", tx_, symb, g["tx_"].astype(wide), g["symb"].astype(wide), g["tx_"].astype(wide), cfg["reference"],
               cfg["ref_tol"])
    r_tx, r_symb, info = sc.restate(g["rx"], g["tx"], p)
    check_sync(f"{name} vs restatement", tx_, symb, r_tx, r_symb, info.moved, cfg["reference"])
    last = synchronization.last_call
    assert np.array_equal(last["info"].delay, info.sync.delay) and np.array_equal(last["info"].swap, info.sync.swap) and last["padL"] == info.padL
    if cfg["reference"] == "symbols":
        assert np.array_equal(last["kept"], g["kept"])


@pytest.mark.parametrize("row", ssc.SYNC_ROWS, ids=lambda r: r["name"])
def test_sync_rows(row):
    rx, tx = ssc.sync_input(row)
    p = ssc.sync_param(row)
    r_tx, r_symb, info = sc.restate(rx, tx, p)
    real = rx.dtype.kind != "c" and tx.dtype.kind != "c"
    sc.check_info(info, row["reference"], real_mode_on_real=real and row["syncMode"] == "real")
    tx_, symb = both_ways(lambda a, b: oa.syncDataSequences(a, b, p), [rx, tx])
    assert tx_.shape == rx.shape and symb.shape == r_symb.shape
    check_sync(row["name"], tx_, symb, r_tx, r_symb, info.moved, row["reference"])
    if row["reference"] == "symbols":
        assert np.array_equal(synchronization.last_call["kept"], info.kept)
    # one side on the device is enough for DeviceArrays
    m_tx, m_symb = oa.syncDataSequences(oa.to_device(rx), tx, p)
    assert isinstance(m_tx, oa.DeviceArray) and m_tx.get().tobytes() == tx_.tobytes() and m_symb.get().tobytes() == symb.tobytes()


@pytest.mark.parametrize("row", ssc.TILE_ROWS, ids=lambda r: r["name"])
def test_tile_rows(row):
    rx, tx = ssc.tile_input(row)
    want_tx, padL = rs.tile(tx, len(rx), row["SpS"])
    before = device.transfer_counts()
    rxd, txd = oa.to_device(rx), oa.to_device(tx)
    rx_pad, tx_rep = synchronization._tile(rxd, txd, len(rx) + padL, row["SpS"])
    assert device.transfer_counts()["d2h"] == before["d2h"]
    got_rx, got_tx = rx_pad.get(), tx_rep.get()
    assert got_tx.dtype == got_rx.dtype == np.complex128 and np.array_equal(got_tx, want_tx.astype(np.complex128))
    assert np.array_equal(got_rx[:len(rx)], rx.astype(np.complex128)) and not np.any(got_rx[len(rx):])
    assert np.array_equal(rxd.get(), rx) and np.array_equal(txd.get(), tx)


@pytest.mark.parametrize("n, src_cols, first, width, dst_cols, at", [(1, 1, 0, 1, 1, 0), (257, 8, 4, 4, 4, 0), (1000, 3, 1, 2, 7, 5), (70000, 7, 4, 3, 3, 0)])
def test_copy_columns(n, src_cols, first, width, dst_cols, at):
    """A block of columns lands bit for bit where it is asked for and nothing else of the destination changes."""
    from opticommpy_amd import _lib
    from opticommpy_amd.models import _state
    rng = np.random.default_rng(n + width)
    src = rng.normal(size=(n, src_cols)) + 1j * rng.normal(size=(n, src_cols))
    dst = rng.normal(size=(n, dst_cols)) + 1j * rng.normal(size=(n, dst_cols))
    sd, dd = oa.to_device(src), oa.to_device(dst)
    synchronization._copy_columns(_lib.load(), _state["device"], sd, first, width, dd, at)
    want = dst.copy()
    want[:, at:at + width] = src[:, first:first + width]
    assert np.array_equal(dd.get(), want) and np.array_equal(sd.get(), src)
    with pytest.raises(ValueError, match="inside both arrays"):
        synchronization._copy_columns(_lib.load(), _state["device"], sd, src_cols, 1, dd, 0)


@pytest.mark.parametrize("row", ssc.EXTRACT_ROWS, ids=lambda r: r["name"])
def test_extract_rows(row):
    x = ssc.extract_input(row)
    n_out = row["n"] // row["SpS"] + 1
    moved, symb, kept = rs.extract(x, n_out)
    xd = oa.to_device(x)
    before = device.transfer_counts()
    got_moved, k0 = synchronization._extract(xd, n_out, False, normalize=False)
    got, k1 = synchronization._extract(xd, n_out, False)
    again, _ = synchronization._extract(xd, n_out, False)
    got_real, _ = synchronization._extract(xd, n_out, True)
    short, k2 = synchronization._extract(xd, max(1, n_out // 2), False, normalize=False)
    assert device.transfer_counts() == before
    assert np.array_equal(k0, kept) and np.array_equal(k1, kept) and np.array_equal(k2, kept)
    assert np.array_equal(got_moved.get(), moved)                    # only moved: bit for bit
    e, ok = sc.close(got.get(), symb)
    print(f"{row['name']}: {e:.2e}")
    assert ok, e
    assert got.get().tobytes() == again.get().tobytes() and np.array_equal(got_real.get(), got.get().real)
    assert np.array_equal(short.get(), moved[:max(1, n_out // 2)])   # a shorter output drops what is beyond it
    assert np.array_equal(xd.get(), x)


# ------------------------------------------------------------------ movingAverage
@pytest.mark.parametrize("name", sc.MA_CASES)
def test_moving_average_fixtures(name):
    g = sc.load(name)
    sc.check_conditions(g)
    (y,) = both_ways(lambda x: oa.movingAverage(x, g["cfg"]["N"]), [g["x"]], staged=True)
    e, ok = sc.close(y, g["y"])
    print(f"{name}: {e:.2e}")
    assert ok and y.dtype == g["y"].dtype, e


@pytest.mark.parametrize("row", ssc.MA_ROWS, ids=lambda r: f"n{r['n']}_N{r['N']}_{r['cols']}x{r['dtype']}")
def test_moving_average_rows(row):
    x = ssc.ma_input(row)
    want = rs.moving_average_direct(x, row["N"])
    (y,) = both_ways(lambda a: oa.movingAverage(a, row["N"]), [x], staged=True)
    assert y.dtype == (np.float64 if x.dtype.kind == "f" else np.complex128) and y.shape == x.shape
    e, ok = sc.close(y, want)
    print(f"n {row['n']} N {row['N']}: {e:.2e}")
    assert ok, e


# ------------------------------------------------------------------ bert
def check_bert(label, Irx, bits, given=True, seed=123):
    """bert with numpy and with DeviceArray arguments against the restatement: (BER, Q)."""
    _, _, want = rs.bert(Irx, bits)
    unsure = int(np.count_nonzero(np.abs(Irx - want.Id) < sc.ID_GAP * np.max(np.abs(Irx))))
    res = []
    for kind in ("numpy", "device"):
        x = oa.to_device(Irx) if kind == "device" else Irx.copy()
        b = None if not given else (oa.to_device(np.ascontiguousarray(bits == 1, dtype=np.uint8)) if kind == "device" else bits.copy())
        before = device.transfer_counts()
        BER, Q = oa.bert(x, b, seed=seed) if b is not None else oa.bert(x, seed=seed)
        BER2, Q2 = oa.bert(x, b, seed=seed) if b is not None else oa.bert(x, seed=seed)
        assert device.transfer_counts() == before, kind              # only the scalars cross the bus
        assert type(BER) is float and type(Q) is float and (BER, Q) == (BER2, Q2)
        assert np.array_equal(host(x), Irx)
        s = oa.bert.last
        assert (s["n1"], s["n0"]) == (want.n1, want.n0) and abs(s["errors"] - want.errors) <= unsure and BER == s["errors"] / len(Irx)
        errs = [abs(s[k] - getattr(want, k)) / max(abs(getattr(want, k)), 1e-300) for k in ("I1", "I0", "Id", "Q")]
        errs += [abs(s[k] - getattr(want, k)) / max(want.std1, want.std0) for k in ("std1", "std0")]
        print(f"{label} [{kind}]: {max(errs):.2e}")
        assert max(errs) <= sc.TOL, (label, errs)
        res.append((BER, Q))
    assert res[0] == res[1]
    return res[0], unsure


@pytest.mark.parametrize("name", sc.BERT_CASES)
def test_bert_fixtures(name):
    g = sc.load(name)
    sc.check_conditions(g)
    cfg = g["cfg"]
    np.random.seed(cfg["seed"])
    bits = np.random.randint(2, size=g["Irx"].size) if cfg["drawn"] else g["bits"]
    (BER, Q), unsure = check_bert(name, g["Irx"], bits, given=not cfg["drawn"], seed=cfg["seed"])
    assert unsure == 0 and round(BER * g["Irx"].size) == int(g["errors"]) and BER == float(g["BER"])    # integer results are equal
    assert abs(Q - float(g["Q"])) <= sc.TOL * abs(float(g["Q"]))


@pytest.mark.parametrize("row", ssc.BERT_ROWS, ids=lambda r: f"n{r['n']}_{r['ones']}_{r['bits_dtype']}")
def test_bert_rows(row):
    Irx, bits = ssc.bert_input(row)
    check_bert(f"n {row['n']}", Irx, bits)


def test_bert_reads_device_bits_as_the_host_does():
    """A bit is 1 where it equals 1: a byte array with other values gives the same result from the host and from the device."""
    Irx, bits = ssc.bert_input(ssc.BERT_ROWS[2])
    odd = bits.astype(np.uint8)
    odd[::7] = 2
    want = oa.bert(Irx, odd)
    assert oa.bert(oa.to_device(Irx), oa.to_device(odd)) == want == oa.bert(Irx, (odd == 1).astype(np.int64))
    assert oa.bert.last["n1"] == int(np.count_nonzero(odd == 1))


def test_bert_reports_an_empty_class_on_the_device():
    Irx = oa.to_device(np.linspace(0.0, 1.0, 300))
    with pytest.raises(ValueError, match="only one of the two classes"):
        oa.bert(Irx, oa.to_device(np.zeros(300, dtype=np.uint8)))


# ------------------------------------------------------------------ chain
def test_imdd_chain_stays_on_the_device():
    """pamTransmitter -> balancedPD -> pnorm -> syncDataSequences -> ffe -> pnorm -> fastBERcalc on DeviceArrays with no host copy in
    between; ``symb`` of syncDataSequences is ffe's reference and fastBERcalc's transmitted sequence, and the transmitted symbols are
    handed over rotated by 321 symbols, which the synchroniser has to undo.

    (The reference's chain has resample between photodiode and the synchroniser.  This package's resample filters complex128
    DeviceArrays only and refuses the photodiode's float64 one -- tests/test_gpu_clock.py -- and ffe takes a PAM table with real data
    only, so the field is made at the equalizer's two samples per symbol and the chain on the device goes without it, as
    tests/test_gpu_siso.py's does.  The second photodiode of the balanced pair, fed the unmodulated carrier, takes off the mean of the
    intensity, which the notebook subtracts on the host.)

    Bounds: the symbols equal the transmitted ones over their root mean square within 1e-9 (they are moved and divided once); the
    channel is noiseless with mild inter-symbol interference (a photodiode of 0.9 Rs bandwidth), so after 1000 training symbols the
    equalised eye is open: BER <= 1e-2 over the symbols past the training, the bound of tests/test_gpu_siso.py's chain."""
    import types
    Rs, sps, nsym, shift = 10e9, 2, 4000, 321
    ptx = types.SimpleNamespace(M=4, Rs=Rs, SpS=sps, nBits=2 * nsym, pulseType="nrz", seed=5, power=-3, nFilterTaps=64)
    sig, symbTx = oa.pamTransmitter(ptx, device_output=True)
    assert isinstance(sig, oa.DeviceArray) and sig.shape == (nsym * sps,) and symbTx.shape[0] == nsym
    symbols = np.ascontiguousarray(np.asarray(symbTx, dtype=np.float64).reshape(-1))
    carrier = oa.to_device(np.full(nsym * sps, np.sqrt(oa.signalPower(sig)), dtype=np.complex128))
    txd = oa.to_device(np.roll(symbols, shift))
    pd = types.SimpleNamespace(Fs=sps * Rs, B=0.9 * Rs, ideal=False, shotNoise=False, thermalNoise=False, seed=1, N=65)
    eq = types.SimpleNamespace(nTaps=11, SpS=sps, mu=5e-3, nTrain=1000, M=4, constType="pam", prec=np.float64)
    ps = types.SimpleNamespace(SpS=sps, reference="symbols", syncMode="amp", nFilterTaps=256)

    before = device.transfer_counts()
    rx = oa.pnorm(oa.balancedPD(sig, carrier, pd))
    tx_, symb = oa.syncDataSequences(rx, txd, ps)
    ref = synchronization._head(symb, nsym).reshape(-1)              # symb carries one more row than there are symbols: a view without it
    y, f, mse = oa.ffe(rx, ref, eq)
    y = oa.pnorm(y)
    BER, SER, SNR = oa.fastBERcalc(y, ref, 4, "pam", discard=1100)
    curve = oa.movingAverage(mse, 500)
    assert device.transfer_counts() == before
    for a in (rx, tx_, symb, y, curve):
        assert isinstance(a, oa.DeviceArray)
    assert tx_.shape == rx.shape and symb.shape == (nsym + 1, 1) and symb.dtype == tx_.dtype == np.float64 and curve.shape == mse.shape
    info = synchronization.last_call
    delay = int(info["info"].delay[0])
    assert abs(delay % (nsym * sps) - shift * sps) <= 1 and info["kept"].tolist() == [nsym] and info["padL"] == 0
    got = symb.get()
    stuffed = np.zeros(nsym * sps)
    stuffed[::sps] = np.roll(symbols, shift)
    moved = np.roll(stuffed, -delay)
    e, ok = sc.close(got[:nsym, 0], moved[moved != 0] / np.sqrt(np.mean(symbols ** 2)))
    print(f"IM/DD chain: symb {e:.2e}  BER {float(BER[0]):.3e}  SNR {float(SNR[0]):.1f} dB  last MSE {float(curve.get()[-300]):.2e}")
    assert ok and got[nsym, 0] == 0.0
    assert float(BER[0]) <= 1e-2
