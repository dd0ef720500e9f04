"""Link metrics on the GPU against the reference's recorded results (tests/golden/metrics/metrics_*.npz, tools/gen_golden_metrics.py),
through numpy arguments and through DeviceArrays (run with -m gpu).

Bounds: BER and SER are compared with == (error counts are integers and count / n is one division, as in the reference; the
fixtures guarantee a decision margin of 1e-6 so rounding cannot flip a decision); demodulated bits are equal; SNR [dB], GMI,
NGMI, MI and EVM (data-aided and blind) are within 1e-9 relative, the project's bound for double-precision receiver functions
against reference fixtures; pnorm within 1e-12 rel-L2 and signalPower within 1e-12 relative."""
import numpy as np
import pytest

import metrics_cases as mc
import opticommpy_amd as oa
from opticommpy_amd import device

pytestmark = pytest.mark.gpu

SEVEN = ("BER", "SER", "SNR", "GMI", "NGMI", "MI", "EVM")


def separate(rx, tx, M, ct, px, discard=0):
    """The reference-named functions, one call each."""
    BER, SER, SNR = oa.fastBERcalc(rx, tx, M, ct, px=px, discard=discard)
    GMI, NGMI = oa.monteCarloGMI(rx, tx, M, ct, px=px, discard=discard)
    MI = oa.monteCarloMI(rx, tx, M, ct, px=px, discard=discard)
    EVM = oa.calcEVM(rx, M, ct, symbTx=tx, discard=discard)
    return dict(BER=BER, SER=SER, SNR=SNR, GMI=GMI, NGMI=NGMI, MI=MI, EVM=EVM)


def rel_l2(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_metrics_match_the_reference(name, on_device):
    g = mc.load(name)
    mc.check_conditions(g)
    cfg = g["cfg"]
    M, ct, px, modes = cfg["M"], cfg["constType"], g["px"], mc.n_modes(g)
    rx0, tx0 = g["rx"].copy(), g["tx"].copy()
    rx, tx = (oa.to_device(rx0), oa.to_device(tx0)) if on_device else (rx0.copy(), tx0.copy())
    before = device.transfer_counts()

    sep = separate(rx, tx, M, ct, px)
    for k, v in sep.items():
        assert isinstance(v, np.ndarray) and v.shape == (modes,) and v.dtype == np.float64, k
    mc.compare(sep, g, "", name)
    blind = oa.calcEVM(rx, M, ct)
    mc.compare({"EVM_blind": blind}, g, "", name)

    # all seven from one library call: the separate functions' values bit for bit, as attributes and as entries
    m = oa.metrics(rx, tx, M, ct, px=px)
    assert sorted(m) == sorted(SEVEN)
    for k in SEVEN:
        assert np.array_equal(m[k], sep[k]) and getattr(m, k) is m[k], k

    # a second call repeats the first bit for bit (fixed-order reductions, no floating-point atomics)
    again = oa.metrics(rx, tx, M, ct, px=px)
    for k in SEVEN:
        assert np.array_equal(again[k], m[k]), k
    assert np.array_equal(oa.calcEVM(rx, M, ct), blind)

    # symbols [discard : n - discard] equal the reference called on that slice
    d = cfg["discard"]
    sep_d = separate(rx, tx, M, ct, px, discard=d)
    mc.compare(sep_d, g, "_d", name)
    mc.compare({"EVM_blind": oa.calcEVM(rx, M, ct, discard=d)}, g, "_d", name)
    m_d = oa.metrics(rx, tx, M, ct, px=px, discard=d)
    for k in SEVEN:
        assert np.array_equal(m_d[k], sep_d[k]), k

    # device arrays: nothing crossed the bus through DeviceArray.get / .set; inputs are unchanged either way
    if on_device:
        assert device.transfer_counts() == before
        assert np.array_equal(rx.get(), rx0) and np.array_equal(tx.get(), tx0)
    else:
        assert np.array_equal(rx, rx0) and np.array_equal(tx, tx0)


@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_numpy_and_device_arguments_agree_bit_for_bit(name):
    g = mc.load(name)
    cfg = g["cfg"]
    a = oa.metrics(g["rx"], g["tx"], cfg["M"], cfg["constType"], px=g["px"])
    b = oa.metrics(oa.to_device(g["rx"]), oa.to_device(g["tx"]), cfg["M"], cfg["constType"], px=g["px"])
    for k in SEVEN:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_demodulate_pnorm_and_signal_power(name):
    g = mc.load(name)
    cfg = g["cfg"]
    symb = mc.demod_input(g)
    bits = oa.demodulateGray(symb, cfg["M"], cfg["constType"])
    assert isinstance(bits, np.ndarray) and bits.dtype.kind == "i" and np.array_equal(bits, g["bits"])
    sd = oa.to_device(symb)
    before = device.transfer_counts()
    bits_d = oa.demodulateGray(sd, cfg["M"], cfg["constType"])
    assert device.transfer_counts() == before
    assert isinstance(bits_d, oa.DeviceArray) and bits_d.dtype.kind == "i" and np.array_equal(bits_d.get(), g["bits"])
    assert np.array_equal(sd.get(), symb)

    rx = g["rx"]
    wide = np.complex128 if np.iscomplexobj(rx) else np.float64
    want = rx.astype(wide) / float(g["pnorm_den"])
    y = oa.pnorm(rx)
    assert isinstance(y, np.ndarray) and y.shape == rx.shape and y.dtype == wide
    assert rel_l2(y, want) <= 1e-12
    assert rel_l2(y.reshape(-1)[:64], g["pnorm_head"]) <= 1e-12          # the reference's own output
    rd = oa.to_device(rx)
    before = device.transfer_counts()
    yd = oa.pnorm(rd)
    p = oa.signalPower(rd)
    assert device.transfer_counts() == before
    assert isinstance(yd, oa.DeviceArray) and yd.shape == rx.shape and np.array_equal(yd.get(), y)
    assert np.array_equal(rd.get(), rx)
    assert abs(p - float(g["signalPower"])) <= 1e-12 * float(g["signalPower"])
    assert oa.signalPower(rx) == p


def test_chain_on_the_device_without_host_copies():
    """The fixture's symbols -> to_device -> pnorm -> metrics: only the two uploads and nModes result records cross the bus."""
    g = mc.load("qam64_18dB")
    rx, tx = oa.to_device(g["rx"]), oa.to_device(g["tx"])
    before = device.transfer_counts()
    m = oa.metrics(oa.pnorm(rx), oa.pnorm(tx), 64, "qam")
    assert device.transfer_counts() == before
    # pnorm scales both arrays by constants: the error counts are those of the raw symbols, the rest moves by rounding only
    mc.compare({k: m[k] for k in SEVEN}, g, "", "chain")


def test_complex64_device_arrays_are_widened_on_load():
    g = mc.load("qam64_c64")
    assert g["rx"].dtype == np.complex64
    rx, tx = oa.to_device(g["rx"]), oa.to_device(g["tx"])
    assert rx.dtype == np.complex64
    mc.compare(dict(oa.metrics(rx, tx, 64, "qam")), g, "", "c64")
    with pytest.raises(TypeError):
        oa.metrics(rx, oa.to_device(g["tx"].astype(np.complex128)), 64, "qam")      # no hidden conversion on the device


def test_large_input_spans_many_workgroups_and_repeats():
    """2^18 symbols x 2 modes: the grid-stride loops, 512 partials per mode; repeated calls and numpy / device calls bit-equal; BER
    against a numpy count of the same decisions."""
    rng = np.random.default_rng(11)
    n = 1 << 18
    const = oa.grayMapping(16, "qam").astype(np.complex128) / np.sqrt(10)
    idx = rng.integers(0, 16, size=(n, 2))
    tx = const[idx]
    rx = (tx + (rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))) * np.sqrt(10 ** -1.2 / 2)) * 0.8 * np.exp(0.2j)
    a = oa.metrics(rx, tx, 16, "qam")
    rd, td = oa.to_device(rx), oa.to_device(tx)
    b = oa.metrics(rd, td, 16, "qam")
    c = oa.metrics(rd, td, 16, "qam")
    for k in SEVEN:
        assert np.array_equal(a[k], b[k]) and np.array_equal(b[k], c[k]), k
    for k in range(2):
        r = np.mean(tx[:, k] / rx[:, k]) * rx[:, k]
        r = r / np.sqrt(np.mean(np.abs(r) ** 2)) * np.sqrt(10)
        dec = np.argmin(np.abs(r[:, None] - oa.grayMapping(16, "qam")[None, :].astype(np.complex128)), axis=1)
        errs = np.sum(np.array([bin(v).count("1") for v in range(16)])[dec ^ idx[:, k]])
        assert a["BER"][k] == errs / (4 * n) and a["SER"][k] == np.mean(dec != idx[:, k])
    assert np.all(a["BER"] > 1e-2)
