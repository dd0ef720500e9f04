"""Host side of syncDataSequences / movingAverage / bert / theoryBER / Qfunc without a GPU: exports and the reference's module names,
every refusal with its message (all raised before the library is touched), the host-side closed forms against recorded values of
the reference's expressions, the layout of ssf_sync_tile_params against its ctypes mirror and the constants against the header."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest

import opticommpy_amd as oa
import syncdata_cases as sc
import syncdata_shape_cases as ssc
from opticommpy_amd import _lib, core, metrics, synchronization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX = np.linspace(-1.0, 1.0, 40)
TX = np.array([1.0, -1.0, 3.0, -3.0] * 5) / 3


class FakeDevice(oa.DeviceArray):
    """A DeviceArray that owns no memory: the refusals come before any pointer is read."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.device, self._ptr, self._owner = tuple(shape), np.dtype(dtype), 0, C.c_void_p(), self


def P(**k):
    return types.SimpleNamespace(**k)


def test_public_names():
    for name in ("syncDataSequences", "movingAverage", "bert", "theoryBER", "Qfunc"):
        assert getattr(oa, name) is getattr(synchronization, name) and name in oa.__all__ and name in synchronization.__all__
    assert core.movingAverage is synchronization.movingAverage
    for name in ("bert", "theoryBER", "Qfunc"):
        assert getattr(metrics, name) is getattr(synchronization, name)
    # the reference's notebooks import these names from these modules
    from opticommpy_amd.core import movingAverage  # noqa: F401
    from opticommpy_amd.metrics import bert, theoryBER  # noqa: F401
    from opticommpy_amd.synchronization import syncDataSequences  # noqa: F401
    assert isinstance(synchronization.last_call, dict)


def test_constants_follow_the_header():
    text = open(os.path.join(ROOT, "opticommpy_amd", "csrc", "syncdata_kernels.h")).read()

    def const(name):
        return int(re.search(rf"\b{name} = (\d+)", text).group(1))
    assert const("kBlock") == _lib.SYNCDATA_BLOCK == ssc.BLOCK and const("kItems") * const("kBlock") == _lib.SYNCDATA_SPAN == ssc.B
    assert const("kMaTile") == _lib.SYNCDATA_MA_TILE == ssc.T and const("kMaMaxN") == _lib.SYNCDATA_MA_MAX_N == synchronization.MAX_N
    assert const("kBertMaxBlocks") == _lib.SYNCDATA_BERT_BLOCKS == ssc.BERT_BLOCKS and const("kMaxModes") == _lib.SYNC_MAX_MODES
    assert C.sizeof(_lib.SyncTileParams) == 40
    header = open(os.path.join(ROOT, "include", "ssf.h")).read()
    for name in ("ssf_sync_tile", "ssf_sync_extract", "ssf_real_part", "ssf_copy_columns", "ssf_moving_average", "ssf_bert"):
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header)


SYNC_REFUSALS = [
    (RX, TX, P(reference="waveform"), ValueError, "reference must be 'signal' or 'symbols'"),
    (RX, TX, P(syncMode="phase"), ValueError, "syncMode must be 'amp' or 'real'"),
    (RX, TX, P(SpS=0), ValueError, "SpS = 0"),
    (RX, TX, P(SpS=1.5), ValueError, "SpS = 1.5"),
    (np.zeros((40, 9)), np.zeros((20, 9)), P(), ValueError, "9 modes"),
    (np.zeros((40, 2)), np.zeros((20, 3)), P(), ValueError, "rx has 2 modes and tx 3"),
    (RX, TX, P(reference="symbols", pulseType="gauss"), ValueError, "pulseType must be"),
    (RX, TX, P(reference="symbols", nFilterTaps=0), ValueError, "nFilterTaps = 0"),
    (RX, TX, P(reference="symbols", nFilterTaps=12.5), ValueError, "nFilterTaps = 12.5"),
    (RX[:1], TX, P(), ValueError, "at least 2 are needed"),
    (RX, TX[:1], P(), ValueError, "at least 2 are needed"),
    (np.zeros((2, 2, 2)), TX, P(), ValueError, "rx must have one or two dimensions"),
    (RX, np.zeros((2, 2, 2)), P(), ValueError, "tx must have one or two dimensions"),
    (RX.astype(np.complex128), TX, P(syncMode="real"), ValueError, "a real tx against a complex rx in syncMode 'real'"),
    (RX, TX, P(M=5), ValueError, "M must be a power of two"),
    (RX, TX, P(constType="apsk"), ValueError, "constType must be"),
    (np.array(["a", "b"]), TX, P(), TypeError, "numbers expected"),
    (FakeDevice((40,), np.float32), TX, P(), TypeError, "complex128, complex64 or float64 expected"),
    (RX, FakeDevice((20,), np.int64), P(), TypeError, "complex128, complex64 or float64 expected"),
]


@pytest.mark.parametrize("i", range(len(SYNC_REFUSALS)))
def test_sync_data_sequences_refuses_before_anything_runs(i, monkeypatch):
    rx, tx, p, exc, text = SYNC_REFUSALS[i]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(exc) as e:
        oa.syncDataSequences(rx, tx, p)
    assert text in str(e.value)


def test_eight_modes_under_both_references():
    """8 modes pass the checks under 'symbols' and under 'signal', where decimate's six columns at 41 samples per symbol are met by
    decimating in groups."""
    assert synchronization.MAX_MODES == 8 and synchronization.DECIMATE_MODES == 6 == 256 // 41
    assert synchronization._prepare_sync(np.zeros((40, 8)), np.zeros((20, 8)), P(reference="symbols", nFilterTaps=16)).modes == 8
    assert synchronization._prepare_sync(np.zeros((40, 8)), np.zeros((20, 8)), P()).modes == 8


def test_sync_host_quantities():
    q = synchronization._prepare_sync(RX, TX, P(SpS=3, reference="symbols"))
    assert (q.period, q.repeats, q.n_pad, q.stuff, q.real_out, q.input1D) == (60, 1, 60, 3, True, True)
    q = synchronization._prepare_sync(np.zeros((121, 2), dtype=np.complex64), np.zeros((20, 2)), P(SpS=3))
    assert (q.period, q.repeats, q.n_pad, q.stuff, q.real_out, q.input1D, q.M, q.syncMode) == (20, 7, 140, 1, False, False, 4, "amp")


MA_REFUSALS = [
    (RX, 1, ValueError, "N = 1"),
    (RX, 0, ValueError, "N = 0"),
    (RX, 2.5, ValueError, "N = 2.5"),
    (RX, 2049, ValueError, "at most 2048"),
    (np.zeros((2, 2, 2)), 3, ValueError, "one or two dimensions"),
    (np.zeros(0), 3, ValueError, "at least one row"),
    (FakeDevice((40,), np.float32), 3, TypeError, "complex128, complex64 or float64 expected"),
]


@pytest.mark.parametrize("i", range(len(MA_REFUSALS)))
def test_moving_average_refuses_before_anything_runs(i, monkeypatch):
    x, N, exc, text = MA_REFUSALS[i]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(exc) as e:
        oa.movingAverage(x, N)
    assert text in str(e.value)


BITS = np.array([0, 1] * 20)
BERT_REFUSALS = [
    (RX, np.zeros(40, dtype=np.int64), ValueError, "only one of the two classes"),
    (RX, np.ones(40, dtype=bool), ValueError, "only one of the two classes"),
    (RX, BITS[:39], ValueError, "40 samples and bitsTx 39 bits"),
    (RX.astype(np.complex128), BITS, TypeError, "Irx must be real"),
    (RX, BITS.astype(np.float64), TypeError, "bitsTx has dtype float64"),
    (np.zeros(0), None, ValueError, "Irx is empty"),
    (FakeDevice((40,), np.float32), BITS, TypeError, "float64 expected"),
    (RX, FakeDevice((40,), np.int64), TypeError, "one byte per bit"),
]


@pytest.mark.parametrize("i", range(len(BERT_REFUSALS)))
def test_bert_refuses_before_anything_runs(i, monkeypatch):
    Irx, bits, exc, text = BERT_REFUSALS[i]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    with pytest.raises(exc) as e:
        oa.bert(Irx, bits)
    assert text in str(e.value)


def test_bert_draws_the_reference_bits():
    """Without bitsTx the bits are numpy's draws under the seed, as the reference takes them; every accepted dtype is converted once."""
    Irx, bits, n = synchronization._prepare_bert(RX, None, 77)
    np.random.seed(77)
    assert np.array_equal(bits, np.random.randint(2, size=40)) and bits.dtype == np.uint8 and n == 40
    for dt in ("int8", "uint8", "int32", "int64", "bool"):
        assert np.array_equal(synchronization._prepare_bert(RX, BITS.astype(dt), 1)[1], BITS)


def test_closed_forms():
    """Qfunc is 0.5 - 0.5 erf(x / sqrt 2); theoryBER the reference's three expressions (optic/comm/metrics.py:669-686), evaluated here
    with math.erf term by term."""
    def Q(x):
        return 0.5 - 0.5 * math.erf(x / math.sqrt(2))
    for x in (-3.0, -0.5, 0.0, 0.3, 1.0, 2.5, 6.0):
        assert abs(oa.Qfunc(x) - Q(x)) <= 1e-15
    assert oa.Qfunc(0.0) == 0.5 and np.allclose(oa.Qfunc(np.array([0.0, 1.0])), [0.5, Q(1.0)], rtol=0, atol=1e-15)
    for EbN0 in (0.0, 4.0, 9.5, 14.0):
        lin = 10 ** (EbN0 / 10)
        for M in (4, 16, 64):
            L = math.sqrt(M)
            want = 2 * (1 - 1 / L) / math.log2(L) * Q(math.sqrt(3 * math.log2(L) / (L**2 - 1) * (2 * lin)))
            assert abs(oa.theoryBER(M, EbN0, "qam") - want) <= 1e-15
        for M in (2, 4, 8):
            k = math.log2(M)
            assert abs(oa.theoryBER(M, EbN0, "psk") - 2 * Q(math.sqrt(2 * k * lin) * math.sin(math.pi / M)) / k) <= 1e-15
            want = (2 * (M - 1) / M) * Q(math.sqrt(6 * math.log2(M) / (M**2 - 1) * lin)) / k
            assert abs(oa.theoryBER(M, EbN0, "pam") - want) <= 1e-15
    with pytest.raises(ValueError):
        oa.theoryBER(4, 3.0, "apsk")
    # ... and against the reference's own values (tests/golden/syncdata/closed_forms.npz)
    g = sc.load("closed_forms")
    assert np.max(np.abs(oa.Qfunc(g["x"]) - g["Q"])) <= 1e-15
    for (M, ct), row in zip(g["cfg"]["rows"], g["ber"]):
        for e, want in zip(g["EbN0"], row):
            assert abs(oa.theoryBER(M, float(e), ct) - want) <= 1e-15, (M, ct, e)
