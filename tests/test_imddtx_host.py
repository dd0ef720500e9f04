"""Host side of the IM/DD transmitter and the AWGN channel, without a GPU: the sources bit for bit, the defaults and their
write-back, the draw order and where numpy's global stream is left, and every refusal -- raised before the library is reached (a
backend that fails the test stands in its place)."""
import numpy as np
import pytest

import imddtx_cases as ic
import opticommpy_amd as oa
from opticommpy_amd import channels, core, devices, imddtx, sources, tx
from opticommpy_amd.device import DeviceArray


class Recorder:
    """Stands in the library's place: records the calls, fills the outputs with zeros."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            out = args[3] if name == "awgn" else args[-1]
            out[...] = 0
        return call


class Unreachable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(imddtx, "_backend", r)
    return r


@pytest.fixture
def unreachable(monkeypatch):
    monkeypatch.setattr(imddtx, "_backend", Unreachable())


def fake_device(shape, dtype):
    """A DeviceArray that owns no memory: enough for the checks that come before any library call."""
    d = object.__new__(DeviceArray)
    d.shape, d.dtype, d.device, d._ptr, d._owner = tuple(shape), np.dtype(dtype), 0, None, d
    return d


def test_exports():
    names = ["pamTransmitter", "mzm", "pm", "iqm", "voa", "upsample", "awgn", "bitSource", "prbsGenerator", "symbolSource"]
    for n in names:
        assert getattr(oa, n) is getattr(imddtx, n) and n in oa.__all__
    assert tx.pamTransmitter is oa.pamTransmitter and tx.simpleWDMTx is oa.simpleWDMTx
    assert devices.mzm is oa.mzm and devices.pm is oa.pm and devices.iqm is oa.iqm and devices.voa is oa.voa and devices.photodiode is oa.photodiode
    assert channels.awgn is oa.awgn and channels.linearFiberChannel is oa.linearFiberChannel
    assert core.upsample is oa.upsample and core.firFilter is oa.firFilter and core.pnorm is oa.pnorm
    assert sources.bitSource is oa.bitSource and sources.symbolSource is oa.symbolSource and sources.prbsGenerator is oa.prbsGenerator


def test_sources_equal_the_reference_bit_for_bit():
    g = ic.load("sources")
    rows = g["cfg"]["rows"]
    for name, d in rows["bits"].items():
        got = oa.bitSource(ic.make_param(d))
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    assert np.array_equal(oa.prbsGenerator(7, None, 1), g["prbs7_full"]) and len(g["prbs7_full"]) == 127
    assert np.array_equal(oa.prbsGenerator(23, 2500, 9), g["prbs23_head"])
    assert len(np.unique(g["bits_prbs23"])) == 2 and len(np.unique(g["bits_prbs7"])) == 2
    for name, d in rows["symbols"].items():
        got = oa.symbolSource(ic.make_param(d))
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    for bad in (dict(order=8), dict(seed=0), dict(seed=-3)):
        with pytest.raises(ValueError):
            oa.prbsGenerator(**dict(dict(order=7, length=10, seed=1), **bad))
    with pytest.raises(ValueError):
        oa.bitSource(ic.make_param(dict(mode="gold")))
    with pytest.raises(ValueError):
        oa.symbolSource(ic.make_param(dict(dist="gaussian")))


def test_normal_is_scale_times_standard_normal():
    """What lets the host draw unit normals while the device reduces the power: element for element, from the same stream."""
    for s, shape in ((0.37, (1001,)), (3.1e-4, (333, 2)), (np.sqrt(0.123 / 2), (5,))):
        np.random.seed(99)
        a = np.random.normal(0, s, shape)
        a2 = np.random.normal(0, s, shape)
        state = np.random.get_state()
        np.random.seed(99)
        b = s * np.random.standard_normal(shape)
        b2 = s * np.random.standard_normal(shape)
        assert np.array_equal(a, b) and np.array_equal(a2, b2)
        assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))


def test_pam_defaults_are_the_code_s_and_are_written_back(rec):
    p = oa.parameters()
    p.nBits, p.seed = 64, 3
    sig, symb = oa.pamTransmitter(p)
    want = dict(M=4, Rs=32e9, SpS=16, probDist="uniform", shapingFactor=0, seed=3, nBits=64, pulseType="nrz", nFilterTaps=256,
                pulseRollOff=0.01, mzmVpi=3, mzmVb=1.5, mzmER=80, mzmScale=0.25, nPolModes=1, power=-3, returnParam=False)
    assert vars(p) == want
    g = ic.load("pam_default")
    assert {k: v for k, v in ic.json.loads(str(g["written"])).items()} == dict(want, nBits=2048, seed=11)
    assert sig.shape == (32 * 16,) and sig.dtype == np.complex128 and symb.shape == (32, 1) and symb.dtype == np.float64
    (name, a), = rec.calls
    assert name == "pam_tx" and a[:3] == (32, 16, 1) and a[5:10] == (0.25, 3.0, -1.5, 80.0, float(np.sqrt(1e-3 * 10 ** (-3 / 10))))
    assert a[4].shape == (1, 32) and np.array_equal(a[4][0], symb[:, 0])


def test_pam_draws_and_global_stream(rec):
    for case in ("pol2", "mb", "retparam"):
        g = ic.load("pam_" + case)
        d = g["cfg"]["param"]
        res = oa.pamTransmitter(ic.make_param(d))
        assert np.array_equal(res[1], g["symbTx"]), case
        assert (len(res) == 3) == bool(d.get("returnParam", False))
        if len(res) == 3:
            assert res[2].power == d["power"]
        after = np.random.get_state()
        # the reference's last draw is the last mode's symbol source under seed + nPolModes - 1
        np.random.seed(d["seed"] + d.get("nPolModes", 1) - 1)
        oa.symbolSource(ic.make_param(dict(nSymbols=g["symbTx"].shape[0], M=d.get("M", 4), constType="pam", dist=d.get("probDist", "uniform"),
                                           shapingFactor=d.get("shapingFactor", 0))))
        assert all(np.array_equal(x, y) for x, y in zip(after, np.random.get_state())), case
    # without a seed the symbols come from the global stream as it stands
    np.random.seed(1234)
    _, a = oa.pamTransmitter(ic.make_param(dict(nBits=40, nPolModes=2)))
    np.random.seed(1234)
    b0 = oa.symbolSource(ic.make_param(dict(nSymbols=20, M=4, constType="pam")))
    b1 = oa.symbolSource(ic.make_param(dict(nSymbols=20, M=4, constType="pam")))
    assert np.array_equal(a[:, 0], b0) and np.array_equal(a[:, 1], b1)


@pytest.mark.parametrize("bad,exc", [
    (dict(M=3), ValueError), (dict(M=6), ValueError), (dict(M=1), ValueError), (dict(M=4.0), ValueError), (dict(nBits=1), ValueError),
    (dict(nBits=0), ValueError), (dict(M=8, nBits=2), ValueError), (dict(pulseType="rrc", nFilterTaps=4097), ValueError),
    (dict(pulseType="nrz", SpS=3000), ValueError), (dict(pulseType="gauss"), ValueError), (dict(probDist="poisson"), ValueError),
    (dict(SpS=0), ValueError), (dict(nPolModes=0), ValueError), (dict(mzmVpi=0), ValueError)])
def test_pam_refusals(unreachable, bad, exc):
    with pytest.raises(exc):
        oa.pamTransmitter(ic.make_param(dict(dict(nBits=64, seed=1), **bad)))


def test_modulator_argument_rules(rec):
    u = np.linspace(-1, 1, 12)
    out = oa.mzm(1, u)
    (name, a), = rec.calls
    assert name == "modulate" and a[0] == "mzm" and a[1] == 12 and a[3] is None and a[4] == 1 + 0j and a[5:11] == (2.0, -1.0, 0.0, 0.0, 60.0, 60.0)
    assert out.shape == (12,) and out.dtype == np.complex128
    rec.calls.clear()
    assert oa.mzm(2.0, 0.5).shape == (1,)                                    # scalars: the reference's np.array([u])
    assert oa.pm(np.ones((3, 2)), np.zeros((3, 2)), 2).shape == (3, 2)
    assert oa.iqm(np.float64(1.0), u + 1j * u).shape == (12,)
    kinds = [c[1][0] for c in rec.calls]
    assert kinds == ["mzm", "pm", "iqm"]
    assert rec.calls[2][1][5:11] == (2.0, -2.0, -2.0, 1.0, 60.0, 60.0) and rec.calls[2][1][2].dtype == np.complex128
    assert rec.calls[1][1][3].dtype == np.complex128 and rec.calls[1][1][3].shape == (3, 2)
    assert oa.mzm(1, np.arange(4)).dtype == np.complex128 and rec.calls[-1][1][2].dtype == np.float64   # integers are widened


def test_modulator_refusals(unreachable):
    u = np.zeros(8)
    for fn in (lambda E, v: oa.mzm(E, v), lambda E, v: oa.iqm(E, v), lambda E, v: oa.pm(E, v, 2)):
        with pytest.raises(AssertionError, match="same dimensions"):
            fn(np.ones(7), u)
        with pytest.raises(AssertionError, match="same dimensions"):
            fn(fake_device((8, 1), np.complex128), u)
        with pytest.raises(TypeError):
            fn(1.0, fake_device((8,), np.complex64))
        with pytest.raises(TypeError):
            fn(1.0, fake_device((8,), np.float32))
        with pytest.raises(TypeError):
            fn(fake_device((8,), np.float64), u)                          # Ei on the device is complex128
        with pytest.raises(TypeError):
            fn(1.0, np.array(["a"] * 8))
    with pytest.raises(ValueError):
        oa.pm(1.0, u, 0)
    with pytest.raises(ValueError):
        oa.mzm(1.0, u, ic.make_param(dict(Vpi=0)))
    with pytest.raises(ValueError):
        oa.mzm(1.0, u, ic.make_param(dict(ER=float("nan"))))
    with pytest.raises(ValueError):
        oa.iqm(1.0, u, ic.make_param(dict(Vphi=float("inf"))))


def test_upsample_and_voa_refusals(unreachable):
    x = np.zeros(5)
    for f in (0, -1):
        with pytest.raises(ValueError):
            oa.upsample(x, f)
    for f in (1.5, "2", True):
        with pytest.raises(TypeError):
            oa.upsample(x, f)
    with pytest.raises(TypeError):
        oa.upsample(x.astype(np.float32), 2)
    with pytest.raises(TypeError):
        oa.upsample(fake_device((5,), np.float32), 2)
    with pytest.raises(TypeError):
        oa.upsample(fake_device((5,), np.int64), 2)
    with pytest.raises(ValueError):
        oa.upsample(np.zeros((2, 2, 2)), 2)
    with pytest.raises(AssertionError, match="positive scalar"):
        oa.voa(x, -0.1)
    with pytest.raises(TypeError):
        oa.voa(fake_device((5,), np.complex64), 1)
    with pytest.raises(ValueError):
        oa.voa(x, float("inf"))


def test_upsample_and_voa_calls(rec):
    out = oa.upsample(np.zeros((4, 3), dtype=np.complex128), 5)
    assert out.shape == (20, 3) and out.dtype == np.complex128 and rec.calls[-1] [1][:4] == (4, 6, 5, 1.0)
    out = oa.upsample(np.zeros(4, dtype=np.complex64), 2)
    assert out.shape == (8,) and out.dtype == np.complex64 and rec.calls[-1][1][:4] == (4, 1, 2, 1.0)
    out = oa.voa(np.zeros((4, 2)), 6)
    assert out.shape == (4, 2) and out.dtype == np.float64 and rec.calls[-1][1][:4] == (4, 2, 1, 10 ** (-6 / 20))


def test_awgn_defaults_draw_order_and_stream(rec):
    sig = np.ones((50, 2)) + 0j
    np.random.seed(7)
    out = oa.awgn(sig, oa.parameters())
    after = np.random.get_state()
    (name, a), = rec.calls
    n, ncols, s, o, cplx, FsB, snr_lin, un, seed = a
    assert (n, ncols, cplx, FsB, snr_lin, seed) == (100, 1, True, 1.0, 100.0, 0) and out.dtype == np.complex128 and out.shape == (50, 2)
    np.random.seed(7)
    zr = np.random.standard_normal((50, 2))
    zi = np.random.standard_normal((50, 2))                                # the real block, then the imaginary block
    assert np.array_equal(un[0], zr.reshape(-1)) and np.array_equal(un[1], zi.reshape(-1))
    assert all(np.array_equal(x, y) for x, y in zip(after, np.random.get_state()))
    rec.calls.clear()
    out = oa.awgn(np.ones(9), ic.make_param(dict(snr=3, Fs=8, B=2, complexNoise=False, seed=5)))
    a = rec.calls[0][1]
    np.random.seed(5)
    assert out.dtype == np.float64 and a[4] is False and a[5] == 4.0 and a[6] == 10 ** 0.3 and a[7].shape == (1, 9)
    assert np.array_equal(a[7][0], np.random.standard_normal(9))
    assert oa.awgn(np.ones(9), oa.parameters()).dtype == np.complex128           # a real signal with complex noise
    assert oa.awgn(np.ones(9, dtype=np.float32), ic.make_param(dict(complexNoise=False))).dtype == np.float64


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-1), dict(Fs=0), dict(Fs=-2.0), dict(snr=float("nan")), dict(snr=float("inf")),
                                 dict(snr=-float("inf")), dict(Fs=float("inf")), dict(B=float("nan")), dict(snr=4000)])
def test_awgn_refusals(unreachable, bad):
    state = np.random.get_state()
    with pytest.raises(ValueError):
        oa.awgn(np.ones(8) + 0j, ic.make_param(dict(dict(seed=1), **bad)))
    assert all(np.array_equal(x, y) for x, y in zip(state, np.random.get_state()))      # refused before anything is drawn


def test_awgn_refuses_what_it_cannot_take(unreachable):
    for dt in (np.complex64, np.float32, np.int64):
        with pytest.raises(TypeError):
            oa.awgn(fake_device((8,), dt), oa.parameters())
    with pytest.raises(ValueError):
        oa.awgn(fake_device((2, 2, 2), np.complex128), oa.parameters())
    with pytest.raises(ValueError):
        oa.awgn(np.zeros(0), oa.parameters())
    with pytest.raises(TypeError):
        oa.awgn(np.array(["x"]), oa.parameters())


def test_library_refuses_with_a_status_before_any_device_work():
    """The C entries check their arguments before they look for a device: a message, not a crash, on a box without a GPU too."""
    import ctypes as C
    from opticommpy_amd import _lib
    lib = _lib.load()
    x = np.zeros(8)
    p = x.ctypes.data_as(C.c_void_p)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ssf_pam_tx(0, 4, 2, 1, 4097, dp, dp, 0.25, 3.0, -1.5, 80.0, 1.0, p) == -6
    assert b"4096" in lib.ssf_last_error(None)
    assert lib.ssf_pam_tx(0, 0, 2, 1, 4, dp, dp, 0.25, 3.0, -1.5, 80.0, 1.0, p) == -1
    assert lib.ssf_pam_tx(0, 4, 2, 1, 4, dp, dp, 0.25, 0.0, -1.5, 80.0, 1.0, p) == -1
    assert lib.ssf_pam_tx(0, 4, 2, 1, 4, None, dp, 0.25, 3.0, -1.5, 80.0, 1.0, p) == -1
    assert lib.ssf_modulate_optical(0, 3, 4, 2, p, None, 1.0, 0.0, 2.0, -1.0, 0.0, 0.0, 60.0, 60.0, p) == -1
    assert lib.ssf_modulate_optical(0, 1, 4, 1, p, None, 1.0, 0.0, 2.0, -1.0, 0.0, 0.0, 60.0, 60.0, p) == -6       # complex64 drive
    assert lib.ssf_modulate_optical(0, 1, 0, 2, p, None, 1.0, 0.0, 2.0, -1.0, 0.0, 0.0, 60.0, 60.0, p) == -1
    assert lib.ssf_awgn(0, 4, 1, 0, 2, 0, 1.0, 10.0, p, p, 0, p) == -1            # complex in, float64 out
    assert lib.ssf_awgn(0, 4, 1, 2, 2, 1, 1.0, 10.0, p, p, 0, p) == -1            # complex noise, float64 out
    assert lib.ssf_awgn(0, 4, 1, 0, 0, 1, 0.0, 10.0, p, p, 0, p) == -1
    assert lib.ssf_awgn(0, 4, 1, 0, 0, 1, 1.0, float("inf"), p, p, 0, p) == -1
    assert lib.ssf_awgn(0, 4, 1, 0, 0, 1, 1.0, 10.0, p, None, 0, p) == -1         # neither normals nor a seed
    assert lib.ssf_awgn(0, 4, 1, 3, 0, 1, 1.0, 10.0, p, p, 0, p) == -6
    assert lib.ssf_upsample(0, 4, 1, 0, 1.0, p, p) == -1
    assert lib.ssf_upsample(0, 4, 1, 2, 1.0, p, p) == -1                          # in place with a factor
    assert lib.ssf_upsample(0, 4, 1, 1, float("nan"), p, p) == -1
