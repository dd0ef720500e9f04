"""modulateOFDM and demodulateOFDM on the GPU against the reference's recorded outputs (tests/golden/ofdm, tools/gen_golden_ofdm.py)
at the bounds of tests/ofdm_cases.py, every way of making the call -- numpy or DeviceArray, complex128 or complex64, either route,
a second time -- and the loop they close on DeviceArrays (run with -m gpu)."""
import numpy as np
import pytest

import ofdm_cases as oc
import ofdm_shape_cases as sc
import opticommpy_amd as oa
from opticommpy_amd import _lib, device, ofdm

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def twice(f, x0, on_device, *args, **kw):
    """One call, made twice on the same input: identical bytes, the input unchanged, no transfer inside for a DeviceArray."""
    x = oa.to_device(x0) if on_device else x0.copy()
    before = device.transfer_counts()
    a = f(x, *args, **kw)
    b = f(x, *args, **kw)
    after = device.transfer_counts()
    if on_device:
        assert after == before, (before, after)
    assert host(x).tobytes() == x0.tobytes()                            # the input is never written
    kind = oa.DeviceArray if on_device else np.ndarray
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    out = []
    for u, v in zip(a, b):
        if isinstance(u, complex):
            assert u == v
            out.append(u)
            continue
        assert type(u) is kind and type(v) is kind
        u, v = host(u), host(v)
        assert u.tobytes() == v.tobytes()
        out.append(u)
    return out


@pytest.mark.parametrize("route", ["auto", "rocfft"])
@pytest.mark.parametrize("name", oc.CASES)
def test_modulator_matches_the_reference(name, route):
    g = oc.load(name)
    oc.check_conditions(g)
    for on_device in (False, True):
        for in_dtype in (np.complex128, np.complex64):
            x = g["symb"].astype(in_dtype)
            got, = twice(oa.modulateOFDM, x, on_device, oc.param(g), _route=route)
            fig = oc.check_mod(g, got, np.complex64)
            wide, = twice(oa.modulateOFDM, x, on_device, oc.param(g), dtype=np.complex128, _route=route)
            fig128 = oc.check_mod(g, wide, np.complex128)
            assert wide.astype(np.complex64).tobytes() == got.tobytes()
            print(name, route, on_device, np.dtype(in_dtype).name, fig, fig128)


@pytest.mark.parametrize("route", ["auto", "rocfft"])
@pytest.mark.parametrize("name", oc.CASES)
def test_demodulator_matches_the_reference(name, route):
    g = oc.load(name)
    for on_device in (False, True):
        for dtype in (np.complex128, np.complex64):
            x = g["rx"].astype(dtype)
            got, H = twice(oa.demodulateOFDM, x, on_device, oc.param(g, returnChannel=True), _route=route)
            fig = oc.check_demod(g, got, H, dtype)
            alone, = twice(oa.demodulateOFDM, x, on_device, oc.param(g), _route=route)           # without returnChannel
            assert alone.tobytes() == got.tobytes()
            print(name, route, on_device, np.dtype(dtype).name, fig)


def test_calls_that_alternate_between_two_plans():
    """The tables of the last plan stay on the device: calls that alternate between two plans must not read each other's."""
    a, b = oc.load("nb_pilots"), oc.load("unsorted")
    for _ in range(2):
        for g in (a, b):
            oc.check_mod(g, oa.modulateOFDM(g["symb"], oc.param(g)), np.complex64)
            got, H = oa.demodulateOFDM(g["rx"], oc.param(g, returnChannel=True))
            oc.check_demod(g, got, H, np.complex128)


def _both_functions(c, route="auto"):
    """One modulator and one demodulator call for a shape case, each against the restatement."""
    sc.check_mod(c, oa.modulateOFDM(c.symb, c.param, dtype=np.complex128, _route=route), np.complex128)
    sc.check_mod(c, oa.modulateOFDM(c.symb, c.param, _route=route), np.complex64)
    for dtype in (np.complex128, np.complex64):
        got, H = oa.demodulateOFDM(c.rx.astype(dtype), c.param, _route=route)
        sc.check_demod(c, got, H, dtype)


# two parameter sets the engine's geometry check cannot tell apart: the same Nfft, SpS and G, the same number of pilots and of nulls
# (hence the same L, Ns, Ni and Np), other carriers.  Only the plan's number says that the tables on the device are the other plan's
TWIN_A = sc.Row("twin_a", 64, 2, 4, False, (3, 40), (32,), 5)
TWIN_B = sc.Row("twin_b", 64, 2, 4, False, (10, 55), (20,), 5)
TWIN_A_NO_PILOTS = sc.Row("twin_a_no_pilots", 64, 2, 4, False, (), (3, 32, 40), 5)
TWIN_B_NO_PILOTS = sc.Row("twin_b_no_pilots", 64, 2, 4, False, (), (10, 20, 55), 5)


@pytest.mark.parametrize("route", ["auto", "rocfft"])
@pytest.mark.parametrize("twins", [(TWIN_A, TWIN_B), (TWIN_A_NO_PILOTS, TWIN_B_NO_PILOTS)], ids=["pilots", "no_pilots"])
def test_calls_that_alternate_between_two_plans_of_one_signature(twins, route):
    """The plans differ in nothing the engine compares but their number: a call that took the tables left on the device for its
    own would put the pilots and nulls (with pilots: gather the data, draw the lines) at the other plan's carriers."""
    a, b = (sc.make(r) for r in twins)
    for c in (a, b):
        sc.check_conditions(c)
    (pa, ga), (pb, gb) = ((ofdm._prepare_mod(c.symb, c.param)["plan"], ofdm._prepare_demod(c.rx, c.param)["plan"]) for c in (a, b))
    assert pa["key"] != pb["key"] and ga["key"] != gb["key"] and len({pa["key"], pb["key"], ga["key"], gb["key"]}) == 4
    assert all(pa[k] == pb[k] and ga[k] == gb[k] for k in ("Nfft", "Ns", "Ni", "Np")) and pa["SpS"] == pb["SpS"]
    assert not np.array_equal(pa["src_map"], pb["src_map"]) and not np.array_equal(ga["data"], gb["data"])
    for _ in range(3):
        for c in (a, b):
            _both_functions(c, route)


@pytest.mark.parametrize("first", ["auto", "rocfft"])
def test_calls_that_alternate_between_the_two_routes_on_one_plan(first):
    """One plan, one number, two tables: register order for the register kernels, natural order around rocFFT."""
    c = sc.make(TWIN_A)
    second = "rocfft" if first == "auto" else "auto"
    assert _lib.ofdm_lds_length(TWIN_A.SpS * TWIN_A.Nfft) and _lib.ofdm_lds_length(TWIN_A.Nfft)
    for _ in range(3):
        for route in (first, second):
            _both_functions(c, route)


CLOSED_LOOP_SEED = 5            # see test_closed_loop_on_device_arrays


@pytest.mark.parametrize("pilots", [False, True], ids=["no_pilots", "pilots"])
@pytest.mark.parametrize("SpS", [2, 1])
def test_closed_loop_on_device_arrays(SpS, pilots):
    """modulateGray -> pnorm -> modulateOFDM(dtype=complex128) -> decimate -> demodulateOFDM -> fastBERcalc, noiseless, on
    DeviceArrays with no transfer in between: BER 0.  Without pilots nothing undoes the 1 / sqrt(SpS) that taking every SpS-th
    sample leaves on the carriers, so the symbols go through pnorm once more.  decimate keeps the sampling phase of largest
    variance and an OFDM signal has the same expected variance in every phase: the seed is one where phase 0 wins, which is
    asserted below on the transmit signal."""
    M, Nfft, G, F = 64, 256, 4, 6
    const = oa.grayMapping(M, "qam").astype(np.complex128)
    const = const / np.sqrt(np.mean(np.abs(const) ** 2))
    prm = oc.Param(Nfft=Nfft, G=G, SpS=SpS, pilot=0.52 * (np.max(const.real) + 1j * np.max(const.imag)),
                   pilotCarriers=np.int64(np.linspace(0, Nfft - 1, 4)) if pilots else np.array([], dtype=np.int64),
                   nullCarriers=np.array([Nfft // 2], dtype=np.int64))
    Ni = Nfft - 1 - (4 if pilots else 0)
    bits = np.random.default_rng(CLOSED_LOOP_SEED).integers(0, 2, size=F * Ni * 6).astype(np.uint8)
    bits_d = oa.to_device(bits)
    before = device.transfer_counts()
    symb = oa.pnorm(oa.modulateGray(bits_d, M, "qam"))
    tx = oa.modulateOFDM(symb, prm, dtype=np.complex128)
    rx = oa.decimate(tx, oc.Param(SpSin=SpS, SpSout=1))
    got = oa.demodulateOFDM(rx, prm)
    if not pilots:
        got = oa.pnorm(got)
    BER, SER, SNR = oa.fastBERcalc(got, symb, M, "qam")
    assert device.transfer_counts() == before
    assert all(type(a) is oa.DeviceArray and a.dtype == np.complex128 for a in (symb, tx, rx, got))
    assert tx.shape == (F * SpS * (Nfft + G),) and rx.shape == (F * (Nfft + G),) and got.shape == (F * Ni,)
    t = tx.get()
    var = np.var(t.reshape(-1, SpS), axis=0)
    assert np.argmax(var) == 0 and np.array_equal(rx.get(), t[::SpS])   # the condition on the seed
    assert np.all(np.asarray(BER) == 0) and np.all(np.asarray(SER) == 0), (BER, SER)
    assert len(np.unique(np.round(got.get(), 6))) == M                  # every point of the constellation came through
