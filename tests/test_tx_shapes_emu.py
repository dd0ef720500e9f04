"""The WDM transmitter without a GPU at every row of tests/tx_shape_cases.py marked for the emulator: the kernel bodies of
rx_kernels.h / fused_kernels.h and the host sequencing of RxCore::wdm_tx are the ones the GPU runs (tests/emu/emu.cpp), the
marshalling is opticommpy_amd/wdm_tx.py itself with its backend swapped.  Bounds as on the GPU (tests/test_gpu_tx_shapes.py); the
emulator also counts the launches: four per channel and polarisation, two more per channel for a device walk, none for a refusal.
Every row's conditions are checked, emulated or not; the restated Philox is pinned to the Random123 vectors; the host's symbol-draw
shortcut is held to the oracle's np.random.choice for every power-of-two alphabet."""
import ctypes as C
import types

import numpy as np
import pytest

import emu_binding as eb
import opticommpy_amd as oa
import tx_shape_cases as ts
from opticommpy_amd import wdm_tx
from oracle import tx_oracle as otx
from oracle.ssf_oracle import parameters as oparams

REFUSAL = {"unsupported": AssertionError}              # what simpleWDMTx ends in on this backend (EmuTxBackend asserts rc == 0)


@pytest.fixture(autouse=True)
def emu_backend(monkeypatch):
    monkeypatch.setattr(wdm_tx, "_backend", eb.EmuTxBackend())


def _wdm_tx(p, symbols, taps, phi, amp, deltaF, out, power):
    e = eb.EmuTxBackend().e
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None   # noqa: E731
    return e.emu_wdm_tx(C.byref(p), symbols.ctypes.data_as(C.c_void_p), dp(taps), dp(phi), dp(amp), dp(deltaF), out.ctypes.data_as(C.c_void_p), dp(power))


def _launches():
    e = eb.load()
    e.emu_rx_launches.restype = C.c_long
    return e.emu_rx_launches()


API = types.SimpleNamespace(simpleWDMTx=oa.simpleWDMTx, wdm_tx=_wdm_tx, empty=lambda dev, shape: np.empty(shape, dtype=np.complex128))


def test_restated_philox_known_answers():
    """Random123 known-answer vectors for philox4x32_10 (Salmon et al., kat_vectors), as tests/test_emu_fused.py holds the kernels' to."""
    f = 0xffffffff
    for ctr, key, want in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([f, f, f, f], [f, f], [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        out = ts.philox4x32_10(*[np.array([c, c], dtype=np.uint64) for c in ctr], *key)
        assert [[int(w[i]) for w in out] for i in (0, 1)] == [want, want]


@pytest.mark.parametrize("row", ts.ROWS, ids=lambda r: r.id)
def test_row_conditions(row):
    ts.check_conditions(row)


def test_table_order_alternates_large_and_small():
    N = [ts.geometry(ts.keywords(r))[0] for r in ts.ROWS]
    assert all(N[i] >= N[i + 1] <= N[i + 2] for i in range(0, len(N) - 2, 2))
    assert max(N) <= 70000


@pytest.mark.parametrize("row", ts.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_kernels_match_the_expected_output(row):
    kw = ts.keywords(row)
    if row.kind == "abi" and row.raises:
        assert ts.call(row, API) == ts.ERR_CODE[row.raises] and _launches() == 0, row.id
        return
    if row.raises:
        with pytest.raises(REFUSAL[row.raises]):
            ts.call(row, API)
        assert _launches() == 0, row.id
        return
    got = ts.call(row, API)
    ts.compare(row, got, "emu")
    assert _launches() == kw["nChannels"] * (2 * (row.kind == "device_pn") + 4 * kw.get("nPolModes", 1)), (row.id, _launches())
    again = ts.call(row, API)
    assert again.sig.tobytes() == got.sig.tobytes(), row.id


def test_two_keys_give_two_fields():
    a, b = (ts.call(ts.BY_ID[f"walk-device-key{i}-n4100"], API) for i in (0, 1))
    assert np.array_equal(a.symb, b.symb)
    assert np.max(np.abs(a.sig - b.sig)) > 1e-3 * np.max(np.abs(a.sig))


@pytest.mark.parametrize("M", [2 ** k for k in range(1, 11)])
def test_symbol_draw_shortcut_is_the_oracles_choice(M):
    """wdm_tx._symbol_source draws a uniform power-of-two alphabet as floor(u M): draw for draw the oracle's symbolSource
    (np.random.choice), with a seed and from the global stream, and np.random ends where the oracle leaves it."""
    n = 3000
    for constType in ("pam", "psk") + (("qam",) if int(np.sqrt(M)) ** 2 == M else ()):
        q = oparams()
        q.nSymbols, q.M, q.constType, q.dist = n, M, constType, "uniform"
        for seed in (M + 5, None):
            q.seed = seed
            np.random.seed(77)
            want = otx.symbolSource(q)
            want_next = np.random.random_sample(3)
            np.random.seed(77)
            got = wdm_tx._symbol_source(n, M, constType, "uniform", 0, seed)
            got_next = np.random.random_sample(3)
            assert np.array_equal(got, want) and np.array_equal(got_next, want_next), (M, constType, seed)
