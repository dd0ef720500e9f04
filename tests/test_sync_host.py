"""Host side of the sequence synchronisation (opticommpy_amd/sync.py) without a GPU: what is out of scope is refused before the
library is even loaded, the shape and type rules hold, and the parameter and result structs are packed as include/ssf.h lays
them out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import opticommpy_amd as oa
from opticommpy_amd import _lib
from opticommpy_amd import sync as osync


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test: the checks under test come before it."""
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


RX = (np.arange(64).reshape(32, 2) + 1j).astype(np.complex128)
TX = (np.arange(32).reshape(16, 2) - 2j).astype(np.complex128)


def test_public_names():
    assert oa.symbolSync is osync.symbolSync and oa.finddelay is osync.finddelay
    assert "symbolSync" in oa.__all__ and "finddelay" in oa.__all__


@pytest.mark.parametrize("rx, tx, SpS, mode", [
    (RX, TX, 2, "phase"), (RX, TX, 2, None),                                    # an unknown mode
    (np.zeros((32, 9), complex), np.zeros((16, 9), complex), 2, "amp"),         # more than 8 modes
    (RX, TX[:, :1], 2, "amp"), (RX[:, 0], TX, 2, "real"),                       # differing mode counts
    (RX, TX[:1], 2, "amp"), (RX[:2], TX, 2, "amp"), (RX[:1], TX, 1, "amp"),     # fewer than 2 symbols on either side
    (RX, TX.real, 2, "amp"), (RX, TX.real.astype(np.float32), 2, "real"), (RX, np.arange(32).reshape(16, 2), 2, "amp"),   # a real tx
    (RX[:31], TX, 2, "amp"), (RX, TX, 3, "amp"),                                # len(rx) is no multiple of SpS
    (RX, TX, 0, "amp"), (RX, TX, 1.5, "amp"),
    (np.zeros((4, 2, 2), complex), TX, 1, "amp"), (RX, np.complex128(1), 1, "amp"),
])
def test_out_of_scope_arguments_raise_before_the_library_loads(no_library, rx, tx, SpS, mode):
    with pytest.raises(ValueError):
        oa.symbolSync(rx, tx, SpS, mode)


def test_device_arrays_of_another_dtype_are_refused(no_library):
    d = object.__new__(oa.DeviceArray)                      # (no GPU needed: the check is on the type)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (32, 2), np.dtype(np.float64), 0, None, d
    with pytest.raises(TypeError, match="complex128 or complex64"):
        oa.symbolSync(d, TX, 2)
    with pytest.raises(ValueError, match="complex"):
        oa.symbolSync(RX, d, 2)                             # a real tx is a ValueError on the device too
    d.dtype = np.dtype(np.int32)
    with pytest.raises(TypeError):
        oa.finddelay(d, np.ones(4))


def test_shape_and_type_rules():
    rx, tx, p = osync._check(RX[:, 0], TX[:, 0].astype(np.complex64), 2, "real")
    assert rx.ndim == 1 and tx.ndim == 1 and tx.dtype == np.complex64 and rx.dtype == np.complex128
    assert (p.n_rx, p.n_tx, p.nModes, p.SpS, p.mode) == (32, 16, 1, 2, 1)
    assert (p.rx_dtype, p.tx_dtype) == (_lib.METRICS_DTYPES["complex128"], _lib.METRICS_DTYPES["complex64"])
    rx, tx, p = osync._check(RX.real, TX, 1, "amp")                          # a real rx is widened
    assert rx.dtype == np.complex128 and p.mode == 0 and p.nModes == 2
    rx, tx, p = osync._check(RX[:, :1], TX[:, 0], 2, "amp")                    # (n, 1) against 1-D: one mode, shapes kept
    assert p.nModes == 1 and rx.shape == (32, 1) and tx.shape == (16,)
    rx, tx, p = osync._check(np.zeros((16, 8), np.complex64), np.zeros((2, 8), complex), 8, "amp")
    assert p.nModes == 8 and p.rx_dtype == _lib.METRICS_DTYPES["complex64"]
    for bad in (np.zeros((2, 2)), np.zeros(0), np.float64(3)):
        with pytest.raises(ValueError):
            osync._vector(bad, "x")
    assert osync._vector([1, 2, 3], "x").dtype == np.float64 and osync._vector(np.ones(3, np.complex64), "x").dtype == np.complex64


def test_struct_layouts_match_the_header(tmp_path):
    """ssf_sync_params and ssf_sync_result as gcc lays them out against the ctypes mirrors."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {"ssf_sync_params": _lib.SyncParams, "ssf_sync_result": _lib.SyncResult}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    (tmp_path / "layout.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert _lib.SYNC_MODES == {"amp": 0, "real": 1} and _lib.SYNC_ROT == (1, -1, 1j, -1j) and _lib.SYNC_MAX_MODES == 8


def test_library_refuses_bad_arguments_without_a_device():
    """The C ABI's own checks come before any allocation or launch: they answer on a box without a GPU."""
    lib = _lib.load()
    rx, tx = np.ascontiguousarray(RX), np.ascontiguousarray(TX)
    out = np.empty_like(tx)
    rp, tp, op = (a.ctypes.data_as(C.c_void_p) for a in (rx, tx, out))
    good = dict(n_rx=32, n_tx=16, nModes=2, SpS=2, mode=0, rx_dtype=0, tx_dtype=0)
    for bad in (dict(mode=2), dict(nModes=0), dict(nModes=9), dict(SpS=0), dict(SpS=3), dict(n_tx=1), dict(n_rx=2), dict(rx_dtype=2),
                dict(tx_dtype=3), dict(SpS=64, nModes=8, n_rx=128)):
        p = _lib.SyncParams(**dict(good, **bad))
        assert lib.ssf_symbol_sync(0, C.byref(p), rp, tp, op, None) == -1, bad
    p = _lib.SyncParams(**good)
    assert lib.ssf_symbol_sync(0, None, rp, tp, op, None) == -1
    assert lib.ssf_symbol_sync(0, C.byref(p), rp, tp, None, None) == -1
    assert b"ssf_symbol_sync" in lib.ssf_last_error(None)
    d = C.c_int64()
    assert lib.ssf_finddelay(0, 0, 4, 0, 0, rp, tp, C.byref(d)) == -1
    assert lib.ssf_finddelay(0, 4, 4, 4, 0, rp, tp, C.byref(d)) == -1
    assert lib.ssf_finddelay(0, 4, 4, 0, 0, rp, tp, None) == -1
    assert b"ssf_finddelay" in lib.ssf_last_error(None)
    s = C.c_double()
    assert lib.ssf_sync_transform_time(0, 1000, 4, 2, 0, 1, C.byref(s)) == -1          # not a power of two
    assert lib.ssf_sync_transform_time(0, 1024, 4, 2, 3, 1, C.byref(s)) == -1          # more second-round transforms than first
    assert lib.ssf_sync_transform_time(0, 1024, 4, 2, 0, 0, C.byref(s)) == -1
    assert lib.ssf_sync_transform_time(0, 1024, 4, 2, 0, 1, None) == -1
