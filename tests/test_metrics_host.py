"""Host side of the link metrics (no GPU): argument rules of opticommpy_amd.metrics, the derived constellation tables against the
values the reference produced (stored in the fixtures), the C ABI's rejection of bad arguments before any device is touched, and
the rule that nothing is computed without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import metrics_cases as mc
import opticommpy_amd as oa
from opticommpy_amd import _lib
from opticommpy_amd import metrics as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names():
    for name in ("fastBERcalc", "monteCarloGMI", "monteCarloMI", "calcEVM", "demodulateGray", "pnorm", "signalPower", "metrics"):
        assert callable(getattr(oa, name)) and name in oa.__all__
    from opticommpy_amd.metrics import fastBERcalc, metrics
    assert fastBERcalc is oa.fastBERcalc and callable(metrics)
    for f in (oa.monteCarloGMI, oa.monteCarloMI):
        assert "left as they are" in f.__doc__                     # the deviation from the reference is stated


@pytest.mark.parametrize("M, constType", [(2, "ook"), (16, "apsk"), (12, "qam"), (32, "qam"), (2048, "qam"), (1, "psk"), (6, "pam"),
                                          (16, "QAM")])
def test_unsupported_constellations_raise_value_error(M, constType):
    x = np.ones(64, dtype=np.complex128)
    for call in (lambda: oa.fastBERcalc(x, x, M, constType), lambda: oa.monteCarloGMI(x, x, M, constType),
                 lambda: oa.monteCarloMI(x, x, M, constType), lambda: oa.calcEVM(x, M, constType),
                 lambda: oa.calcEVM(x, M, constType, x), lambda: oa.metrics(x, x, M, constType),
                 lambda: oa.demodulateGray(x, M, constType)):
        with pytest.raises(ValueError):
            call()


def test_shape_and_argument_rules_raise_value_error():
    x = np.ones((64, 2), dtype=np.complex128)
    with pytest.raises(ValueError, match="differ in shape"):
        oa.fastBERcalc(x, x[:32], 16, "qam")
    with pytest.raises(ValueError, match="differ in shape"):
        oa.metrics(x, x[:, 0], 16, "qam")
    with pytest.raises(ValueError, match="differ in shape"):
        oa.monteCarloGMI(x, np.ascontiguousarray(x.T), 16, "qam")
    with pytest.raises(ValueError, match="dimensions"):
        oa.monteCarloMI(x.reshape(32, 2, 2), x.reshape(32, 2, 2), 16, "qam")
    with pytest.raises(ValueError, match="discard"):
        oa.fastBERcalc(x, x, 16, "qam", discard=32)
    with pytest.raises(ValueError, match="discard"):
        oa.calcEVM(x, 16, "qam", discard=-1)
    with pytest.raises(ValueError, match="px"):
        oa.fastBERcalc(x, x, 16, "qam", px=np.ones(8) / 8)
    with pytest.raises(ValueError):
        oa.demodulateGray(x, 16, "qam")                             # one-dimensional sequences only
    with pytest.raises(ValueError, match="modes"):
        oa.fastBERcalc(np.ones((100, 65), complex), np.ones((100, 65), complex), 16, "qam")


def test_shape_rules_of_the_reference():
    assert om._columns(np.ones(8, complex), "rx")[1:] == (8, 1, 0)
    assert om._columns(np.ones((8, 2), complex), "rx")[1:] == (8, 2, 0)
    assert om._columns(np.ones((2, 8), complex), "rx")[1:] == (8, 2, 1)       # shape[1] > shape[0]: transposed
    assert om._columns(np.ones((2, 2), complex), "rx")[1:] == (2, 2, 0)
    assert om._columns(np.ones(8, np.int32), "rx")[0].dtype == np.float64     # other types are widened to double


@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_tables_equal_the_references(name):
    """Single-precision storage, double-precision normalisation, single-precision pnorm for the blind EVM: value for value."""
    g = mc.load(name)
    cfg = g["cfg"]
    raw, norm, px, Es, H = om._tables(cfg["M"], cfg["constType"], g["px"])
    ref_raw, ref_norm = g["const_raw"], g["const_norm"]
    assert ref_raw.dtype in (np.complex64, np.float32)
    assert ref_norm.dtype in (np.complex128, np.float64), f"fixture made by numpy {cfg['numpy']}"
    assert np.array_equal(raw, ref_raw.astype(np.complex128))
    assert np.array_equal(norm, ref_norm.astype(np.complex128))
    assert Es == float(g["Es"]) and H == float(g["H"])
    assert np.array_equal(px, np.ones(cfg["M"]) / cfg["M"] if g["px"] is None else g["px"])
    table, w32 = om._evm_tables(cfg["M"], cfg["constType"])
    assert g["evm_table"].dtype in (np.complex64, np.float32)
    assert np.array_equal(table, g["evm_table"].astype(np.complex128))
    assert w32.dtype == np.float32 and np.array_equal(w32, np.abs(g["evm_table"]) ** 2)


def test_bitmap_is_the_binary_expansion_of_the_point_index():
    """What lets the kernels count bit errors as popcount(irx ^ itx): the fixtures' demodulated bits of symbols that sit on a table
    point are the binary digits of that point's index."""
    g = mc.load("qam16_12dB")
    symb, bits = mc.demod_input(g), g["bits"].reshape(-1, 4)
    raw = om._tables(16, "qam")[0]
    idx = np.argmin(np.abs(symb[:, None] - raw[None, :]), axis=1)
    assert np.array_equal(bits, (idx[:, None] >> np.arange(3, -1, -1)) & 1)


def test_struct_layouts_match_header(tmp_path):
    structs = {"ssf_metrics_params": _lib.MetricsParams, "ssf_metrics_result": _lib.MetricsResult}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    c = tmp_path / "layout.c"
    c.write_text(src)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    want = {"SSF_METRICS_BER": _lib.METRICS_BER, "SSF_METRICS_GMI": _lib.METRICS_GMI, "SSF_METRICS_MI": _lib.METRICS_MI,
            "SSF_METRICS_EVM": _lib.METRICS_EVM, "SSF_METRICS_EVM_BLIND": _lib.METRICS_EVM_BLIND,
            "SSF_M_C128": 0, "SSF_M_C64": 1, "SSF_M_F64": 2, "SSF_M_F32": 3}
    header = open(os.path.join(ROOT, "include", "ssf.h")).read()
    for k, v in want.items():
        assert f"{k} = {v}" in " ".join(header.split()), k


def _params(**kw):
    base = dict(n=64, discard=0, nModes=1, M=16, dtype=0, transposed=0, rotate=1, want=_lib.METRICS_BER, Es=10.0, H=4.0)
    base.update(kw)
    return _lib.MetricsParams(**base)


def test_abi_rejects_bad_arguments_before_touching_a_device():
    """Every check precedes the first allocation or launch: the calls fail with 'bad argument' (-1) on a machine with no GPU too,
    where anything that reached the device layer would answer 'no device' (-5)."""
    lib = _lib.load()
    x = np.ones(64, dtype=np.complex128)
    xp = x.ctypes.data_as(C.c_void_p)
    tab = np.zeros(32)
    tp = tab.ctypes.data_as(C.POINTER(C.c_double))
    w32 = np.zeros(16, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    out = (_lib.MetricsResult * 1)()
    call = lambda p, rx=xp, tx=xp, raw=tp, norm=tp, w=None, o=out: lib.ssf_metrics(0, p, rx, tx, raw, norm, None, w, o)   # noqa: E731
    assert call(None) == -1
    assert call(C.byref(_params()), rx=None) == -1
    assert call(C.byref(_params()), tx=None) == -1
    assert call(C.byref(_params()), raw=None) == -1
    assert call(C.byref(_params()), norm=None) == -1
    assert call(C.byref(_params()), o=None) == -1
    for bad in (dict(M=12), dict(M=1), dict(M=2048), dict(dtype=4), dict(dtype=-1), dict(nModes=0), dict(nModes=65), dict(n=0),
                dict(discard=-1), dict(discard=32), dict(want=0), dict(want=64), dict(Es=0.0), dict(H=0.0),
                dict(want=_lib.METRICS_EVM_BLIND | _lib.METRICS_BER)):
        assert call(C.byref(_params(**bad))) == -1, bad
    blind = _params(want=_lib.METRICS_EVM_BLIND)
    assert call(C.byref(blind), tx=None, w=None) == -1              # needs the float32 weights
    assert call(C.byref(blind), tx=xp, w=w32) == -1                 # takes no tx
    assert b"ssf_metrics" in lib.ssf_last_error(None)
    y = np.empty(64, np.complex128).ctypes.data_as(C.c_void_p)
    assert lib.ssf_pnorm(0, 64, 0, None, y) == -1 and lib.ssf_pnorm(0, 0, 0, xp, y) == -1 and lib.ssf_pnorm(0, 64, 9, xp, y) == -1
    p = C.c_double()
    assert lib.ssf_signal_power(0, 64, 3, 0, xp, C.byref(p)) == -1  # count is not a multiple of rows
    assert lib.ssf_signal_power(0, 64, 64, 0, xp, None) == -1
    bits = np.empty(256, np.int32).ctypes.data_as(C.c_void_p)
    assert lib.ssf_demodulate(0, 64, 0, 12, tp, xp, bits) == -1 and lib.ssf_demodulate(0, 64, 0, 16, None, xp, bits) == -1
    assert lib.ssf_demodulate(0, 0, 0, 16, tp, xp, bits) == -1


@pytest.mark.skipif(oa.checkGPU(), reason="needs a box WITHOUT a GPU")
def test_no_cpu_fallback_when_no_gpu():
    g = mc.load("qam16_12dB")
    rx, tx = g["rx"], g["tx"]
    for call in (lambda: oa.fastBERcalc(rx, tx, 16, "qam"), lambda: oa.monteCarloGMI(rx, tx, 16, "qam"),
                 lambda: oa.monteCarloMI(rx, tx, 16, "qam"), lambda: oa.calcEVM(rx, 16, "qam"), lambda: oa.calcEVM(rx, 16, "qam", tx),
                 lambda: oa.metrics(rx, tx, 16, "qam"), lambda: oa.pnorm(rx), lambda: oa.signalPower(rx),
                 lambda: oa.demodulateGray(rx[:, 0], 16, "qam")):
        with pytest.raises(RuntimeError):
            call()


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libssf_hip.so")
    x = np.ones(64, dtype=np.complex128)
    with pytest.raises(RuntimeError, match="HIP extension not built"):
        oa.fastBERcalc(x, x, 16, "qam")
    with pytest.raises(RuntimeError, match="HIP extension not built"):
        oa.pnorm(x)
