"""The IM/DD transmitter's and the AWGN channel's kernels without a GPU: tests/emu/emu_imddtx.cpp includes
opticommpy_amd/csrc/imddtx_kernels.h -- the bodies the gfx950 kernels call -- and walks them with g++ over the device's grids.  The
walk stands in the library's place (imddtx_cases.Emu), so every fixture and shape row goes through the public functions: their
checks, draws and layouts are the package's own.  Bounds as in tests/test_gpu_imddtx.py.  The pulse-shaping filter is not walked
(tests/test_emu_tx.py walks the overlap-save launch); the rows one sample either side of the element-wise grid-stride span run on
the GPU only.  The same walk is also built as a program under -fsanitize=address,undefined and run, never loaded into Python."""
import numpy as np
import pytest

import imddtx_cases as ic
import imddtx_restatement as ir
from opticommpy_amd import imddtx
from opticommpy_amd.wdm_tx import pulseShape


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return ic.build_emu(tmp_path_factory.mktemp("emu_imddtx") / "emu_imddtx")


@pytest.fixture
def emu(exe, tmp_path, monkeypatch):
    e = ic.Emu(exe, tmp_path)
    monkeypatch.setattr(imddtx, "_backend", e)
    return e


def pam_taps(p):
    pp = ic.make_param(dict(pulseType=p.pulseType, nFilterTaps=p.nFilterTaps, rollOff=p.pulseRollOff, SpS=p.SpS))
    return pulseShape(pp)


@pytest.mark.parametrize("case", ic.PAM_CASES)
def test_pam_fixture(emu, case):
    g = ic.load("pam_" + case)
    p = ic.make_param(g["cfg"]["param"])
    res = imddtx.pamTransmitter(p)
    assert len(res) == (3 if g["cfg"]["param"].get("returnParam") else 2)
    assert np.array_equal(res[1], g["symbTx"]) and res[1].dtype == np.float64
    assert res[0].dtype == np.complex128
    err = ic.rel_peak(res[0], g["sigTxo"])
    print(f"pam_{case}: {err:.2e}")
    assert err <= ic.BOUND
    assert emu.calls == [0]


@pytest.mark.parametrize("rid", list(ic.PAM_ROWS))
def test_pam_shape_row(emu, rid):
    d = ic.PAM_ROWS[rid]
    p = ic.make_param(d)
    sig, symb = imddtx.pamTransmitter(p)
    want = ic.pam_restated(symb, pam_taps(p), vars(p))
    assert sig.shape == want.shape
    assert ic.rel_peak(sig, want) <= ic.BOUND


@pytest.mark.parametrize("rid", list(ic.PEAK_ROWS))
def test_peak_row(emu, rid):
    got, want = ic.run_peak_row(rid)
    assert ic.rel_peak(got, want) <= ic.BOUND


@pytest.mark.parametrize("case", ic.MOD_CASES)
def test_modulator_fixture(emu, case):
    g = ic.load("mod_" + case)
    out = ic.mod_call(g)
    assert out.dtype == np.complex128 and out.shape == g["out"].shape
    err = ic.rel_peak(out, g["out"])
    print(f"mod_{case}: {err:.2e}")
    assert err <= ic.BOUND


@pytest.mark.parametrize("kind", ["pm", "mzm", "iqm"])
@pytest.mark.parametrize("n", ic.MOD_ROW_SIZES)
def test_modulator_shape_row(emu, kind, n):
    Ei, u = ic.mod_row_inputs(n, kind)
    if kind == "pm":
        got, want = imddtx.pm(Ei, u, 2.5), ir.pm(Ei, u, 2.5)
    elif kind == "mzm":
        got, want = imddtx.mzm(Ei, u, ic.make_param(dict(Vpi=2, Vb=-0.6, ER=25))), ir.mzm(Ei, u, 2, -0.6, 25)
    else:
        prm = dict(Vpi=2, VbI=-1.7, VbQ=-2.2, Vphi=0.9, ERI=10, ERQ=80)
        got, want = imddtx.iqm(Ei, u, ic.make_param(prm)), ir.iqm(Ei, u, **prm)
    assert ic.rel_peak(got, ir.narrow(want)) <= ic.BOUND


@pytest.mark.parametrize("case", ic.AWGN_CASES)
def test_awgn_fixture(emu, case):
    g = ic.load("awgn_" + case)
    ic.awgn_seed_global(g)
    out = imddtx.awgn(g["sig"], ic.make_param(g["cfg"]["param"]))
    assert out.dtype == g["out"].dtype and out.shape == g["out"].shape
    err = ic.rel_peak(out, g["out"])
    print(f"awgn_{case}: {err:.2e}")
    assert err <= ic.BOUND


@pytest.mark.parametrize("shape,real", [((1,), False), ((257, 1), False), ((300, 3), False), ((513,), True), ((2,), True)])
def test_awgn_shape_row(emu, shape, real):
    rng = np.random.default_rng(sum(shape))
    sig = rng.standard_normal(shape) if real else rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    prm = dict(snr=11, Fs=3.0, B=2.0, complexNoise=not real, seed=77)
    out = imddtx.awgn(sig, ic.make_param(prm))
    np.random.seed(77)
    zr = np.random.standard_normal(shape)
    zi = None if real else np.random.standard_normal(shape)
    want = ir.narrow(ir.awgn(sig, zr, zi, 1.5, 10 ** 1.1))
    assert out.dtype == want.dtype and ic.rel_peak(out, want) <= ic.BOUND


def test_awgn_device_generator_is_walked_too(emu):
    """The Philox branch of the noise pass: repeatable per seed, different between seeds and columns, the asked power."""
    n = 4096
    sig = np.ones((n, 2), dtype=np.complex128)

    def run(seed):
        out = np.empty((n, 2), dtype=np.complex128)
        emu.awgn(n, 2, sig, out, True, 1.0, 10.0, None, seed)
        return out - sig
    a, b, c = run(5), run(5), run(6)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a[:, 0], a[:, 1])
    assert abs(np.mean(np.abs(a) ** 2) / 0.1 - 1) <= 6 / np.sqrt(2 * n)


def test_upsample_and_voa(emu):
    g = ic.load("sources")
    for name, factor in g["cfg"]["rows"]["upsample"].items():
        got = imddtx.upsample(g[name + "_in"], factor)
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name
    x = g["up_2d_5_in"]
    assert np.array_equal(imddtx.voa(x, 3.0), x * 10 ** (-3.0 / 20)) and np.array_equal(imddtx.voa(x.real.copy(), 0.5), x.real * 10 ** (-0.5 / 20))
    assert np.array_equal(imddtx.voa(x), x)
    assert np.array_equal(imddtx.upsample(g["bits_random"], 2), ir.upsample(g["bits_random"], 2))      # int64: any 8-byte dtype


def test_the_walk_is_clean_under_the_sanitizers(tmp_path):
    """Built and run as a program with its own main: one call of every kind."""
    exe = ic.build_emu(tmp_path / "emu_imddtx_san", flags=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    e = ic.Emu(exe, tmp_path)
    s = ic.peak_row("peak_last")
    out = np.empty((len(s), 2), dtype=np.complex128)
    e.pam_tx(len(s), 1, 2, np.ones(1), np.stack([s, s[::-1]]), 0.4, 3.0, -1.2, 30.0, 0.02, out)
    assert ic.rel_peak(out[:, 0], ir.narrow(ir.pam_field(s, np.ones(1), 1, 0.4, 3.0, 1.2, 30.0, 10 * np.log10(0.02 ** 2 / 1e-3))[0])) <= ic.BOUND
    Ei, u = ic.mod_row_inputs(257, "iqm")
    o = np.empty(257, dtype=np.complex128)
    e.modulate("iqm", 257, u, Ei, 0j, 2.0, -2.0, -2.0, 1.0, 60.0, 60.0, o)
    assert ic.rel_peak(o, ir.narrow(ir.iqm(Ei, u))) <= ic.BOUND
    sig = np.ones((300, 3))
    o = np.empty((300, 3))
    un = np.random.default_rng(1).standard_normal((1, 900))
    e.awgn(300, 3, sig, o, False, 1.0, 100.0, un, 0)
    assert ic.rel_peak(o, ir.narrow(ir.awgn(sig, un, None, 1.0, 100.0))) <= ic.BOUND
    o = np.empty((300, 3), dtype=np.complex128)
    e.awgn(300, 3, sig, o, True, 1.0, 100.0, None, 9)
    x = np.arange(21.0).reshape(7, 3)
    o = np.empty((28, 3))
    e.stuff(7, 3, 4, 1.0, x, o)
    assert np.array_equal(o, ir.upsample(x, 4))
