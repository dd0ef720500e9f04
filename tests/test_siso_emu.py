"""The arithmetic of the ffe / dfe / volterra kernels without a GPU: tests/emu/emu_siso.cpp includes
opticommpy_amd/csrc/siso_kernels.h -- the per-symbol bodies the gfx950 kernels call -- and loops them over lanes and symbols with
g++, in the kernel's lane layout and reduction order, with the kernel's own division of the symbols between the serial walk and
the frozen tail and its way of carrying the window over a restart.  Every fixture and every shape row of tests/siso_cases.py is
held to the bounds of tests/test_gpu_siso.py."""
import numpy as np
import pytest

import siso_cases as sc
import siso_restatement as sr
from opticommpy_amd import sisoeq


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return sc.build_emu(tmp_path_factory.mktemp("emu_siso") / "emu_siso")


@pytest.mark.parametrize("name", sc.EXPECTED_CASES)
def test_emulated_kernels_match_the_reference(emu, tmp_path, name):
    g = sc.load(name)
    sc.check_conditions(g)
    kind = g["cfg"]["kind"]
    x, r = sc.inputs(g)
    sig, coef, mse, info = sc.run_emu(emu, tmp_path, kind, x, r, sc.param(g))
    sc.compare_results((sig, coef, mse), (g["sigOut"], sc.coefficients(g), g["mse"]), name)
    assert (info["serial_symbols"], info["parallel_symbols"]) == sisoeq.expected_split(sisoeq._prepare(kind, x, r, sc.param(g)))
    if g["cfg"]["single"]:                  # prec left unset: against the reference's single-precision run
        x32, r32 = sc.inputs(g, double=False)
        sig = sc.run_emu(emu, tmp_path, kind, x32, r32, sc.param(g, double=False))[0]
        d = sc.rel_l2(sig, g["sigOut32"].astype(np.float64))
        print(f"{name}: distance to the single-precision run {d:.2e}, the reference's own {float(g['self_err']):.2e}")
        assert d <= 2 * float(g["self_err"]), d


@pytest.mark.parametrize("name", sc.EXPECTED_CASES)
def test_restatement_matches_the_reference(name):
    g = sc.load(name)
    kind = g["cfg"]["kind"]
    x, r = sc.inputs(g)
    w = sr.restate(kind, x, r, sc.param(g))
    sc.compare_results((w["sigOut"], w["coef"], w["mse"]), (g["sigOut"], sc.coefficients(g), g["mse"]), name)
    assert w["gap"] == pytest.approx(float(g["gap"]), rel=1e-6) or (np.isinf(w["gap"]) and np.isinf(float(g["gap"])))


@pytest.mark.parametrize("rid", sc.ROW_IDS)
def test_emulated_shape_row_matches_the_restatement(emu, tmp_path, rid):
    kind, x, tx, prm = sc.row(rid)
    want = sr.restate(kind, x, tx, prm)
    sig, coef, mse, info = sc.run_emu(emu, tmp_path, kind, x, tx, prm)
    sc.compare_results((sig, coef, mse), (want["sigOut"], want["coef"], want["mse"]), rid)
    q = sisoeq._prepare(kind, x, tx, prm)
    assert (info["serial_symbols"], info["parallel_symbols"]) == sisoeq.expected_split(q)
    # with the frozen kernel switched off the serial walk gives the same symbols (to rounding: the sums run in another order)
    sig2, coef2, mse2, info2 = sc.run_emu(emu, tmp_path, kind, x, tx, prm, frozen=False)
    assert info2["parallel_symbols"] == 0
    sc.compare_results((sig2, coef2, mse2), (want["sigOut"], want["coef"], want["mse"]), rid + " (serial only)")
