"""The arithmetic of the mlse / detector / autocorr kernels without a GPU: tests/emu/emu_seqdet.cpp includes
opticommpy_amd/csrc/seqdet_kernels.h -- the bodies the gfx950 kernels call -- and walks them with g++ in the kernels' lane layout,
buffer rotation, chunking and three-step traceback.  The restatement is held to every fixture first; then every fixture and every
shape row of tests/seqdet_cases.py is held to the bounds of tests/test_gpu_seqdet.py."""
import numpy as np
import pytest

import seqdet_cases as sc
import seqdet_restatement as rs
from opticommpy_amd import seqdet


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return sc.build_emu(tmp_path_factory.mktemp("emu_seqdet") / "emu_seqdet")


@pytest.mark.parametrize("name", sc.MLSE_CASES)
def test_restatement_matches_the_reference_mlse(name):
    g = sc.load(f"mlse_{name}")
    sc.check_conditions(g)
    w = rs.mlse(g["y"], g["h"], g["c"])
    assert np.array_equal(g["c"][w["index"]].astype(g["y"].dtype), g["out"]) and np.array_equal(w["index"], g["index"])
    assert sc.rel(w["metric"], g["metric"]) <= 1e-15 and w["ties"] == int(g["ties"]) and w["states"] == g["cfg"]["states"]
    assert w["gap"] == pytest.approx(float(g["gap"]), rel=1e-6)


@pytest.mark.parametrize("name", sc.MLSE_CASES)
def test_emulated_mlse_matches_the_reference(emu, tmp_path, name):
    g = sc.load(f"mlse_{name}")
    out, metric, info = sc.emu_mlse(emu, tmp_path, g["y"], g["h"], g["c"])
    assert out.dtype == g["out"].dtype and np.array_equal(out, g["out"])
    d = sc.rel(metric[0], g["metric"])
    print(f"{name}: final metric within {d:.2e} relative")
    assert d <= sc.TOL
    S = g["cfg"]["states"]
    assert info["states"] == S and info["chunk"] == seqdet.T
    assert info["kernel"] == (0 if S <= 64 else 1) and info["survivor_bytes"] == seqdet.survivor_bytes(len(g["y"]), 1, S)


@pytest.mark.parametrize("rid", sc.MLSE_ROW_IDS)
def test_emulated_mlse_row_matches_the_restatement(emu, tmp_path, rid):
    y, h, c, want = sc.mlse_row(rid)
    out, metric, info = sc.emu_mlse(emu, tmp_path, y, h, c)
    cols = len(want)
    assert out.shape == y.shape and info["states"] == want[0]["states"]
    for k, w in enumerate(want):
        got = out if cols == 1 else out[:, k]
        assert np.array_equal(got, c[w["index"]]), (rid, k)
        assert sc.rel(metric[k], w["metric"]) <= sc.TOL, (rid, k)
    if cols > 1:                              # a column alone is the 1-D call, bit for bit
        one, m1, _ = sc.emu_mlse(emu, tmp_path, np.ascontiguousarray(y[:, 1]), h, c)
        assert np.array_equal(one, out[:, 1]) and m1[0] == metric[1]
    tail = sc.MLSE_ROWS[rid]["tail"]
    if tail:
        assert want[0]["final_state"] == (want[0]["states"] - 1 if tail == "last" else 0)


def test_rows_cover_what_they_claim():
    T, C = seqdet.T, seqdet.CHUNK
    rows = {rid: sc.mlse_row(rid) for rid in sc.MLSE_ROW_IDS}
    assert {w[3][0]["states"] for w in rows.values()} >= {1, 2, 3, 4, 9, 16, 64, 128, 256, 1024}
    assert {len(w[2]) for w in rows.values()} >= {2, 3, 4, 8, 16, 64}
    assert {len(w[0]) for w in rows.values()} >= {1, 2, 3, 4, T - 1, T, T + 1, 2 * T + 1, C - 1, C, C + 1}
    assert {w[0].ndim == 2 and w[0].shape[1] for w in rows.values()} >= {False, 2, 3}
    assert {np.iscomplexobj(w[0]) for w in rows.values()} == {False, True}
    assert C % T == 0


@pytest.mark.parametrize("name", sc.DET_CASES)
def test_emulated_detector_matches_the_reference(emu, tmp_path, name):
    g = sc.load(f"det_{name}")
    sc.check_conditions(g)
    cfg = g["cfg"]
    px = g["px"] if cfg["has_px"] else None
    want, gap = rs.detector(g["r"], cfg["sigma2"], g["c"], px, cfg["rule"])
    assert np.array_equal(want, g["ind"]) and gap == pytest.approx(float(g["gap"]), rel=1e-6)
    decided, ind = sc.emu_detector(emu, tmp_path, g["r"], cfg["sigma2"], g["c"], px, cfg["rule"])
    assert np.array_equal(ind, g["ind"]) and np.array_equal(decided, g["decided"]) and decided.dtype == g["decided"].dtype
    assert ind.dtype == np.int64


@pytest.mark.parametrize("rid", sc.DET_ROW_IDS)
def test_emulated_detector_row_matches_the_restatement(emu, tmp_path, rid):
    r, sigma2, c, px, rule, want = sc.det_row(rid)
    decided, ind = sc.emu_detector(emu, tmp_path, r, sigma2, c, px, rule)
    assert ind.shape == r.shape and np.array_equal(ind, want) and np.array_equal(decided, c[want].astype(r.dtype))


@pytest.mark.parametrize("name", sc.WHITE_CASES)
def test_emulated_autocorr_matches_the_reference(emu, tmp_path, name):
    g = sc.load(name)
    sc.check_conditions(g)
    nTaps = g["cfg"]["nTaps"]
    r = sc.emu_autocorr(emu, tmp_path, g["x"], nTaps)
    d = float(np.max(np.abs(r - g["r"])) / abs(g["r"][0]))
    w = seqdet.levinson(r, nTaps)
    dw = float(np.max(np.abs(w - g["w"])) / np.max(np.abs(g["w"])))
    print(f"{name}: autocorr within {d:.2e} of r[0], w within {dw:.2e} of max |w|")
    assert d <= sc.TOL and dw <= sc.TOL
    sc.check_autocorr(r, g["x"], nTaps, name)


@pytest.mark.parametrize("i", range(len(sc.AC_ROWS)), ids=sc.AC_ROW_IDS)
def test_emulated_autocorr_row_matches_the_restatement(emu, tmp_path, i):
    x, nTaps = sc.ac_row(i)
    sc.check_autocorr(sc.emu_autocorr(emu, tmp_path, x, nTaps), x, nTaps, sc.AC_ROW_IDS[i])
