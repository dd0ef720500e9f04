"""The kernels of engine_syncdata.hip on the host: tests/emu/emu_syncdata.cpp walks the bodies of syncdata_kernels.h over the kernels'
workgroups and lanes (g++), against tests/syncdata_restatement.py over the fixtures and the shape rows of
tests/syncdata_shape_cases.py.  Bounds as in tests/syncdata_cases.py: moves bit for bit, counts equal, sums within 1e-9."""
import numpy as np
import pytest

import syncdata_cases as sc
import syncdata_restatement as rs
import syncdata_shape_cases as ssc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sc.build_emu(tmp_path_factory.mktemp("emu_syncdata") / "emu_syncdata")


def same_bits(a, b):
    """Equal up to the sign of zeros."""
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("row", ssc.TILE_ROWS, ids=lambda r: r["name"])
def test_tile_rows(exe, tmp_path, row):
    rx, tx = ssc.tile_input(row)
    want_tx, padL = rs.tile(tx, len(rx), row["SpS"])
    n_pad = len(rx) + padL
    got_rx, got_tx = sc.emu_tile(exe, tmp_path, rx, tx, n_pad, row["SpS"])
    assert got_tx.dtype == got_rx.dtype == np.complex128
    assert same_bits(got_tx, want_tx.astype(np.complex128))
    assert same_bits(got_rx[:len(rx)], rx.astype(np.complex128)) and not np.any(got_rx[len(rx):])
    if row["name"] == "len_P":
        assert padL == 0
    if row["name"] == "len_short":
        assert n_pad == row["nTx"] * row["SpS"]


@pytest.mark.parametrize("row", ssc.EXTRACT_ROWS, ids=lambda r: r["name"])
def test_extract_rows(exe, tmp_path, row):
    x = ssc.extract_input(row)
    n_out = row["n"] // row["SpS"] + 1
    moved, symb, kept = rs.extract(x, n_out)
    got_moved, got_kept = sc.emu_extract(exe, tmp_path, x, n_out, True, False)
    assert np.array_equal(got_kept, kept) and same_bits(got_moved, moved)                      # only moved: bit for bit
    got, got_kept = sc.emu_extract(exe, tmp_path, x, n_out, True, True)
    e, ok = sc.close(got, symb)
    assert ok and np.array_equal(got_kept, kept), (row["name"], e)
    got_real, _ = sc.emu_extract(exe, tmp_path, x, n_out, False, True)
    assert np.array_equal(got_real, got.real)
    # a shorter output drops the samples beyond it and writes nothing out of bounds
    short, k2 = sc.emu_extract(exe, tmp_path, x, max(1, n_out // 2), True, False)
    assert same_bits(short, moved[:max(1, n_out // 2)]) and np.array_equal(k2, kept)


@pytest.mark.parametrize("row", ssc.MA_ROWS, ids=lambda r: f"n{r['n']}_N{r['N']}_{r['cols']}x{r['dtype']}")
def test_moving_average_rows(exe, tmp_path, row):
    x = ssc.ma_input(row)
    want = rs.moving_average_direct(x, row["N"])
    got = sc.emu_moving_average(exe, tmp_path, x, row["N"])
    assert got.dtype == (np.float64 if x.dtype.kind == "f" else np.complex128) and got.shape == x.shape
    e, ok = sc.close(got, want)
    assert ok, e


@pytest.mark.parametrize("name", sc.MA_CASES)
def test_moving_average_fixtures(exe, tmp_path, name):
    g = sc.load(name)
    e, ok = sc.close(sc.emu_moving_average(exe, tmp_path, g["x"], g["cfg"]["N"]), g["y"])
    assert ok, (name, e)


def check_bert(s, Irx, bits):
    """The ten scalars against the restatement; returns the largest relative error of the computed ones."""
    _, _, want = rs.bert(Irx, bits)
    assert (int(s[0]), int(s[1])) == (want.n1, want.n0)
    errs = [abs(s[i] - getattr(want, k)) / max(abs(getattr(want, k)), 1e-300) for i, k in ((2, "I1"), (3, "I0"), (6, "Id"), (7, "Q"))]
    scale = max(want.std1, want.std0)
    errs += [abs(s[4] - want.std1) / scale, abs(s[5] - want.std0) / scale]
    assert max(errs) <= sc.TOL, errs
    # samples within 1e-9 max |Irx| of the threshold may fall either way (none in the fixtures; the single sample of a one-sample class
    # sits exactly on it)
    unsure = int(np.count_nonzero(np.abs(Irx - want.Id) < sc.ID_GAP * np.max(np.abs(Irx))))
    assert abs(int(s[8]) - want.errors) <= unsure and s[8] == int(s[8])
    return max(errs), unsure


@pytest.mark.parametrize("row", ssc.BERT_ROWS, ids=lambda r: f"n{r['n']}_{r['ones']}_{r['bits_dtype']}")
def test_bert_rows(exe, tmp_path, row):
    Irx, bits = ssc.bert_input(row)
    assert bits.dtype.name == row["bits_dtype"]
    _, unsure = check_bert(sc.emu_bert(exe, tmp_path, Irx, bits), Irx, bits)
    assert unsure == (1 if row["ones"] in (1, row["n"] - 1) else 0)


@pytest.mark.parametrize("name", sc.BERT_CASES)
def test_bert_fixtures(exe, tmp_path, name):
    g = sc.load(name)
    bits = g["bits"]
    if g["cfg"]["drawn"]:
        np.random.seed(g["cfg"]["seed"])
        bits = np.random.randint(2, size=g["Irx"].size)
    s = sc.emu_bert(exe, tmp_path, g["Irx"], bits)
    _, unsure = check_bert(s, g["Irx"], bits)
    assert unsure == 0 and int(s[8]) == int(g["errors"]) and abs(s[7] - float(g["Q"])) <= sc.TOL * abs(float(g["Q"]))


@pytest.mark.parametrize("name", [n for n in sc.SYNC_CASES if sc.load(n)["cfg"]["reference"] == "symbols"])
def test_the_fixtures_glue(exe, tmp_path, name):
    """Tile and extraction on the fixtures' own sequences: the emulator's tiles through the restated symbolSync give the reference's
    symbols."""
    import sync_restatement as srs
    g = sc.load(name)
    cfg = g["cfg"]
    rx, tx = g["rx"], g["tx"]
    n_rx = len(rx)
    n_pad = n_rx + int(g["padL"])
    rx_pad, tiled = sc.emu_tile(exe, tmp_path, rx, tx, n_pad, cfg["SpS"])
    aligned, info = srs.symbolSync(rx_pad, tiled.copy(), 1, cfg["syncMode"])
    got, kept = sc.emu_extract(exe, tmp_path, np.ascontiguousarray(aligned[:n_rx]), n_rx // cfg["SpS"] + 1, True, True)
    assert np.array_equal(kept, g["kept"])
    want = g["symb"].astype(np.complex128)
    e, ok = sc.close(got, want, cfg["ref_tol"])
    assert ok, (name, e)
