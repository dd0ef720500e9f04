"""tests/syncdata_restatement.py held to the reference's recorded results (tests/golden/syncdata/*.npz,
tools/gen_golden_syncdata.py) before anything else is held to it, and the shape rows' own conditions: every row the emulator and the
GPU run has one right answer."""
import numpy as np
import pytest

import syncdata_cases as sc
import syncdata_restatement as rs
import syncdata_shape_cases as ssc


@pytest.mark.parametrize("name", sc.SYNC_CASES)
def test_sync_restatement_matches_the_reference(name):
    g = sc.load(name)
    sc.check_conditions(g)
    cfg = g["cfg"]
    tx_, symb, info = sc.restate(g["rx"], g["tx"], sc.param_of(cfg))
    sc.check_info(info, cfg["reference"])
    assert info.margin == float(g["margin"]) and info.padL == int(g["padL"])
    real = g["rx"].dtype.kind != "c" and g["tx"].dtype.kind != "c"
    assert tx_.dtype == symb.dtype == (np.float64 if real else np.complex128)
    assert tx_.shape == g["tx_"].shape and symb.shape == g["symb"].shape
    e_tx, ok_tx = sc.close(tx_, g["tx_"].astype(tx_.dtype), cfg["ref_tol"])
    e_sy, ok_sy = sc.close(symb, g["symb"].astype(symb.dtype), cfg["ref_tol"])
    print(f"{name}: tx_ {e_tx:.2e}  symb {e_sy:.2e}")
    assert ok_tx and ok_sy, (name, e_tx, e_sy)
    if cfg["reference"] == "signal":
        assert np.array_equal(tx_, g["tx_"].astype(tx_.dtype)), name           # only moved
    else:
        assert np.array_equal(info.kept, g["kept"]), name
        if cfg["zeros"]:                                                        # the zero points were dropped: fewer kept than symbols seen
            assert info.kept[0] < -(-len(g["rx"]) // cfg["SpS"]) - 5


@pytest.mark.parametrize("name", sc.MA_CASES)
def test_moving_average_restatement_matches_the_reference(name):
    g = sc.load(name)
    sc.check_conditions(g)
    for f in (rs.moving_average, rs.moving_average_direct):
        e, ok = sc.close(f(g["x"], g["cfg"]["N"]), g["y"], 1e-14)
        assert ok, (name, f.__name__, e)
    with pytest.raises(ValueError):
        rs.moving_average(g["x"], 1)


@pytest.mark.parametrize("name", sc.BERT_CASES)
def test_bert_restatement_matches_the_reference(name):
    g = sc.load(name)
    sc.check_conditions(g)
    cfg = g["cfg"]
    bits = g["bits"]
    if cfg["drawn"]:
        np.random.seed(cfg["seed"])
        bits = np.random.randint(2, size=g["Irx"].size)
    ber, q, s = rs.bert(g["Irx"], bits)
    assert s.errors == int(g["errors"]) == round(float(g["BER"]) * g["Irx"].size) and abs(q - float(g["Q"])) <= 1e-12 * abs(q)
    assert s.id_gap >= sc.ID_GAP


@pytest.mark.parametrize("row", ssc.SYNC_ROWS, ids=lambda r: r["name"])
def test_sync_rows_have_one_right_answer(row):
    rx, tx = ssc.sync_input(row)
    assert rx.dtype.name == row["rx_dtype"] and tx.dtype.name == row["tx_dtype"] and rx.ndim == (1 if row["modes"] == 0 else 2)
    tx_, symb, info = sc.restate(rx, tx, ssc.sync_param(row))
    real = rx.dtype.kind != "c" and tx.dtype.kind != "c"
    sc.check_info(info, row["reference"], real_mode_on_real=real and row["syncMode"] == "real")
    if "perm" in row:
        assert info.sync.swap.tolist() == row["perm"]
    if row["name"] == "kept_beyond_B":
        assert info.kept[0] > ssc.B
    if row["name"] == "ook_zeros_dropped":
        assert np.all(info.kept < 0.75 * len(rx) / row["SpS"])
    assert tx_.shape == rx.shape and symb.ndim == 2


def test_extract_rows_sit_at_the_edges():
    kept = {}
    for row in ssc.EXTRACT_ROWS:
        x = ssc.extract_input(row)
        moved, symb, k = rs.extract(x, row["n"] // row["SpS"] + 1)
        kept[row["name"]] = (k, row["n"] // row["SpS"] + 1)
        assert np.allclose(np.sqrt(np.mean(np.abs(symb[:k[0], 0]) ** 2)), 1.0)
    B = ssc.B
    assert [int(kept[f"kept_{s}"][0][0]) for s in ("B-1", "B", "B+1", "2B+1")] == [B - 1, B, B + 1, 2 * B + 1]
    assert kept["sps2_kept_B+1"][0].tolist() == [B + 1, B + 1] and kept["sps2_kept_B+1"][1] == B + 2       # one less than symb's rows
    assert kept["sps2_fills_every_row"][0].tolist() == [B + 1] and kept["sps2_fills_every_row"][1] == B + 1
    assert len(set(kept["eight_modes"][0].tolist())) > 1 and kept["zeros_among_symbols"][0].max() < 1500
