"""The numpy restatement of the OFDM functions (tests/ofdm_restatement.py) against the reference-generated fixtures, at the bounds
of tests/ofdm_cases.py: it is the yardstick of the shape tests, so it is held to the reference first.  No GPU, no library."""
import numpy as np
import pytest

import ofdm_cases as oc
import ofdm_restatement as rs


def test_every_case_has_its_fixture():
    import glob
    import os
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(oc.GOLDEN, "*.npz"))) == oc.CASES


@pytest.mark.parametrize("name", oc.CASES)
def test_fixture_meets_its_conditions(name):
    oc.check_conditions(oc.load(name))


@pytest.mark.parametrize("name", oc.CASES)
def test_restated_modulator_matches_the_reference(name):
    g = oc.load(name)
    want = rs.modulate(g["symb"], **oc.kwargs(g))
    assert want.dtype == np.complex128
    # the stored distance is the one from the reference's output to this computation
    d = np.max(np.abs(g["tx"] - want)) / np.max(np.abs(want))
    assert d == float(g["dist_mod"])
    oc.check_mod(g, want.astype(np.complex64), np.complex64)
    # complex64 symbols: the frame holds the same values
    assert np.array_equal(rs.modulate(g["symb"].astype(np.complex64).astype(np.complex128), **oc.kwargs(g)).astype(np.complex64),
                          rs.modulate(g["symb"].astype(np.complex64), **oc.kwargs(g)).astype(np.complex64))


@pytest.mark.parametrize("name", oc.CASES)
def test_restated_demodulator_matches_the_reference(name):
    g = oc.load(name)
    rx = g["rx"].copy()
    got, H = rs.demodulate(rx, **oc.kwargs(g))
    assert np.array_equal(rx, g["rx"])                                  # the signal is not written
    oc.check_demod(g, got, H, np.complex128)
    got, H = rs.demodulate(g["rx"].astype(np.complex64), **oc.kwargs(g))
    oc.check_demod(g, got.astype(np.complex64), H, np.complex64)


def test_the_path_over_an_array_of_frames_is_byte_equal_to_the_loops():
    """``modulate_frames`` / ``demodulate_frames`` restate the big row (116 600 frames); the loops stay the yardstick, so the two
    must agree to the byte on every shape row and every fixture, with and without turned frames, in both input types."""
    import ofdm_shape_cases as sc
    for row in sc.ROWS:
        c = sc.make(row)
        assert row.frames < sc.LOOP_FRAMES                              # c.tx, c.dem and c.H are the loops'
        assert rs.modulate_frames(c.symb, **c.kwargs).tobytes() == c.tx.tobytes(), row.id
        assert rs.modulate_frames(c.symb.astype(np.complex64), **c.kwargs).tobytes() == c.tx.tobytes(), row.id
        for x, (dem, H) in ((c.rx, (c.dem, c.H)), (c.rx.astype(np.complex64), rs.demodulate(c.rx.astype(np.complex64), **c.kwargs))):
            got, Hg = rs.demodulate_frames(x, **c.kwargs)
            assert got.tobytes() == dem.tobytes() and np.asarray(Hg).tobytes() == np.asarray(H).tobytes(), row.id
    for name in oc.CASES:
        g = oc.load(name)
        assert rs.modulate_frames(g["symb"], **oc.kwargs(g)).tobytes() == rs.modulate(g["symb"], **oc.kwargs(g)).tobytes()
        (got, H), (dem, Hw) = rs.demodulate_frames(g["rx"], **oc.kwargs(g)), rs.demodulate(g["rx"], **oc.kwargs(g))
        assert got.tobytes() == dem.tobytes() and np.asarray(H).tobytes() == np.asarray(Hw).tobytes()


def test_every_shape_row_meets_its_conditions():
    """The conditions of tests/ofdm_shape_cases.py hold on the restatement alone: quadrants, distance from the cut, the mean
    angle of the alternating rows, the line of the delay rows beyond pi, |H| >= 0.3 -- and the big row is restated by the
    array path."""
    import ofdm_shape_cases as sc
    for row in sc.ROWS + sc.BIG_ROWS:
        sc.check_conditions(sc.make(row))
    assert all(r.frames >= sc.LOOP_FRAMES for r in sc.BIG_ROWS)
    assert {sc.kind(r) for r in sc.EMU_ROWS} == {None, "II", "III", "alternating", "delay"}


def test_the_loop_closes_without_a_channel():
    g = oc.load("nb_pilots")
    k = oc.kwargs(g)
    tx = rs.modulate(g["symb"], **k)
    got, H = rs.demodulate(np.sqrt(k["SpS"]) * tx[::k["SpS"]], **k)
    # the frame holds the pilot in single precision, the estimate divides by the pilot in double
    h = complex(np.complex64(k["pilot"])) / k["pilot"]
    assert np.max(np.abs(H - h)) <= 1e-12 and np.max(np.abs(got * h - g["symb"].astype(np.complex64))) <= 1e-12
