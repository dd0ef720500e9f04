"""The carrier-recovery restatement (tests/cpr_restatement.py) and its case table (tests/cpr_shape_cases.py) without a GPU.

The restatement is held to the reference's nine recorded fixtures and, at short lengths, to np.unwrap itself; then every row of
the table that the g++ emulator of the kernel bodies (tests/emu/emu_cpr.cpp, run_emu of tests/test_cpr_emu.py) can run is held
to the bounds of tests/test_gpu_cpr_shapes.py: raw test phases bit-equal wherever the restatement's margin is >= 1e-9 (for a
crafted row: everywhere, and equal to the crafted sequence), unwrapped phases within 1e-9 rad of the extended-precision unwrap
of the emulator's own raw phases, sigOut and the frequency-compensated signal within 1e-9 (rel-L2 and per element), fo equal to
numpy's grid value.  Every row's conditions are checked on the restatement alone, the GPU-only row's too.

The emulator replaces every workgroup-level structure by a sequential loop, so it shows faults of the bodies (the unwrap rule,
the fftshift index) and of its own copy of the running minimum (the all-zero rows, where every test phase ties exactly), and
validates table and reference; the segmented prefix sums, the chunks of test phases, the kernel's running minimum across them,
the tree scan and the grid-stride loops are the GPU file's to judge."""
import numpy as np
import pytest

import cpr_cases as cc
import cpr_restatement as cr
import cpr_shape_cases as sc
from opticommpy_amd import cpr as ocpr
from test_cpr_emu import BPS, CPR, FOE, emu, run_emu  # noqa: F401  (emu: the fixture that compiles the emulator)


@pytest.mark.parametrize("name", cc.EXPECTED_CASES)
def test_restatement_matches_the_reference(name):
    g = cc.load(name)
    cc.check_conditions(g)
    cfg = g["cfg"]
    table = ocpr._table(cfg["M"], cfg["constType"], cfg["param"].get("shapingFactor", 0))
    w = cr.restate(g["sigIn"], table, cfg["N"] // 2, cfg["B"], cfg["foe"], cfg["P"], 1 / cfg["Ts"])
    shape = g["sigIn"].shape
    assert w["left_out"] == 0 and w["min_margin"] >= 1e-7
    cc.compare_phases(w["raw"].reshape(shape), g["raw"], cc.RAW_ABS, f"{name} raw")
    cc.compare_phases(w["phase"].astype(np.float64).reshape(shape), g["phaseEst"], cc.PHASE_ABS, f"{name} phaseEst")
    cc.compare_signal(w["sig"].astype(np.complex128).reshape(shape), g["sigOut"], f"{name} sigOut")
    if cfg["foe"]:
        assert np.array_equal(w["fo"], g["fo"]) and np.all(w["foe_margin"] >= 1e-6)
        # (the reference rounds the compensated signal of a complex64 input to single precision: compared in the input's type)
        cc.compare_signal(w["sig_foe"].astype(g["sig_foe"].dtype).astype(np.complex128).reshape(shape),
                          g["sig_foe"].astype(np.complex128), f"{name} fourthPowerFOE")


def test_unwrap_is_numpys_where_numpy_does_not_drift():
    """Every crafted row of up to 4097 symbols: the written-out recurrence against np.unwrap, exact-pi jumps included."""
    rows = [r for r in sc.ROWS if r.gen == "crafted" and r.n <= 4097]
    assert len(rows) >= 20
    for row in rows:
        raw = cr.phase_grid(row.B)[sc.crafted_index(row)]
        phase, cond = cr.unwrap(raw)
        want = np.unwrap(4 * raw, axis=0) / 4
        e = float(np.max(np.abs(phase - want)))
        assert e <= 1e-12, (row.id, e)


@pytest.mark.parametrize("M", [4, 16])
@pytest.mark.parametrize("B", [2, 8, 64, 1024])
def test_crafted_decisions_are_known_exactly(emu, tmp_path, M, B):
    """x = table[s] exp(-1j testph[b]) + 1e-4 noise under a window of one symbol: restatement and emulator return testph[b]
    at every symbol, with a margin of at least 7 between the two smallest distances.  16-QAM at B = 1024 draws s from the four
    corner points: an inner point, 0.45 from the origin, moves 6.9e-4 per test phase while the noise reaches 4e-4 (a margin of
    0.8 with all 16 points); a corner, 1.34 from the origin, moves 2.1e-3."""
    gen = "corners" if (M, B) == (16, 1024) else "crafted"
    row = sc._row("crafted", "cpr", gen, 600, 2, M, 0, B, 700 + B)
    sc.check_conditions(row)
    want = sc.expected(row)
    print(f"M = {M}, B = {B}: smallest margin {want['min_margin']:.1f}")
    assert want["min_margin"] >= 7
    raw = run_emu(emu, tmp_path, BPS, sc.signal(row), sc.table(row), 0, B)
    grid = np.arange(B) * (np.pi / 2) / B
    assert np.array_equal(raw, grid[sc.crafted_index(row)]) and np.array_equal(want["raw"], raw)


def emulate(exe, tmp, row):
    x, table = sc.signal(row), sc.table(row)
    if row.kind == "bps":
        return dict(raw=run_emu(exe, tmp, BPS, x, table, row.Nh, row.B))
    if row.kind == "foe":
        sig_foe, fo = run_emu(exe, tmp, FOE, x, table, P=row.P, Fs=row.Fs)
        return dict(sig_foe=sig_foe, fo=fo)
    foe = row.kind == "cprfoe"
    sig, phase, raw, fo = run_emu(exe, tmp, CPR, x, table, row.Nh, row.B, int(foe), row.P, row.Fs)
    got = dict(sig=sig, phase=phase, raw=raw)
    if foe:
        got["fo"] = fo
    return got


@pytest.mark.parametrize("row", sc.EMU_ROWS, ids=lambda r: r.id)
def test_emulated_kernels_match_the_restatement(emu, tmp_path, row):
    sc.check_conditions(row)
    sc.compare(row, emulate(emu, tmp_path, row), "emulator")


def test_rows_the_emulator_skips_meet_their_conditions():
    rows = [r for r in sc.ROWS if not r.emu]
    assert [r.id for r in rows] == ["foe-M4-263169x2-Nh2-B8-P4"]
    for row in rows:
        sc.check_conditions(row)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_a_flat_spectrum_takes_the_first_position_of_fftshift(emu, tmp_path, n):
    """A position of the maximum search is a position of np.fft.fftshift: the transform of a single pulse is 1 in every bin
    (the emulator's DFT gives exactly that; numpy's own transform is a few ulp off at 243 and 257, so it is not asked), all n
    bins tie, and np.argmax's rule takes position 0, the most negative frequency -(n // 2) Fs / n.  (The positions are labels
    used twice, for the bin that is read and for the frequency that is returned, so an enumeration that starts elsewhere
    gives the same fo wherever one bin is the largest: only a tie tells.)"""
    x = np.zeros((n, 1), dtype=np.complex128)
    x[0] = 1.0
    want = np.fft.fftshift(np.fft.fftfreq(n))[np.argmax(np.ones(n))]
    assert want == -(n // 2) / n
    y, got = run_emu(emu, tmp_path, FOE, x, np.ones(2), P=1, Fs=1.0)
    assert got[0] == want, (n, got, want)
    assert np.array_equal(y, x)
