"""Every row of tests/eq_shape_cases.py through the g++ emulation of the equalizer's kernel bodies (tests/emu/emu_eq.cpp includes
opticommpy_amd/csrc/eq_kernels.h) against the numpy restatement at eq_cases.REL, after the row's conditions were checked on the
restated values alone.  The emulation leaves out the chunking, the prefetch and the walk over segments: those are judged by the
same rows on the GPU (tests/test_gpu_eq_shapes.py).  What it can judge of the launch geometry it does: the header's
chunk_symbols and coeffs_per_lane for the row's geometry, which it prints."""
import subprocess

import numpy as np
import pytest

import eq_cases as ec
import eq_shape_cases as sc
from opticommpy_amd import _lib
from test_eq_emu import emu, run_emu  # noqa: F401  (the module-scoped fixture that compiles the emulator)


def geometry(exe, tmp):
    """(chunk_symbols, coeffs_per_lane) of eq_kernels.h for the input run_emu wrote last."""
    out = subprocess.check_output([exe, str(tmp / "in.bin"), str(tmp / "out.bin")]).decode().split()
    return int(out[out.index("chunk") + 1]), int(out[out.index("coeffs_per_lane") + 1])


@pytest.mark.parametrize("name", [r.id for r in sc.ROWS])
def test_emulated_kernels_match_the_restatement_on_every_row(emu, tmp_path, name):  # noqa: F811
    row = sc.BY_ID[name]
    sc.check_conditions(row)
    x, prm, tx = sc.build(row)
    got = run_emu(emu, tmp_path, x, prm, tx)
    sc.compare(row, got, "emu")
    sc.zero_regions(row, got[0], got[2])
    modes = max(row.modes, 1)
    chunk, R = geometry(emu, tmp_path)
    assert chunk == _lib.eq_chunk(modes, row.taps, row.sps) and R == -(-modes * row.taps // sc.WAVE), (name, chunk, R)
    assert row.chunk is None or chunk == row.chunk, (name, chunk)
    assert ((chunk - 1) * row.sps + row.taps) * modes <= _lib.EQ_STAGE_ELEMS, name
    assert chunk == _lib.EQ_CHUNK or (chunk * row.sps + row.taps) * modes > _lib.EQ_STAGE_ELEMS, name
    if row.xdtype != "complex128" or row.rdtype != "complex128":       # the same values widened on the host: the same bits
        wide = run_emu(emu, tmp_path, *sc.widened(row))
        for a, b in zip(got, wide):
            assert np.array_equal(a, b), name


def test_every_instantiation_and_both_candidate_loops_have_a_row():
    """The six instantiations of k_eq_serial and the two loops over candidates beyond the first of a lane, from the rows' own
    geometry, dtype, M and nRadii."""
    cov = sc.coverage()
    for R in (1, 2, 4):
        for xt in ("Cplx", "CplxF"):
            assert cov.get(f"k_eq_serial<{R}, {xt}>"), (R, xt)
    assert cov.get("points beyond lane + 64") and cov.get("radii beyond lane + 64")
    assert {r.group for r in sc.ROWS} == set(sc.GROUPS)


def test_exact_ties_between_two_radii_exist_from_64_qam_on():
    """16-QAM has none: |R_a - a| == |R_b - a| is false in doubles around the midpoint of both neighbouring pairs of its radii."""
    assert sc.rde_ties(16) == []
    for M, picks in sc.RDE_TIES.items():
        radii = sc.oeq._tables(M, "qam", 0, np.complex128)[2]
        ties = {(lo, hi): a for lo, hi, a in sc.rde_ties(M)}
        for lo, hi in picks:
            a = ties[lo, hi]
            assert hi == lo + 1 and abs(radii[lo] - a) == abs(radii[hi] - a) > 0 and np.sqrt(a * a) == a
        assert any(lo % 2 for lo, _ in picks)


def test_nlms_scale_keeps_the_square_root_round_trip(emu):  # noqa: F811
    """np.linalg.norm(x) ** 2 is sqrt(sum)^2, an ulp off the sum for about half of all doubles: far below eq_cases.REL on any
    signal, so the function is held bit for bit on literal sums that tell the two apart."""
    sums = [0.1, 0.3, 0.7, 1.1, 2.0, 3.0, 5.0, 7.3, 15.0, 29.7, 1e-3, 123.456]
    want = [1.0 / (np.sqrt(np.float64(s)) ** 2) for s in sums]
    assert sum(w != 1.0 / np.float64(s) for w, s in zip(want, sums)) >= 3
    out = subprocess.check_output([emu, "--nlms-scale"] + [float(s).hex() for s in sums]).decode().split()
    assert [float.fromhex(o) for o in out] == want
