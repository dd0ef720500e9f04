"""The numpy restatement of the link metrics (tests/metrics_restatement.py) held to the reference's recorded results, and the
kernel bodies held to the restatement without a GPU.

Restatement against the fixtures: on every fixture of tests/golden/metrics, with discard 0 and with the fixture's discard, BER and
SER are equal and SNR [dB], GMI, NGMI, MI and both EVMs are within 1e-12 relative.  With the package's tables the restatement is
at most 2.6e-15 off (MI of pam128; 1.2e-15 on the blind EVM, 6e-16 on the other values): 1e-12 leaves three orders over that and stays three
orders under the 1e-9 the kernels are held to, so the restatement can stand in for the reference where no fixture exists.

Emulator against the restatement: every row of tests/metrics_shape_cases.py through the g++ emulator of the kernel bodies
(tests/emu/emu_metrics.cpp) at the bounds of tests/test_gpu_metrics_shapes.py.  That finds a fault in a body (a label bit, a
combine step) without a GPU, and shows that every row's conditions hold for the restatement alone."""
import functools

import numpy as np
import pytest

import metrics_cases as mc
import metrics_restatement as mr
import metrics_shape_cases as sc
from opticommpy_amd import _lib
from test_metrics_emu import DEMOD, WANT_ALL, emu, run_emu  # noqa: F401  (emu: the fixture that compiles the emulator)

FIXTURE_REL = 1e-12
VALUES = ("SNR", "GMI", "NGMI", "MI", "EVM", "EVM_blind")


@functools.lru_cache(maxsize=None)
def fixture_errors(name):
    """Largest relative error of each value over the modes and both discards; BER and SER asserted equal."""
    g = mc.load(name)
    cfg = g["cfg"]
    worst = dict.fromkeys(VALUES, 0.0)
    for discard, suffix in ((0, ""), (cfg["discard"], "_d")):
        got = mr.restate(g["rx"], g["tx"], cfg["M"], cfg["constType"], g["px"], discard)
        blind = mr.restate_blind(g["rx"], cfg["M"], cfg["constType"], discard)
        got["EVM_blind"] = blind["EVM"]
        for k in mc.EXACT:
            assert np.array_equal(got[k], g[k + suffix]), (name, k + suffix, got[k], g[k + suffix])
        for k in VALUES:
            assert got[k].shape == g[k + suffix].shape
            worst[k] = max(worst[k], mc.rel_err(got[k], g[k + suffix]))
        if not suffix:
            # the restatement's side conditions are the generator's
            assert np.array_equal(got["bit_errors"], g["bit_errors"]), name
            assert min(got["margin"], blind["margin"]) >= 1e-6
            assert (got["clipped"] > 0) == bool(cfg["clip"]), (name, got["clipped"])
    return worst


@pytest.mark.parametrize("name", mc.EXPECTED_CASES)
def test_restatement_matches_the_fixtures(name):
    worst = fixture_errors(name)
    print(f"{name}: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= FIXTURE_REL, (name, k, v)


def test_largest_error_against_the_fixtures(capsys):
    """Shown whether or not output is captured."""
    worst = {k: max((fixture_errors(name)[k], name) for name in mc.EXPECTED_CASES) for k in VALUES}
    with capsys.disabled():
        print("\nrestatement against the fixtures, largest relative error: "
              + "  ".join(f"{k} {v:.1e} ({name})" for k, (v, name) in worst.items()))
    assert max(v for v, _ in worst.values()) <= FIXTURE_REL


def test_new_width_fixtures_keep_their_likelihood_sums_normal():
    """The fixtures for the label widths 1, 5, 7 and 10 are compared at 1e-9 like the others: no likelihood sum may sit among the
    denormals, where two exp() implementations differ by far more than rounding."""
    for name in ("bpsk_6dB", "psk32", "pam128", "qam1024_1d"):
        g = mc.load(name)
        got = mr.restate(g["rx"], g["tx"], g["cfg"]["M"], g["cfg"]["constType"], g["px"])
        assert got["clipped"] == 0 and got["min_sum"] >= sc.MIN_SUM, (name, got["min_sum"])


@pytest.mark.parametrize("row", sc.ROWS, ids=lambda r: r.id)
def test_emulated_kernels_match_the_restatement(emu, tmp_path, row):  # noqa: F811
    rx, tx, px = sc.arrays(row)
    want = sc.expected(row)
    sc.check_conditions(row, want)
    path = tmp_path / "in.bin"
    if row.kind == "metrics":
        got = run_emu(emu, path, WANT_ALL, rx, tx, row.M, row.ct, px, row.discard)
    elif row.kind == "blind":
        got = run_emu(emu, path, _lib.METRICS_EVM_BLIND, rx, None, row.M, row.ct, None, row.discard)
    else:
        got = {"bits": run_emu(emu, path, DEMOD, rx, None, row.M, row.ct)}
    sc.compare(row, got, want, "emulator")
