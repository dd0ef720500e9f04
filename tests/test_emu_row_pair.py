"""Paired row stage (fused_kernels.h, the note at Ctrl::last_nit; FusedCore::run_span) on the emulated kernels.

In a fixed-step run the row launch in front of a step's final stage also runs the first half step of the next step, from the
values it still holds, and the host leaves that step's own row launch out.  Each sandwich is the code of an unpaired launch, so
the paired run must equal the unpaired one bit for bit, with the same counters, in fewer launches.  SSF_ROW_PAIR=1 forces the
pairing on at these under-filled sizes (by default it is on only where the field fills the chip)."""
import numpy as np
import pytest

import emu_binding as eb
from helpers import load_golden, synth_field

N = 1 << 12
COUNTERS = ("steps", "iterations", "nonconverged_steps", "rebuilt_iterates", "recovered_fields")
# two spans of ten steps of 0.08 and a short (rounding-sized) last one
BASE = dict(func="manakovSSF", alpha=0.2, D=16, gamma=1.3, Fc=193.1e12, Fs=512e9, maxIter=10, tol=1e-5, prgsBar=False,
            Ltotal=1.6, Lspan=0.8, hz=0.08, nlprMethod=False, amp="ideal", saveSpanN=[], prec="complex128")


def _field(p_dbm=8.4):
    return synth_field(N, 2, 43, p_dbm).astype(np.complex128)


def _both(monkeypatch, E, cfg):
    """(field, info) of the unpaired and of the paired run; fields and counters must agree."""
    monkeypatch.setenv("SSF_ROW_V", "16")
    monkeypatch.setenv("SSF_COL_V", "16")
    res = {}
    for pair in ("0", "1"):
        monkeypatch.setenv("SSF_ROW_PAIR", pair)
        res[pair] = eb.run("manakovSSF", E, cfg, trace=False)
    (a, ia), (b, ib) = res["0"], res["1"]
    print({k: (ia[k], ib[k]) for k in COUNTERS + ("launches",)})
    assert np.array_equal(a, b)
    for k in COUNTERS:
        assert ia[k] == ib[k], k
    return ia, ib


def _spans(cfg):
    return int(round(cfg["Ltotal"] / cfg["Lspan"]))


def test_paired_run_equals_the_unpaired_run_in_fewer_launches(monkeypatch):
    """Every step that a step of the same size follows in its span is paired with it: all but the last two of a span that ends in
    a short step.  One launch less per paired boundary: steps - 2 spans here, at least steps - 2 spans - 2 asked for."""
    ia, ib = _both(monkeypatch, _field(), BASE)
    assert ia["steps"] == 22
    assert ia["launches"] - ib["launches"] >= ia["steps"] - 2 * _spans(BASE) - 2


@pytest.mark.parametrize("kw", [dict(maxIter=1), dict(p=-10.0), dict(p=11.0, Lspan=6.0, Ltotal=6.0, alpha=3.0)],
                         ids=["one_iteration", "weak_nonlinearity", "iteration_count_falls"])
def test_paired_run_where_the_pattern_is_disturbed(monkeypatch, kw):
    """maxIter = 1: the final iterate is iterate 0 and its lim_0 sums wait, through the H stage, for the next row launch.
    Weak nonlinearity: iterates are rebuilt as final (the row launch behind a rebuild pairs as well).  A lossy span: the
    iteration count falls inside the span, so the host's pattern is wrong for a step and finds the state again."""
    kw = dict(kw)
    weak = kw.get("p", 0.0) < 0
    E = _field(kw.pop("p", 8.4))
    cfg = dict(BASE, **kw)
    ia, ib = _both(monkeypatch, E, cfg)
    assert ia["launches"] - ib["launches"] >= ia["steps"] - 2 * _spans(cfg) - 2
    if weak:                                            # the cases are what they say: iterates are rebuilt ...
        assert ia["rebuilt_iterates"] > 0
    if "alpha" in kw:                                   # ... the iteration count changes inside the span
        monkeypatch.setenv("SSF_ROW_PAIR", "0")
        _, it = eb.run("manakovSSF", E, cfg)
        assert len(set(it["iters"])) > 1


def test_paired_run_with_recovered_step_start_fields(monkeypatch):
    """tol just above the lower bound of lim_0 at some steps (the bound is about lim_0 / 4.3 for this field): those steps need the
    exact lim_0, and the first of them in a span finds a sparse field and recovers the field at the step start from E_hd, into
    the buffer whose other half of the ping-pong took the paired launch's spectrum.  The factors are the ones at which that
    happens while rebuilds stay rare enough for the call to keep the stage pattern (9 ... 13 rebuilt iterates in 22 steps; from
    14 on the host goes back to the general kernel, which does not pair), so every run recovers a field and must still save one
    launch per paired boundary: the same bound as in the undisturbed run."""
    E = _field()
    monkeypatch.setenv("SSF_ROW_V", "16")
    monkeypatch.setenv("SSF_COL_V", "16")
    monkeypatch.setenv("SSF_ROW_PAIR", "0")
    _, it = eb.run("manakovSSF", E, BASE)
    lim0 = sorted(float(l[0]) for l in it["lims"])
    for f in (0.23240, 0.23244, 0.23246):
        cfg = dict(BASE, tol=lim0[len(lim0) // 2] * f)
        ia, ib = _both(monkeypatch, E, cfg)
        assert ib["recovered_fields"] > 0 and ib["rebuilt_iterates"] > 0, f
        assert ia["launches"] - ib["launches"] >= ia["steps"] - 2 * _spans(cfg) - 2, f


def test_adaptive_step_is_not_paired(monkeypatch):
    ia, ib = _both(monkeypatch, _field(), dict(BASE, nlprMethod=True, maxNlinPhaseRot=2e-3))
    assert ia["launches"] == ib["launches"]


def test_pairing_is_off_by_default_where_the_field_does_not_fill_the_chip(monkeypatch):
    """Without the knob an under-filled plan enqueues what it did before the paired stage existed: the fixed-step golden vector
    of the launch-sequence test (N = 1024, 80 steps, 240 iterations) takes its 656 launches, and the forced-off run of the
    shape above takes as many launches as the default one."""
    monkeypatch.delenv("SSF_ROW_PAIR", raising=False)
    d, cfg = load_golden("mk_fix_p8_ideal_2span")
    _, info = eb.run("manakovSSF", d["Ei"], cfg)
    assert (info["steps"], info["iterations"], info["launches"]) == (80, 240, 656)
    monkeypatch.setenv("SSF_ROW_V", "16")
    monkeypatch.setenv("SSF_COL_V", "16")
    E = _field()
    a, ia = eb.run("manakovSSF", E, BASE, trace=False)
    monkeypatch.setenv("SSF_ROW_PAIR", "0")
    b, ib = eb.run("manakovSSF", E, BASE, trace=False)
    assert np.array_equal(a, b) and ia["launches"] == ib["launches"]
