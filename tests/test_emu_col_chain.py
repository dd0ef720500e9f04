"""Chained column stage (fused_kernels.h: col_body, kChain; FusedCore::run_span) on the emulated kernels.

After a paired row launch the final stage of a step and the H stage of the next one are two column launches back to back on the
same tile of the same workgroup.  With SSF_COL_CHAIN=1 the H kernel carries the final stage's observing part and goes on with the H
stage in the same launch; the host leaves out the FIN launch and the next step's row and H launches.  Every part is the code of
the unchained launches, so the chained run must equal the paired and the unpaired run bit for bit, with the same counters, in one
column launch less per paired boundary.  SSF_ROW_PAIR=1 forces the pairing on at these under-filled sizes."""
import numpy as np
import pytest

import emu_binding as eb
from helpers import load_golden, synth_field

N = 1 << 12
COUNTERS = ("steps", "iterations", "nonconverged_steps", "rebuilt_iterates", "recovered_fields")
# two spans of ten steps of 0.08 and a short (rounding-sized) last one: the BASE of tests/test_emu_row_pair.py
BASE = dict(func="manakovSSF", alpha=0.2, D=16, gamma=1.3, Fc=193.1e12, Fs=512e9, maxIter=10, tol=1e-5, prgsBar=False,
            Ltotal=1.6, Lspan=0.8, hz=0.08, nlprMethod=False, amp="ideal", saveSpanN=[], prec="complex128")
# (a) unpaired, (b) paired and not chained, (c) paired and chained
RUNS = dict(a=dict(SSF_ROW_PAIR="0"), b=dict(SSF_ROW_PAIR="1", SSF_COL_CHAIN="0"), c=dict(SSF_ROW_PAIR="1", SSF_COL_CHAIN="1"))


def _field(p_dbm=8.4):
    return synth_field(N, 2, 43, p_dbm).astype(np.complex128)


def _three(monkeypatch, E, cfg):
    """info of the runs (a), (b), (c); fields and counters must agree."""
    monkeypatch.setenv("SSF_ROW_V", "16")
    monkeypatch.setenv("SSF_COL_V", "16")
    res = {}
    for name, env in RUNS.items():
        monkeypatch.delenv("SSF_COL_CHAIN", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        res[name] = eb.run("manakovSSF", E, cfg, trace=False)
    monkeypatch.delenv("SSF_COL_CHAIN", raising=False)
    (a, ia), (b, ib), (c, ic) = res["a"], res["b"], res["c"]
    print({k: (ia[k], ib[k], ic[k]) for k in COUNTERS + ("launches",)})
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for k in COUNTERS:
        assert ia[k] == ib[k] == ic[k], k
    return ia, ib, ic


def _spans(cfg):
    return int(round(cfg["Ltotal"] / cfg["Lspan"]))


def test_chained_run_equals_the_paired_run_in_fewer_launches(monkeypatch):
    """Every paired boundary saves one more launch: FIN + H in one.  steps - 2 spans boundaries here, at least
    steps - 2 spans - 2 asked for (the bound and the slack of the row-pair test; both runs take the same first short chunk)."""
    ia, ib, ic = _three(monkeypatch, _field(), BASE)
    assert ia["steps"] == 22
    assert ib["launches"] - ic["launches"] >= ia["steps"] - 2 * _spans(BASE) - 2


def test_chained_run_with_one_iteration_per_step(monkeypatch):
    """maxIter = 1: the final iterate is iterate 0, and the lim_0 sums of the observing part wait through the chained H stage for
    the next row launch."""
    cfg = dict(BASE, maxIter=1)
    ia, ib, ic = _three(monkeypatch, _field(), cfg)
    assert ib["launches"] - ic["launches"] >= ia["steps"] - 2 * _spans(cfg) - 2


@pytest.mark.parametrize("kw", [dict(p=-10.0), dict(p=11.0, Lspan=6.0, Ltotal=6.0, alpha=3.0)],
                         ids=["weak_nonlinearity", "iteration_count_falls"])
def test_chained_run_where_the_pattern_is_disturbed(monkeypatch, kw):
    """Weak nonlinearity: iterates are rebuilt as final, and the rebuild rides in the kernel at the step-end slot.  A lossy span:
    the iteration count falls inside the span, the host's pattern is wrong for a step and finds the state again.  Chaining must
    not lose what pairing gained over the unpaired run."""
    kw = dict(kw)
    weak = kw.get("p", 0.0) < 0
    E = _field(kw.pop("p", 8.4))
    cfg = dict(BASE, **kw)
    ia, ib, ic = _three(monkeypatch, E, cfg)
    assert ia["launches"] - ic["launches"] >= ia["steps"] - 2 * _spans(cfg) - 2
    if weak:
        assert ia["rebuilt_iterates"] > 0
    if "alpha" in kw:
        monkeypatch.setenv("SSF_ROW_PAIR", "0")
        _, it = eb.run("manakovSSF", E, cfg)
        assert len(set(it["iters"])) > 1


def test_chained_run_with_recovered_step_start_fields(monkeypatch):
    """The three tol factors of test_emu_row_pair.py's recovery test: steps that need the exact lim_0 find a sparse field and
    recover the field at the step start; the recovery stages ride in the kernel that also chains."""
    E = _field()
    monkeypatch.setenv("SSF_ROW_V", "16")
    monkeypatch.setenv("SSF_COL_V", "16")
    monkeypatch.setenv("SSF_ROW_PAIR", "0")
    _, it = eb.run("manakovSSF", E, BASE)
    lim0 = sorted(float(l[0]) for l in it["lims"])
    for f in (0.23240, 0.23244, 0.23246):
        cfg = dict(BASE, tol=lim0[len(lim0) // 2] * f)
        ia, ib, ic = _three(monkeypatch, E, cfg)
        assert ic["recovered_fields"] > 0, f
        assert ia["launches"] - ic["launches"] >= ia["steps"] - 2 * _spans(cfg) - 2, f


def test_adaptive_step_is_not_chained(monkeypatch):
    ia, ib, ic = _three(monkeypatch, _field(), dict(BASE, nlprMethod=True, maxNlinPhaseRot=2e-3))
    assert ic["launches"] == ia["launches"]


def test_chaining_is_off_by_default_where_the_field_does_not_fill_the_chip(monkeypatch):
    """No knobs set: an under-filled plan enqueues what it did before (the golden vector of the launch-sequence test takes its
    656 launches), and the default run of the shape above takes as many launches as SSF_COL_CHAIN=0."""
    monkeypatch.delenv("SSF_ROW_PAIR", raising=False)
    monkeypatch.delenv("SSF_COL_CHAIN", raising=False)
    d, cfg = load_golden("mk_fix_p8_ideal_2span")
    _, info = eb.run("manakovSSF", d["Ei"], cfg)
    assert (info["steps"], info["iterations"], info["launches"]) == (80, 240, 656)
    monkeypatch.setenv("SSF_ROW_V", "16")
    monkeypatch.setenv("SSF_COL_V", "16")
    E = _field()
    a, ia = eb.run("manakovSSF", E, BASE, trace=False)
    monkeypatch.setenv("SSF_COL_CHAIN", "0")
    b, ib = eb.run("manakovSSF", E, BASE, trace=False)
    assert np.array_equal(a, b) and ia["launches"] == ib["launches"]
