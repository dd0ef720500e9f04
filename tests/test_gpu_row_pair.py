"""Paired row stage on the GPU (fused_kernels.h, the note at Ctrl::last_nit): tests/tools/row_pair_check.py in
processes of their own, each under its own time limit, as tests/test_experiments.py starts its checks."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "opticommpy_amd", "libssf_hip_exp.so")
CHECK = os.path.join(ROOT, "tests", "tools", "row_pair_check.py")


def _check(mode, env, limit):
    r = subprocess.run([sys.executable, CHECK, mode], env=dict(os.environ, **env), capture_output=True, timeout=limit)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0, (out[-3000:], r.stderr.decode(errors="replace")[-3000:])
    return out


def _need_exp():
    if not os.path.exists(EXP):
        pytest.skip("experiment library not built (make -C opticommpy_amd/csrc exp)")


@pytest.mark.gpu
def test_paired_rows_against_unpaired_rows_at_the_smallest_stage_specialised_shape():
    """2-pol N = 2^19 complex128, 256-point columns, 12 fixed steps over two spans (with and without a short last step):
    SSF_ROW_PAIR=1 against 0 is bit-equal with equal counters, and the profiled row launches fall by the number of paired
    boundaries.  (2^19 and not 2^16: at 2^16 the column geometry has four columns per workgroup, for which there are no
    stage-specialised kernels, so the pattern that carries the pairing is not enqueued; and the rows of 2^8 would run on the
    run-time-length row kernel, which does not carry the second round.)"""
    _need_exp()
    _check("small", dict(SSF_LIB=EXP), 300)


@pytest.mark.gpu
def test_default_pairing_at_2_20_equals_the_unpaired_experiment_build():
    """The product library pairs by default from 2-pol N = 2^20 complex128 on; the experiment library with SSF_ROW_PAIR=0 runs
    the same kernels unpaired.  Eight steps: the same bits, the same counters, one row launch less per paired boundary."""
    _need_exp()
    env = {k: v for k, v in os.environ.items() if k not in ("SSF_LIB", "SSF_ROW_PAIR")}
    prod = subprocess.run([sys.executable, CHECK, "default"], env=env, capture_output=True, timeout=300)
    assert prod.returncode == 0, (prod.stdout.decode(errors="replace")[-2000:], prod.stderr.decode(errors="replace")[-3000:])
    exp = _check("default", dict(SSF_LIB=EXP, SSF_ROW_PAIR="0"), 300)
    a = [ln for ln in prod.stdout.decode(errors="replace").splitlines() if ln.startswith("digest")]
    b = [ln for ln in exp.splitlines() if ln.startswith("digest")]
    print(a, b)
    assert len(a) == 1 and a == b

    def rows(text):
        w = [ln for ln in text.splitlines() if ln.startswith("row_n")][0].split()
        return int(w[1]), int(w[3])
    (rp, want), (ru, _) = rows(prod.stdout.decode(errors="replace")), rows(exp)
    assert want > 0 and ru - rp == want, (ru, rp, want)              # the default did pair
