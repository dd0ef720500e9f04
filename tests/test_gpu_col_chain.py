"""Chained column stage on the GPU (fused_kernels.h: col_body, kChain): tests/tools/col_chain_check.py in processes
of their own, each under its own time limit, as tests/test_gpu_row_pair.py starts its checks.

Measured on an MI355X at 2^19: bit-equal fields and equal counters, the stage-kernel column launches fall by exactly the paired
boundaries (54 -> 44 and 54 -> 46) and the row launches stay (44, 46)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "opticommpy_amd", "libssf_hip_exp.so")
CHECK = os.path.join(ROOT, "tests", "tools", "col_chain_check.py")
KNOBS = ("SSF_LIB", "SSF_ROW_PAIR", "SSF_COL_CHAIN")


def _check(mode, env, limit):
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([sys.executable, CHECK, mode], env=dict(base, **env), capture_output=True, timeout=limit)
    out = r.stdout.decode(errors="replace")
    print(out)
    assert r.returncode == 0, (out[-3000:], r.stderr.decode(errors="replace")[-3000:])
    return out


def _need_exp():
    if not os.path.exists(EXP):
        pytest.skip("experiment library not built (make -C opticommpy_amd/csrc exp)")


@pytest.mark.gpu
def test_chained_columns_against_unchained_columns_at_the_smallest_stage_specialised_shape():
    """2-pol N = 2^19 complex128, 256-point columns, paired rows, 12 fixed steps over two spans (with and without a short last
    step): SSF_COL_CHAIN=1 against 0 is bit-equal with equal counters, the profiled stage-kernel column launches fall by exactly
    the number of paired boundaries and the row launches stay.  (2^19: the smallest size with stage-specialised column kernels
    and a row kernel that pairs; below it the chained code does not run.)"""
    _need_exp()
    _check("small", dict(SSF_LIB=EXP), 300)


@pytest.mark.gpu
def test_default_at_2_20_equals_the_unchained_experiment_build():
    """The product library's default at 2-pol N = 2^20 complex128 against the experiment library with SSF_COL_CHAIN=0, which
    runs the same kernels unchained.  Eight steps: the same bits, the same counters, the same row launches, and one column launch
    less per paired boundary -- which proves that the default chains."""
    _need_exp()
    prod = _check("default", {}, 300)
    exp = _check("default", dict(SSF_LIB=EXP, SSF_COL_CHAIN="0"), 300)
    a = [ln for ln in prod.splitlines() if ln.startswith("digest")]
    b = [ln for ln in exp.splitlines() if ln.startswith("digest")]
    print(a, b)
    assert len(a) == 1 and a == b

    def counts(text):
        w = [ln for ln in text.splitlines() if ln.startswith("col_sg_n")][0].split()
        return int(w[1]), int(w[3]), int(w[5])
    (cp, rp, want), (cu, ru, _) = counts(prod), counts(exp)
    assert want > 0 and cu - cp == want and ru == rp, (cu, cp, ru, rp, want)
