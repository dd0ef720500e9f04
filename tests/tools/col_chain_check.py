#!/usr/bin/env python3
"""Chained column stage (fused_kernels.h: col_body, kChain; FusedCore::run_span) ON THE GPU, one process per mode:

  small    experiment library (SSF_LIB=.../libssf_hip_exp.so), 2-pol N = 2^19 complex128 with 256-point columns (SSF_SPLIT_L1=8,
           SSF_ROW_V=16, SSF_COL_V=16, SSF_ROW_PAIR=1): the smallest field with stage-specialised column kernels and a row kernel that
           pairs (tests/tools/row_pair_check.py) -- below it the chained code does not run.  12 fixed steps over two spans at 8.4 dBm,
           once with spans of six equal steps and once with five steps and a short last one: SSF_COL_CHAIN=1 against 0 gives
           bit-equal fields, equal counters, and -- HIP-event profiling on -- as many stage-kernel column launches less as there
           are paired boundaries, with the row launches unchanged.
  default  the library's own default at 2-pol N = 2^20 complex128, 8 steps: prints a digest of the result with the counters, and
           the profiled launch counts.  Run once with the product library and once with the experiment library and
           SSF_COL_CHAIN=0; the caller compares the digests and the launch counts.

Exit code 0 = all agree."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import opticommpy_amd as oa  # noqa: E402
from helpers import make_param, synth_field  # noqa: E402
from opticommpy_amd import _lib, models  # noqa: E402

BASE = dict(Fs=512e9, Fc=193.1e12, alpha=0.2, D=16, gamma=1.3, maxIter=10, tol=1e-5, prgsBar=False, nlprMethod=False, amp="ideal",
            saveSpanN=[])
COUNTERS = ("steps", "iterations", "nonconverged_steps", "rebuilt_iterates", "recovered_fields")


def paired_boundaries(hz, Lspan, nspans):
    """Steps that a step of the same size follows in their span, with the device's own arithmetic (pick_hz, z += hz)."""
    n, z = 0, 0.0
    while True:
        h = Lspan - z if Lspan - z < hz else hz
        if not z + h < Lspan:
            break
        z1 = z + h
        h1 = Lspan - z1 if Lspan - z1 < hz else hz
        n += h1 == h
        z = z1
    return n * nspans


def run(E, cfg):
    """Result, counters and the HIP-event launch counts of the second of two calls (the first one gives the plan its history)."""
    models.release_plans()                                   # (the knobs are read when the plan is created)
    oa.manakovSSF(E, make_param(oa.parameters, cfg))
    pl = models._get_plan(E.shape[0], 2, _lib.SSF_C128)
    pl.lib.ssf_set_profiling(pl.h, 1)
    out = oa.manakovSSF(E, make_param(oa.parameters, cfg))
    info = {k: int(models.last_run[k]) for k in COUNTERS}
    kt = _lib.KernelTimes()
    pl.lib.ssf_get_kernel_times(pl.h, C.byref(kt))
    pl.lib.ssf_set_profiling(pl.h, 0)
    info["row_n"] = int(kt.row_n)
    info["col_sg_n"] = int(kt.col_h_n) + int(kt.col_adv_n) + int(kt.col_fin_n)
    return out, info


def small():
    for k, v in dict(SSF_SPLIT_L1="8", SSF_ROW_V="16", SSF_COL_V="16", SSF_ROW_PAIR="1").items():
        os.environ[k] = v
    E = synth_field(1 << 19, 2, 77, 8.4)
    bad = 0
    for hz, Lspan in ((0.0625, 0.375), (0.08, 0.44)):
        cfg = dict(BASE, hz=hz, Lspan=Lspan, Ltotal=2 * Lspan)
        res = {}
        for chain in ("0", "1"):
            os.environ["SSF_COL_CHAIN"] = chain
            res[chain] = run(E, cfg)
        (a, ia), (b, ib) = res["0"], res["1"]
        want = paired_boundaries(hz, Lspan, 2)
        ok = (np.array_equal(a, b) and all(ia[k] == ib[k] for k in COUNTERS) and ia["steps"] == 12 and want > 0 and
              ia["col_sg_n"] - ib["col_sg_n"] == want and ia["row_n"] == ib["row_n"])
        print(f"hz {hz} Lspan {Lspan}: unchained {ia}  chained {ib}  paired boundaries {want}  bit-equal {np.array_equal(a, b)}  "
              f"{'OK' if ok else 'MISMATCH'}", flush=True)
        bad += not ok
    models.release_plans()
    return 1 if bad else 0


def default():
    E = synth_field(1 << 20, 2, 78, 8.4)
    hz, Lspan = 0.08, 0.32
    cfg = dict(BASE, hz=hz, Lspan=Lspan, Ltotal=2 * Lspan)
    out, info = run(E, cfg)
    models.release_plans()
    row_n, col_n = info.pop("row_n"), info.pop("col_sg_n")
    print("digest", hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest(), info, flush=True)
    print("col_sg_n", col_n, "row_n", row_n, "paired_boundaries", paired_boundaries(hz, Lspan, 2), flush=True)
    return 0 if info["steps"] == 8 else 1


if __name__ == "__main__":
    sys.exit({"small": small, "default": default}[sys.argv[1]]())
