#!/usr/bin/env python3
"""Time ``perturbationNLIN`` on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Cases (16-QAM, two polarisations, Pin 0 dBm; the input is a DeviceArray, the result stays on the device):
  notebook     10^5 symbols, matrixOrder 75, 'AMR' at -30 dB, prec complex64, length 1600 km, spans of 80 km:
               examples/test_perturbation_models.ipynb
  am25, am75   10^5 symbols, 'AM', matrixOrder 25 and 75, prec complex128
  n17_c128, n17_c64   2^17 symbols, 'AM', matrixOrder 25, prec complex128 and complex64

Per case: call_s, the median over the repetitions of (a host clock around `inner` device-resident whole calls, each ending in a
stream synchronise) / inner, with inner chosen per case so that a window lasts at least 0.2 s (200 to 1100 calls); terms, the
coefficient terms of the reference's sum (symbols x kept coefficients; 'AM' keeps (2L + 1)^2) and terms_per_s; fp64_share, the share of the FP64 vector ceiling as DESIGN.md 4.8 defines it: the least time the
chip's SIMDs need for the FP64 instructions of the sum alone -- four multiply-adds per term and lane, one wave-instruction
occupying its SIMD for 1.91 ns (profiles/r4_valu_rates.txt), 1024 SIMDs -- over the time of the whole call; the launch geometry.
Next to it cpu_emulator: the g++ -O2 walk of the dense main kernel (tests/emu/emu_nlin.cpp bench) on one core of the same box,
at matrixOrder 25 and 75 on 4096 symbols, as terms per second (the reference's own numba build does not run without numba).

Writes profiles/nlin_bench.json.   Usage: python tools/bench_nlin.py [--out FILE] [--quick] [--rehearse]
(--rehearse: no GPU needed; builds every case at a few hundred symbols, prepares the call and walks the emulator's bench once,
 times nothing;
 --trace CASE: that case alone, 20 calls, as the workload of `rocprofv3 --kernel-trace --stats`, whose database
 tools/rocpd_stats.py summarises: the kernel times of DESIGN.md 4.15)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib, perturbation as pt  # noqa: E402

SIMDS = 1024
FP64_NS = 1.91                      # one FP64 wave-instruction on its SIMD (profiles/r4_valu_rates.txt)
FMA_PER_TERM = 4                    # a complex multiply-add
INNER = 20
WINDOW_S = 0.2                      # a timed window lasts at least this long

CASES = {
    "notebook": dict(N=100000, param=dict(matrixOrder=75, mode="AMR", coeffTol=-30, prec="complex64", length=1600, lspan=80)),
    "am25": dict(N=100000, param=dict(matrixOrder=25, mode="AM", prec="complex128")),
    "am75": dict(N=100000, param=dict(matrixOrder=75, mode="AM", prec="complex128")),
    "n17_c128": dict(N=1 << 17, param=dict(matrixOrder=25, mode="AM", prec="complex128")),
    "n17_c64": dict(N=1 << 17, param=dict(matrixOrder=25, mode="AM", prec="complex64")),
}


class Param:
    pass


def build(c, N):
    p = Param()
    for k, v in c["param"].items():
        setattr(p, k, np.dtype(v).type if k == "prec" else v)
    rng = np.random.default_rng(1)
    lv = np.arange(-3, 4, 2)
    E = rng.choice(lv, (N, 2)) + 1j * rng.choice(lv, (N, 2))
    return p, E.astype(np.complex128)


def timed(fn, warmup, reps, inner=None):
    for _ in range(warmup):
        fn()
    if inner is None:                   # calls per window: at least INNER, and enough for WINDOW_S seconds
        t0 = time.perf_counter()
        for _ in range(INNER):
            fn()
        inner = max(INNER, int(np.ceil(WINDOW_S / ((time.perf_counter() - t0) / INNER))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts), min(ts), max(ts), inner


def emulator_rate(sizes):
    """terms per second of the dense main kernel walked by g++ -O2 on one core."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "emu_nlin")
        subprocess.check_call(["g++", "-O2", "-mfma", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"),
                               os.path.join(ROOT, "tests", "emu", "emu_nlin.cpp"), "-o", exe])
        for L, N in sizes:
            r = json.loads(subprocess.check_output([exe, "bench", str(L), str(N)]).decode())
            out[f"L{L}"] = dict(N=N, seconds=r["seconds"], terms=r["terms"], terms_per_s=r["terms"] / r["seconds"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlin_bench.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--trace", default="", help="a case's name: run it alone (under a kernel trace), time nothing")
    a = ap.parse_args()
    if a.rehearse:
        for name, c in CASES.items():
            p, E = build(c, 300)
            q = pt._prepare_nlin(E, p)
            print(f"{name}: {len(q['plan']['passes'])} passes, {len(q['plan']['coef'])} coefficients, "
                  f"{_lib.nlin_split(c['N'], len(q['plan']['passes']))} shares at N = {c['N']}")
        print(emulator_rate([(3, 512)]))
        return
    assert oa.checkGPU(), "bench_nlin.py measures on a GPU"
    if a.trace:
        p, E = build(CASES[a.trace], CASES[a.trace]["N"])
        Ed = oa.to_device(E)
        for _ in range(20):
            oa.perturbationNLIN(Ed, p)
        return
    warmup, reps = (1, 3) if a.quick else (3, 9)
    res = dict(device=_lib.load().ssf_version().decode(), window_s=WINDOW_S, reps=reps, simds=SIMDS, fp64_ns=FP64_NS, fma_per_term=FMA_PER_TERM,
               cases={})
    for name, c in CASES.items():
        p, E = build(c, c["N"])
        Ed = oa.to_device(E)
        plan = pt._prepare_nlin(Ed, p)["plan"]
        out = oa.perturbationNLIN(Ed, p)
        assert np.all(np.isfinite(out.get()))
        med, lo, hi, inner = timed(lambda: oa.perturbationNLIN(Ed, p), warmup, reps)
        terms = float(c["N"]) * plan["nReducedCoeffs"]
        floor = terms * FMA_PER_TERM / 64 * FP64_NS * 1e-9 / SIMDS
        npass = len(plan["passes"])
        res["cases"][name] = dict(N=c["N"], param=c["param"], inner=inner, call_s=med, min_s=lo, max_s=hi, kept_coefficients=plan["nReducedCoeffs"],
                                  terms=terms, terms_per_s=terms / med, fp64_floor_s=floor, fp64_share=floor / med, passes=npass,
                                  coefficients_walked=len(plan["coef"]), shares=_lib.nlin_split(c["N"], npass),
                                  workgroups=_lib.nlin_split(c["N"], npass) * ((c["N"] + _lib.NLIN_TILE - 1) // _lib.NLIN_TILE))
        print(f"{name}: {med * 1e3:.3f} ms per call ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), {terms / med:.3e} terms/s, "
              f"{floor / med:.3f} of the FP64 vector ceiling", flush=True)
    res["cpu_emulator"] = emulator_rate([(25, 4096), (75, 4096)])
    for k, v in res["cpu_emulator"].items():
        print(f"emulator {k}: {v['terms_per_s']:.3e} terms/s on one core")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
