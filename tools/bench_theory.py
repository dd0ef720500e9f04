#!/usr/bin/env python3
"""Time theoryMI and calcMI on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Cases: theoryMI for 16-, 64-, 256- and 1024-QAM at one SNR and over the SNR grid of examples/test_metrics.ipynb (np.arange(-2, 35),
37 points, one library call); calcMI of 16-QAM at 2^16 and 2^20 symbols held on the device.  Method: one warm-up call, then the
median of 21 whole calls by a host clock (each call ends in a stream synchronise and brings its results to the host); the
1024-QAM grid, seconds per call, is repeated 5 times.

exps_per_s is M^2 x 17161 nodes x SNRs (theoryMI) or M x symbols (calcMI) over the median time: the figure to hold against
metrics()'s likelihood terms per second (profiles/metrics_bench.json), the comparable kernel.

The reference's theoryMI, run without a JIT on one CPU core when the fixtures were made (tools/gen_golden_theory.py, the `seconds`
of tests/golden/theory/*.npz), is quoted next to it.

Writes profiles/theory_bench.json.   Usage: python tools/bench_theory.py [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib  # noqa: E402

NODES = 131 * 131
GRID = np.arange(-2, 35, 1)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def reference_seconds():
    out = {}
    golden = os.path.join(ROOT, "tests", "golden", "theory")
    for name in ("qpsk_5dB", "qam16_10dB", "qam64_15dB"):
        z = np.load(os.path.join(golden, f"{name}.npz"))
        cfg = json.loads(str(z["cfg"]))
        out[name] = dict(symmetry=cfg["symmetry"], tol=cfg["tol"], seconds=[float(s) for s in z["seconds"]],
                         order="per symmetry flag: default tol" + (", then the accurate tol" if cfg["tol"] is not None else ""))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "theory_bench.json"))
    ap.add_argument("--quick", action="store_true", help="16- and 64-QAM only, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_theory.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    cases = []
    for M in ((16, 64) if args.quick else (16, 64, 256, 1024)):
        for snr, label in ((15.0, "one SNR"), (GRID, "notebook grid, 37 SNRs")):
            nS = int(np.size(snr))
            reps = 3 if args.quick else (5 if (M == 1024 and nS > 1) else 21)
            t, t_min, t_max = timed(lambda: oa.theoryMI(M, "qam", snr), reps)
            exps = float(M) * M * NODES * nS
            case = dict(call="theoryMI", M=M, snr=label, reps=reps, seconds=t, seconds_min=t_min, seconds_max=t_max, exps=exps, exps_per_s=exps / t)
            cases.append(case)
            print(json.dumps(case), flush=True)
    rng = np.random.default_rng(3)
    const = oa.grayMapping(16, "qam").astype(np.complex128) / np.sqrt(10.0)
    px = np.ones(16) / 16
    for log2n in ((16,) if args.quick else (16, 20)):
        n = 1 << log2n
        tx = const[rng.integers(0, 16, size=n)]
        rx = tx + 0.18 * (rng.normal(size=n) + 1j * rng.normal(size=n))
        rd, td = oa.to_device(rx), oa.to_device(tx)
        reps = 3 if args.quick else 21
        t, t_min, t_max = timed(lambda: oa.calcMI(rd, td, 0.0648, const, px), reps)
        case = dict(call="calcMI", M=16, log2_symbols=log2n, reps=reps, seconds=t, seconds_min=t_min, seconds_max=t_max, exps=16.0 * n,
                    exps_per_s=16.0 * n / t, symbols_per_s=n / t)
        cases.append(case)
        print(json.dumps(case), flush=True)
    arch = info.arch.decode(errors="replace")
    out = dict(tool="tools/bench_theory.py", device=info.name.decode(errors="replace") or arch, arch=arch,    # (a card may report no name)
               compute_units=info.compute_units, numpy=np.__version__,
               method="one warm-up call, median of reps; host clock around whole calls that end in a stream synchronise",
               reference_cpu_no_jit=reference_seconds(), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
