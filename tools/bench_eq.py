#!/usr/bin/env python3
"""Time the adaptive MIMO equalizer on the GPU: the device-resident ``mimoAdaptEqualizer`` call at 2^16 and 2^20 input samples
with the settings of the reference's notebooks (2 modes, 15 taps, 2 samples per symbol, numIter = 5, 30 % training and 70 %
tracking) for ['nlms', 'dd-lms'] and ['da-rde', 'rde'] at 16- and 64-QAM, and the static kernel alone over the same signal.
Runs on the GPU box only; reads nothing but this repository.

The serial kernel's figure of merit is its latency per symbol -- a reduction, a decision and an update on one wavefront per output
mode -- so the time of a call is divided by the symbol updates it makes, numIter L[0] + L[1].  The comparator is the same box's
CPU: tests/emu/emu_eq.cpp (g++ -O2, the same per-symbol bodies looped over 64 emulated lanes; its own clock around the loops,
file transfer left out), run once per case at 2^16 samples and once at 2^20.  The reference's numba build does not run without
numba.  There is no ratio to meet: what the device path buys is residency, not throughput.

Method: the input is uploaded once, 2 warm-up calls per case, then the median of the repetitions of a host clock around calls
that each end in a stream synchronise.  Every figure is therefore the time of a whole call: the argument checks and tables on the
host, two memsets, the upload and download of H and the synchronise ride along with the kernels.  Against the serial kernel that
is nothing at either size; the static figures are mostly that overhead at 2^16 samples and close to the kernel at 2^20.

Writes profiles/eq_bench.json.   Usage: python tools/bench_eq.py [--out FILE] [--quick]
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
from opticommpy_amd import _lib  # noqa: E402
from opticommpy_amd import equalization as oeq  # noqa: E402

NUM_ITER, TAPS, SPS, MODES = 5, 15, 2, 2
SNR_DB = {16: 22, 64: 28}


class Param:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def make(n, M, seed):
    """Noisy M-QAM at 2 samples per symbol through a polarisation rotation of 0.6 rad and a 3-tap channel."""
    rng = np.random.default_rng(seed)
    table = oeq._tables(M, "qam", 0, np.complex128)[0]
    tx = table[rng.integers(0, M, size=(n // SPS, MODES))]
    x = np.repeat(tx, SPS, axis=0)
    x = x + 0.15 * np.roll(x, 1, axis=0) - 0.05j * np.roll(x, 2, axis=0)
    th = 0.6
    x = x @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T * 0.8
    x = x + (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape)) * np.sqrt(np.mean(np.abs(x) ** 2) * 10 ** (-SNR_DB[M] / 10) / 2)
    return x, tx


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def emu_seconds(exe, tmp, x, prm, tx):
    """Seconds the emulator's loops take on this box's CPU for the same arguments (the input file of tests/emu/emu_eq.cpp: the
    arguments as the package hands them to the library)."""
    q = oeq._prepare(x, prm, tx)
    p = q["params"]
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        f.write(np.array([p.n, p.total, p.nref, p.nModes, p.nTaps, p.SpS, p.dtype, p.ref_dtype, p.nStages, p.numIter, p.M, p.nRadii],
                         dtype=np.int64).tobytes())
        f.write(np.array([p.Rcma], dtype=np.float64).tobytes())
        for st in q["stages"]:
            f.write(np.array([st.L, st.alg], dtype=np.int64).tobytes())
            f.write(np.array([st.mu], dtype=np.float64).tobytes())
        for a in (q["table"], q["radii"], q["H"], q["x"]) + (() if q["ref"] is None else (q["ref"],)):
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.check_output([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
    return float(out.decode().split()[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eq_bench.json"))
    ap.add_argument("--quick", action="store_true", help="2^16 samples only, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_eq.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    tmp = tempfile.mkdtemp(prefix="bench_eq_")
    exe = os.path.join(tmp, "emu_eq")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_eq.cpp"), "-o", exe])
    cases = []
    for log2n in ((16,) if args.quick else (16, 20)):
        n = 1 << log2n
        total = oeq.total_symbols(n, TAPS, SPS)
        L = [int(round(0.3 * total)), total - int(round(0.3 * total))]
        updates = NUM_ITER * L[0] + L[1]
        for M in (16, 64):
            x, tx = make(n, M, 400 + M + log2n)
            xd, txd = oa.to_device(x), oa.to_device(tx)
            for alg, mu in ((["nlms", "dd-lms"], [5e-3, 1e-3]), (["da-rde", "rde"], [2e-3, 5e-4])):
                prm = Param(alg=alg, mu=mu, L=L, nTaps=TAPS, SpS=SPS, M=M, numIter=NUM_ITER, prec=np.complex128)
                reps = 3 if args.quick or log2n == 20 else 10
                t, tmin, tmax = timed(lambda: oa.mimoAdaptEqualizer(xd, prm, txd), 2, reps)
                st = Param(alg=["static"], mu=[0.0], L=[total], nTaps=TAPS, SpS=SPS, M=M, prec=np.complex128)
                ts, _, _ = timed(lambda: oa.mimoAdaptEqualizer(xd, st), 2, max(reps, 5))
                y = oa.mimoAdaptEqualizer(xd, prm, txd).get()
                dec = np.argmin(np.abs(y[-2000:, :, None] - oeq._tables(M, "qam", 0, np.complex128)[0][None, None, :]), axis=2)
                sent = np.argmin(np.abs(tx[total - 2000:total, :, None] - oeq._tables(M, "qam", 0, np.complex128)[0][None, None, :]), axis=2)
                case = dict(log2_samples=log2n, symbols=total, modes=MODES, nTaps=TAPS, SpS=SPS, numIter=NUM_ITER, L=L, M=M, alg=alg, reps=reps,
                            symbol_updates=updates, call_s=t, call_s_min=tmin, call_s_max=tmax, us_per_symbol=1e6 * t / updates,
                            static_call_s=ts, static_call_ns_per_symbol=1e9 * ts / total,
                            ser_last_2000=float(np.mean(dec != sent)) if alg[0] == "nlms" else None)     # (the radius rules leave the phase free)
                if log2n == 16 or (M == 16 and alg[0] == "nlms"):
                    cpu = emu_seconds(exe, tmp, x, prm, tx)
                    case.update(cpu_emu_s=cpu, cpu_us_per_symbol=1e6 * cpu / updates, cpu_over_gpu=cpu / t)
                cases.append(case)
                print(json.dumps(case), flush=True)
    out = dict(tool="tools/bench_eq.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=info.compute_units, numpy=np.__version__,
               method="2 warm-up calls, median of reps; host clock around synchronous device-resident calls; us_per_symbol = call time / "
                      "(numIter L[0] + L[1]); static_call_s: the whole call of a one-stage static run, host overhead included; cpu_emu_s: tests/emu/emu_eq.cpp built with g++ -O2, its own clock around the loops",
               cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
