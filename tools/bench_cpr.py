#!/usr/bin/env python3
"""Time the carrier phase recovery on the GPU: device-resident ``cpr`` (blind phase search, with and without the 4th-power
frequency offset estimation) and ``bps`` alone, against the vectorised numpy formulation (``bpsGPU``'s, chunked) on the same box's
CPU.  Runs on the GPU box only; reads nothing but this repository.

Cases: 2^16 and 2^20 symbols x 2 modes, 16-, 64- and 256-QAM, N = 85, B = 64 -- the settings of the reference's GPU benchmark
notebook (examples/benchmarck_GPU_processing.ipynb).  Method: the input is uploaded once, 3 warm-up calls per case, then the
median of the repetitions of a host clock around calls that each end in a stream synchronise.  The numpy baseline is timed once
per case, at 2^16 symbols for M = 16 and 64 (it runs for many seconds).

Derived figures per case
    distance_evals_per_s   n x modes x B x M / median time of bps alone: the distances |x e^{j phi_b} - c_m|^2 the search stands for.
                           For square QAM the kernel finds their minimum from 2 sqrt(M) one-dimensional comparisons, so this rate may
                           exceed what M evaluations per test phase would allow.
    fp64_ceiling_frac      the least time the FP64 vector units could take for the arithmetic the search kernel issues, over the
                           measured time of bps alone.  Per symbol and test phase the kernel issues 4 FP64 instructions for the
                           rotation, 3 per level and axis (subtract, multiply, minimum) and one add -- 4 + 6 sqrt(M) + 1 --, the
                           distances of the 2 Nh halo symbols of every 256-symbol tile included, and 2 for the window sum; an FP64
                           vector instruction of one wave occupies its SIMD for 1.91 ns (profiles/r4_valu_rates.txt, 8 waves per
                           SIMD: 68.6 TFLOP/s of FMA over 256 CUs).  Address arithmetic and LDS traffic are left out: a lower bound
                           on the work, so the fraction is a lower bound on the utilisation.
    share_of_equal_phases  share of the unwrapped phases that equal numpy's bit for bit.  The decisions are the same, but numpy sums the
                           unwrap's corrections in one sequence and the kernels in blocks, so most phases differ in the last bits;
                           rel_l2_to_numpy is the figure to read.

Writes profiles/cpr_bench.json.   Usage: python tools/bench_cpr.py [--out FILE] [--quick]
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
from opticommpy_amd import cpr as ocpr  # noqa: E402

SNR_DB = {16: 20, 64: 26, 256: 32}
N, B, RS = 85, 64, 32e9
FP64_NS_PER_WAVE_INSTR = 1.91
TILE = 256


class Param:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def make(n, M, seed):
    """Noisy M-QAM with a Wiener phase walk (100 kHz linewidth at 32 GBd) and a 61.3 MHz frequency offset."""
    rng = np.random.default_rng(seed)
    table = ocpr._table(M, "qam", 0).astype(np.complex128)
    tx = table[rng.integers(0, M, size=(n, 2))]
    noise = (rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))) * np.sqrt(10 ** (-SNR_DB[M] / 10) / 2)
    walk = np.cumsum(rng.normal(size=(n, 2)) * np.sqrt(2 * np.pi * 100e3 / RS), axis=0)
    return (tx + noise) * np.exp(1j * (walk + 2 * np.pi * 61.3e6 * np.arange(n)[:, None] / RS))


def numpy_cpr(x, M, chunk=2048):
    """bpsGPU's formulation vectorised in numpy (chunked so that the (chunk, B, M) temporaries stay in cache), then the unwrap,
    the rotation and the norm of cpr."""
    table = ocpr._table(M, "qam", 0).astype(np.complex128)
    Nh = N // 2
    phases = np.arange(0, B) * (np.pi / 2) / B
    rot = np.exp(1j * phases)
    raw = np.empty(x.shape)
    for m in range(x.shape[1]):
        xp = np.concatenate((np.zeros(Nh, complex), x[:, m], np.zeros(Nh, complex)))
        dmin = np.empty((len(xp), B))
        rows = max(1, (1 << 20) // (B * M))
        for q in range(0, len(xp), rows):
            r = xp[q:q + rows, None] * rot[None, :]
            dmin[q:q + rows] = np.min(np.abs(r[:, :, None] - table[None, None, :]) ** 2, axis=2)
        c = np.concatenate((np.zeros((1, B)), np.cumsum(dmin, axis=0)))
        sums = c[2 * Nh + 1:] - c[:-(2 * Nh + 1)]
        raw[:, m] = phases[np.argmin(sums, axis=1)]
    ph = np.unwrap(4 * raw, axis=0) / 4
    y = x * np.exp(1j * ph)
    return y / np.sqrt(np.mean(y * np.conj(y)).real), ph


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cpr_bench.json"))
    ap.add_argument("--quick", action="store_true", help="2^16 symbols only, few repetitions, no numpy baseline (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_cpr.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    cus = info.compute_units
    cases = []
    for log2n in ((16,) if args.quick else (16, 20)):
        for M in (16, 64, 256):
            n = 1 << log2n
            x = make(n, M, 300 + M + log2n)
            xd = oa.to_device(x)
            table = ocpr._table(M, "qam", 0)
            reps = 5 if args.quick else (30 if log2n == 16 else 10)
            t_bps, t_bps_min, t_bps_max = timed(lambda: oa.bps(xd, N // 2, table, B), 3, reps)
            case = dict(log2_symbols=log2n, modes=2, M=M, N=N, B=B, snr_dB=SNR_DB[M], reps=reps,
                        bps_s=t_bps, bps_s_min=t_bps_min, bps_s_max=t_bps_max)
            for foe in (False, True):
                prm = Param(M=M, constType="qam", N=N, B=B, runFOE=foe, Ts=1 / RS, returnPhases=True)
                t, tmin, tmax = timed(lambda: oa.cpr(xd, prm), 3, reps)
                key = "cpr_foe" if foe else "cpr"
                case.update({f"{key}_s": t, f"{key}_s_min": tmin, f"{key}_s_max": tmax, f"{key}_symbols_per_s": 2.0 * n / t})
            case["cpr_numpy_args_s"] = timed(lambda: oa.cpr(x, Param(M=M, N=N, B=B, runFOE=False)), 2, max(3, reps // 3))[0]
            evals = 2.0 * n * B * M
            instr = 2.0 * n * B * ((4 + 6 * np.sqrt(M) + 1) * (TILE + 2 * (N // 2)) / TILE + 2)
            ideal_s = instr / 64 * FP64_NS_PER_WAVE_INSTR * 1e-9 / (cus * 4)
            case.update(distance_evals=evals, distance_evals_per_s=evals / t_bps, fp64_ceiling_frac=ideal_s / t_bps)
            if not args.quick and log2n == 16 and M in (16, 64):
                sig, ph = oa.cpr(xd, Param(M=M, constType="qam", N=N, B=B, runFOE=False, returnPhases=True))
                t0 = time.perf_counter()
                ref, ref_ph = numpy_cpr(x, M)
                cpu_s = time.perf_counter() - t0
                same = np.mean(ph.get() == ref_ph)
                case.update(cpu_numpy_s=cpu_s, speedup_over_numpy=cpu_s / case["cpr_s"], share_of_equal_phases=float(same),
                            rel_l2_to_numpy=float(np.linalg.norm(sig.get() - ref) / np.linalg.norm(ref)))
            cases.append(case)
            print(json.dumps(case), flush=True)
    out = dict(tool="tools/bench_cpr.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=cus, numpy=np.__version__, method="3 warm-up calls, median of reps; host clock around synchronous calls",
               fp64_ns_per_wave_instruction=FP64_NS_PER_WAVE_INSTR,
               fp64_instructions_per_symbol_and_phase="(4 + 6 sqrt(M) + 1) x (256 + 2 Nh) / 256 + 2", cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
