#!/usr/bin/env python3
"""Time the link metrics on the GPU: device-resident ``metrics()`` against the four separate calls and a vectorised numpy
restatement on the same box's CPU.  Runs on the GPU box only; reads nothing but this repository.

Cases: 2^16 and 2^20 symbols x 2 modes, 16-, 64- and 256-QAM at an SNR that gives a BER of a few percent.  Method: inputs
uploaded once, 3 warm-up calls per case and shape, then the median of the repetitions of a host clock around calls that each end
in a stream synchronise (the results come back to the host).  The numpy baseline is timed once per case (it runs for seconds);
at 2^20 symbols only for M = 16.

Derived figures per case
    symbols_per_s        symbols x modes / median time of metrics()
    exps_per_s           likelihood terms (M per symbol) / median time
    fp64_ceiling_frac    the least time the FP64 vector units could take for the soft-demapping pass over the measured time of the
                         whole call.  Per likelihood term that kernel issues about 33 vector instructions, 28.5 of them FP64
                         (read off the gfx950 disassembly of k_soft's loop over a group of 16 terms, M >= 16: exp by range reduction
                         and polynomial, the sums per bit position); an FP64 vector instruction of one wave occupies its SIMD
                         for 1.91 ns (profiles/r4_valu_rates.txt, 8 waves per SIMD).  The 32-bit selects are left out: a lower bound
                         on the work, so the fraction is a lower bound on the utilisation.

Writes profiles/metrics_bench.json.   Usage: python tools/bench_metrics.py [--out FILE] [--quick]
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

SNR_DB = {16: 12, 64: 18, 256: 24}
FP64_NS_PER_WAVE_INSTR = 1.91
FP64_PER_TERM = 28.5


def make(n, M, seed):
    rng = np.random.default_rng(seed)
    const = oa.grayMapping(M, "qam").astype(np.complex128)
    const = const / np.sqrt(np.mean(np.abs(const) ** 2))
    tx = const[rng.integers(0, M, size=(n, 2))]
    noise = (rng.normal(size=(n, 2)) + 1j * rng.normal(size=(n, 2))) * np.sqrt(10 ** (-SNR_DB[M] / 10) / 2)
    return (tx + noise) * 0.7 * np.exp(0.3j), tx


def numpy_metrics(rx, tx, M, chunk=1 << 14):
    """The reference's arithmetic, vectorised over symbols (chunked so that the (chunk, M) temporaries stay in cache)."""
    const = oa.grayMapping(M, "qam")
    b = int(np.log2(M))
    px = np.ones(M) / M
    Es = np.sum(np.abs(const) ** 2 * px)
    H = np.sum(-px * np.log2(px))
    cn = const.astype(np.complex128) / np.sqrt(Es)
    bitmap = ((np.arange(M)[:, None] >> np.arange(b - 1, -1, -1)) & 1).astype(bool)
    out = {k: np.zeros(rx.shape[1]) for k in ("BER", "SER", "SNR", "GMI", "NGMI", "MI", "EVM")}
    s, t = rx / np.sqrt(np.mean(np.abs(rx) ** 2)), tx / np.sqrt(np.mean(np.abs(tx) ** 2))
    for k in range(rx.shape[1]):
        r = np.mean(tx[:, k] / rx[:, k]) * rx[:, k]
        r, x = r / np.sqrt(np.mean(np.abs(r) ** 2)), tx[:, k] / np.sqrt(np.mean(np.abs(tx[:, k]) ** 2))
        d = r - x
        sigma2 = np.var(d)
        out["SNR"][k] = 10 * np.log10(np.mean(np.abs(x) ** 2) / np.mean(np.abs(d) ** 2))
        e = np.mean(t[:, k] / s[:, k]) * s[:, k] - t[:, k]
        out["EVM"][k] = np.mean(np.abs(e) ** 2) / np.mean(np.abs(t[:, k]) ** 2)
        biterr = symerr = 0
        gsum = misum = 0.0
        for i in range(0, len(r), chunk):
            rc, xc = r[i:i + chunk], x[i:i + chunk]
            d2 = np.abs(rc[:, None] - cn[None, :]) ** 2
            irx, itx = np.argmin(d2, axis=1), np.argmin(np.abs(xc[:, None] - cn[None, :]), axis=1)
            diff = irx ^ itx
            symerr += np.count_nonzero(diff)
            biterr += sum(np.count_nonzero(diff & (1 << j)) for j in range(b))
            p = np.exp(-d2 / sigma2) * px
            for j in range(b):
                with np.errstate(divide="ignore"):
                    llr = np.log(np.sum(p[:, ~bitmap[:, j]], axis=1)) - np.log(np.sum(p[:, bitmap[:, j]], axis=1))
                llr = np.clip(llr, -500, 500)
                gsum += np.sum(np.log2(1 + np.exp((2.0 * bitmap[itx, j] - 1) * llr)))
            misum += np.sum(-(1 / sigma2) * np.abs(rc - xc) ** 2 * np.log2(np.exp(1)) + np.log2(px[itx]) - np.log2(np.sum(p, axis=1)))
        n = len(r)
        out["BER"][k], out["SER"][k] = biterr / (n * b), symerr / n
        out["GMI"][k] = H - gsum / n
        out["NGMI"][k] = out["GMI"][k] / H
        out["MI"][k] = H + misum / n
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--quick", action="store_true", help="2^16 symbols only, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_metrics.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    cus = info.compute_units
    cases = []
    for log2n in ((16,) if args.quick else (16, 20)):
        for M in (16, 64, 256):
            n = 1 << log2n
            rx, tx = make(n, M, 100 + M + log2n)
            rd, td = oa.to_device(rx), oa.to_device(tx)
            reps = 5 if args.quick else (30 if log2n == 16 else 10)
            full = lambda: oa.metrics(rd, td, M, "qam")   # noqa: E731

            def four():
                oa.fastBERcalc(rd, td, M, "qam")
                oa.monteCarloGMI(rd, td, M, "qam")
                oa.monteCarloMI(rd, td, M, "qam")
                oa.calcEVM(rd, M, "qam", symbTx=td)

            t_full, t_min, t_max = timed(full, 3, reps)
            t_four = timed(four, 3, reps)[0]
            t_host = timed(lambda: oa.metrics(rx, tx, M, "qam"), 2, max(3, reps // 3))[0]
            got = oa.metrics(rd, td, M, "qam")
            cpu_s = None
            check = None
            if log2n == 16 or M == 16:
                t0 = time.perf_counter()
                ref = numpy_metrics(rx, tx, M)
                cpu_s = time.perf_counter() - t0
                check = {k: float(np.max(np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300))) for k in ref}
            terms = 2.0 * n * M
            ideal_s = terms * FP64_PER_TERM / 64 * FP64_NS_PER_WAVE_INSTR * 1e-9 / (cus * 4)
            case = dict(log2_symbols=log2n, modes=2, M=M, snr_dB=SNR_DB[M], reps=reps,
                        metrics_s=t_full, metrics_s_min=t_min, metrics_s_max=t_max, four_calls_s=t_four, metrics_numpy_args_s=t_host,
                        cpu_numpy_s=cpu_s, speedup_over_numpy=None if cpu_s is None else cpu_s / t_full,
                        symbols_per_s=2.0 * n / t_full, exps_per_s=terms / t_full, fp64_ceiling_frac=ideal_s / t_full,
                        max_rel_diff_to_numpy=check, BER=[float(v) for v in got["BER"]], GMI=[float(v) for v in got["GMI"]])
            cases.append(case)
            print(json.dumps(case), flush=True)
    out = dict(tool="tools/bench_metrics.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=cus, numpy=np.__version__, method="3 warm-up calls, median of reps; host clock around synchronous calls",
               valu_per_term="about 33 vector instructions, 28.5 FP64 (k_soft, gfx950 disassembly, groups of 16 terms)",
               fp64_ns_per_wave_instruction=FP64_NS_PER_WAVE_INSTR, cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
