#!/usr/bin/env python3
"""Time syncDataSequences, movingAverage and bert on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Sizes are the IM/DD notebook's: 5e5 PAM-4 symbols with the received signal at 2 samples per symbol (1e6 samples), in both reference
modes; movingAverage at 5e5 samples with N = 500; bert at 1e6 samples.  Everything is timed on DeviceArrays: 2 warm-up calls, then the
median of `reps` whole calls with a host clock (every call ends in a device synchronise).

    host_ms      the same steps in numpy / scipy double precision on one core of the same box (FFT correlations and convolutions:
                 the extended-precision restatement of tests/syncdata_restatement.py correlates directly, O(n^2), and cannot run at
                 this size; movingAverage and bert ARE the restatement's functions).  Its result is compared with the device's.
    --trace W    runs only workload W ('symbols', 'signal', 'small') a few times, for `rocprofv3 --kernel-trace` in a run of its own
    --kernel-trace DIR [DIR ...]   reads the kernel_trace.csv files of such runs: per-kernel totals (profiles/syncdata_kt_*.txt), the
                 share of a syncDataSequences call spent in the kernels this engine adds (k_tile, k_ext_*, k_real_part) against
                 everything else (symbolSync's transforms and gathers, firFilter, resample, decimate, pnorm, detector), and the achieved
                 bytes per second of the extraction and windowed-mean kernels from the bytes their algorithms need

Writes profiles/syncdata_bench.json.   Usage: python tools/bench_syncdata.py [--out FILE] [--quick]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opticommpy_amd as oa  # noqa: E402
import syncdata_restatement as rs  # noqa: E402
from opticommpy_amd import _lib, synchronization  # noqa: E402

HBM_GBS = 8000.0           # the HBM rate DESIGN.md §4 divides by (MI355X: 8 TB/s)
NEW_KERNELS = ("k_tile", "k_ext_count", "k_ext_offsets", "k_ext_scatter", "k_real_part", "k_moving_average", "k_bert_")


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * statistics.median(ts), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts))


def make_pair(nsym, SpS, reference, seed=3, delay=12345):
    """PAM-4 symbols, their NRZ-like waveform at SpS samples per symbol, and a delayed, twice-repeated-then-cut noisy copy."""
    rng = np.random.default_rng(seed)
    table = np.array([-3.0, -1.0, 1.0, 3.0]) / np.sqrt(5)
    sym = table[rng.integers(0, 4, size=nsym)]
    wave = np.repeat(sym, SpS)
    wave = 0.25 * np.roll(wave, 1) + 0.5 * wave + 0.25 * np.roll(wave, -1)
    rx = np.roll(wave, delay) + 0.02 * rng.normal(size=len(wave))
    return rx, (sym if reference == "symbols" else wave)


def host_sync(rx, tx, p):
    """syncDataSequences' steps in numpy / scipy double precision, one mode, syncMode 'amp'."""
    from scipy.signal import correlate, fftconvolve
    SpS, reference = p.SpS, p.reference
    tiled, padL = rs.tile(tx, len(rx), SpS if reference == "symbols" else 1)
    tiled = tiled[:, 0]
    rxp = np.concatenate((rx, np.zeros(padL)))
    a, b = np.abs(tiled) - np.mean(np.abs(tiled)), np.abs(rxp) - np.mean(np.abs(rxp))
    for _ in range(2):                                                  # the correlation matrix, then finddelay
        c = np.abs(correlate(a, b, method="fft"))
    delay = int(np.argmax(c)) - len(a) + 1
    aligned = np.roll(tiled, -delay)[:len(rx)]
    if reference == "symbols":
        s = aligned[aligned != 0]
        symb = np.zeros(len(rx) // SpS + 1)
        symb[:len(s)] = s / np.sqrt(np.mean(s * s))
        pulse = oa.pulseShape(types.SimpleNamespace(pulseType="rrc", SpS=SpS, rollOff=0.01, nFilterTaps=1024))
        w = fftconvolve(aligned, pulse, mode="same")
        return w / np.sqrt(np.mean(w * w)), symb.reshape(-1, 1), delay
    import clock_restatement as crs
    x = crs.clock_interp(aligned.reshape(-1, 1), SpS, 41)[:, 0]
    x = fftconvolve(x, oa.lowPassFIR(SpS / 2, 41, 501, typeF="rect"), mode="same")
    n = len(x) // 41
    ph = int(np.argmax(np.var(x[:n * 41].reshape(-1, 41), axis=0)))
    s = np.roll(x[:n * 41], -ph)[::41]
    s = s / np.sqrt(np.mean(s * s))
    const = oa.grayMapping(4, "pam")
    table = (const / np.sqrt(np.mean(const * np.conj(const)).real)).astype(np.float64)
    d = table[np.argmin(np.abs(s[:, None] - table[None, :]), axis=1)]
    return aligned, (d / np.sqrt(np.mean(d * d))).reshape(-1, 1), delay


def workloads(quick):
    nsym = 50_000 if quick else 500_000
    w = {}
    for reference in ("symbols", "signal"):
        rx, tx = make_pair(nsym, 2, reference)
        p = types.SimpleNamespace(SpS=2, reference=reference, syncMode="amp", M=4, constType="pam")
        w[reference] = (rx, tx, p)
    rng = np.random.default_rng(9)
    w["ma"] = (np.abs(rng.normal(size=nsym)) + 0.1, 500)
    bits = rng.integers(0, 2, size=2 * nsym)
    w["bert"] = (np.where(bits == 1, 1.0, 0.1) + rng.normal(size=2 * nsym) * np.where(bits == 1, 0.2, 0.1), bits.astype(np.uint8))
    return w


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def run_trace(what, w, calls=5):
    if what in ("symbols", "signal"):
        rx, tx, p = w[what]
        rxd, txd = oa.to_device(rx), oa.to_device(tx)
        for _ in range(calls + 1):
            oa.syncDataSequences(rxd, txd, p)
    else:
        xd, bd, id_ = oa.to_device(w["ma"][0]), oa.to_device(w["bert"][1]), oa.to_device(w["bert"][0])
        for _ in range(calls + 1):
            oa.movingAverage(xd, w["ma"][1])
            oa.bert(id_, bd)
    print(f"trace workload {what}: {calls + 1} calls")


def read_traces(dirs, rec, nsym):
    """Per-kernel totals of every trace directory (named <anything>_<workload>) into rec["kernel_trace"] and text tables."""
    rec["kernel_trace"] = {}
    for d in dirs:
        what = os.path.basename(os.path.normpath(d)).rsplit("_", 1)[-1]
        rows = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
                rows.setdefault(r["Kernel_Name"], []).append(t)
        if not rows:
            raise SystemExit(f"{d}: no kernel_trace.csv with rows")
        total = sum(sum(v) for v in rows.values())
        new = sum(sum(v) for k, v in rows.items() if any(n in k for n in NEW_KERNELS))
        table = sorted(rows.items(), key=lambda kv: -sum(kv[1]))
        lines = [f"{'kernel':<110} {'calls':>6} {'total_ms':>9} {'avg_us':>9} {'min_us':>8} {'max_us':>8} {'%':>6}"]
        for k, v in table:
            lines.append(f"{k[:110]:<110} {len(v):>6} {sum(v) / 1e3:>9.3f} {statistics.mean(v):>9.2f} {min(v):>8.2f} {max(v):>8.2f} {100 * sum(v) / total:>6.2f}")
        with open(os.path.join(ROOT, "profiles", f"syncdata_kt_{what}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        entry = dict(kernel_us_total=total, new_kernels_us=new, new_kernels_share=new / total, existing_share=1 - new / total,
                     kernels={k: dict(calls=len(v), median_us=statistics.median(v)) for k, v in table if any(n in k for n in NEW_KERNELS)})
        # bytes the algorithms need: the extraction reads the aligned sequence twice (count, scatter: 16 B a sample) and writes the kept
        # symbols (8 B, real output); the windowed mean reads and writes 8 B a sample
        n_rx = 2 * nsym
        need = {"k_ext_count": 16 * n_rx, "k_ext_scatter": 16 * n_rx + 8 * nsym, "k_moving_average": 16 * nsym}
        for k, v in entry["kernels"].items():
            for name, nbytes in need.items():
                if name in k:
                    v.update(bytes=nbytes, GBs=nbytes / (v["median_us"] * 1e-6) / 1e9, of_hbm_rate=nbytes / (v["median_us"] * 1e-6) / 1e9 / HBM_GBS)
        rec["kernel_trace"][what] = entry
        print(what, json.dumps(entry), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syncdata_bench.json"))
    ap.add_argument("--quick", action="store_true", help="a tenth of the samples, few repetitions (rehearsal)")
    ap.add_argument("--trace", choices=("symbols", "signal", "small"))
    ap.add_argument("--kernel-trace", nargs="+", default=[])
    args = ap.parse_args()
    w = workloads(args.quick)
    nsym = len(w["ma"][0])
    if args.kernel_trace:
        rec = json.load(open(args.out))
        read_traces(args.kernel_trace, rec, nsym)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        return
    if not oa.checkGPU():
        raise SystemExit("bench_syncdata.py needs a GPU: nothing is measured without one")
    if args.trace:
        return run_trace(args.trace, w)
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    reps = 3 if args.quick else 11
    rec = dict(tool="tools/bench_syncdata.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               numpy=np.__version__, quick=bool(args.quick), symbols=nsym, hbm_GBs=HBM_GBS,
               method="2 warm-up calls, median of reps; host clock around synchronous device-resident calls (whole calls); host_ms: one "
                      "run of the same steps in numpy / scipy double precision on one core of the same box")
    for reference in ("symbols", "signal"):
        rx, tx, p = w[reference]
        rxd, txd = oa.to_device(rx), oa.to_device(tx)
        case = dict(rx_samples=len(rx), tx_rows=len(tx), SpS=2, reps=reps, device=timed(lambda: oa.syncDataSequences(rxd, txd, p), 2, reps))
        tx_, symb = oa.syncDataSequences(rxd, txd, p)
        t0 = time.perf_counter()
        h_tx, h_symb, h_delay = host_sync(rx, tx, p)
        case["host_ms"] = 1e3 * (time.perf_counter() - t0)
        case.update(host_over_device=case["host_ms"] / case["device"]["median_ms"], delay=int(synchronization.last_call["info"].delay[0]),
                    host_delay=h_delay, tx_vs_host=rel(tx_.get(), h_tx), symb_vs_host=rel(symb.get(), h_symb))
        rec[f"syncDataSequences_{reference}"] = case
        print(reference, json.dumps(case), flush=True)
    x, N = w["ma"]
    xd = oa.to_device(x)
    case = dict(samples=len(x), N=N, reps=reps, device=timed(lambda: oa.movingAverage(xd, N), 2, reps))
    t0 = time.perf_counter()
    want = rs.moving_average(x, N)
    case["host_ms"] = 1e3 * (time.perf_counter() - t0)
    case.update(host_over_device=case["host_ms"] / case["device"]["median_ms"], vs_host=rel(oa.movingAverage(xd, N).get(), want))
    rec["movingAverage"] = case
    print("movingAverage", json.dumps(case), flush=True)
    Irx, bits = w["bert"]
    Id, bd = oa.to_device(Irx), oa.to_device(bits)
    case = dict(samples=len(Irx), reps=reps, device=timed(lambda: oa.bert(Id, bd), 2, reps))
    t0 = time.perf_counter()
    ber, q, s = rs.bert(Irx, bits)
    case["host_ms"] = 1e3 * (time.perf_counter() - t0)
    got = oa.bert(Id, bd)
    case.update(host_over_device=case["host_ms"] / case["device"]["median_ms"], errors_equal=bool(round(got[0] * len(Irx)) == s.errors),
                Q_vs_host=abs(got[1] - q) / abs(q))
    rec["bert"] = case
    print("bert", json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
