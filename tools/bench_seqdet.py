#!/usr/bin/env python3
"""Time mlse, detector and autocorr on the GPU.  Runs on the GPU box only; reads nothing but this repository.

mlse: 5e5 PAM-4 symbols, the size of the reference's IM/DD notebook, at 16, 64 and 256 states (3, 4 and 5 taps), and 1e5 PAM-2
symbols at 1024 states (11 taps); one column and eight columns.  What is timed is the whole device-resident call -- host checks,
the upload of the tables, the four launches, the download of the final metrics and the one synchronise -- with a host clock:
2 warm-up calls, then the median of 21.  A second series with seqdet._TIMING set (a switch of this tool) reads the device time
of the forward pass and of the three traceback launches from events around them.
    ns_per_step       call time / symbols of one column: the latency of one trellis step (all columns advance together)
    cpu               tests/emu/emu_seqdet.cpp built with g++ -O2 on one core of the same box, its own clock around the walk of one
                      column (forward pass and traceback), the fastest of 3, in ns per symbol step
For comparison the file repeats ffe's recorded serial latency per symbol from profiles/siso_bench.json.

detector, autocorr: on DeviceArrays of 2^20 samples, call time against the time their bytes take at the copy bandwidth measured
in the same run (ssf_device_copy_bandwidth).

Writes profiles/seqdet_bench.json.   Usage: python tools/bench_seqdet.py [--out FILE] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opticommpy_amd as oa  # noqa: E402
import seqdet_cases as sc  # noqa: E402
from opticommpy_amd import _lib, seqdet  # noqa: E402

TAPS = [1, .6, .5, .4, .3, .3, .2, .2, .1, .1, .05]
CASES = [(4, 2, 500_000), (4, 3, 500_000), (4, 4, 500_000), (2, 10, 100_000)]      # M, L, symbols


def make(M, L, n, cols, seed):
    rng = np.random.default_rng(seed)
    c, h = sc.pam_table(M), np.array(TAPS[:L + 1])
    tx = rng.integers(0, M, size=(n, cols))
    y = np.stack([np.convolve(c[tx[:, k]], h)[:n] for k in range(cols)], axis=1) + 0.2 * rng.normal(size=(n, cols))
    return (y[:, 0].copy() if cols == 1 else y), h, c, tx


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * statistics.median(ts), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqdet_bench.json"))
    ap.add_argument("--quick", action="store_true", help="a tenth of the symbols, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_seqdet.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="bench_seqdet_"))
    exe = sc.build_emu(tmp / "emu_seqdet")
    reps = 5 if args.quick else 21
    cases = []
    for M, L, n in CASES:
        n = n // 10 if args.quick else n
        for cols in (1, 8):
            y, h, c, tx = make(M, L, n, cols, 31 + L)
            yd = oa.to_device(y)
            case = dict(M=M, taps=L + 1, states=M ** L, symbols=n, columns=cols, reps=reps)
            case["call"] = timed(lambda: oa.mlse(yd, h, c), 2, reps)
            case.update(kernel=seqdet.last_call["kernel"], survivor_bytes=seqdet.last_call["survivor_bytes"],
                        ns_per_step=1e6 * case["call"]["median_ms"] / n, ns_per_symbol=1e6 * case["call"]["median_ms"] / (n * cols))
            fwd, tb = [], []
            seqdet._TIMING = True
            try:
                for r in range(2 + reps):
                    out = oa.mlse(yd, h, c)
                    if r >= 2:
                        fwd.append(seqdet.last_call["fwd_ms"])
                        tb.append(seqdet.last_call["tb_ms"])
            finally:
                seqdet._TIMING = False
            case.update(forward_ms=statistics.median(fwd), traceback_ms=statistics.median(tb),
                        traceback_over_forward=statistics.median(tb) / statistics.median(fwd))
            got = out.get()
            case["symbol_error_rate"] = float(np.mean(got != c[tx[:, 0] if cols == 1 else tx]))
            if cols == 1:
                e_out, _, e_info = sc.emu_mlse(exe, tmp, y, h, c, reps=3)
                case.update(cpu_s=e_info["seconds"], cpu_ns_per_step=1e9 * e_info["seconds"] / n, cpu_equals_gpu=bool(np.array_equal(e_out, got)),
                            cpu_over_gpu=1e3 * e_info["seconds"] / case["call"]["median_ms"])
            cases.append(case)
            print(json.dumps(case), flush=True)

    n20 = 1 << 20
    bw = C.c_double(0.0)
    assert lib.ssf_device_copy_bandwidth(0, 16 * n20, 50, C.byref(bw)) == 0
    rng = np.random.default_rng(5)
    c16 = sc.qam_table(16)
    r = oa.to_device(c16[rng.integers(0, 16, size=n20)] + 0.2 * (rng.normal(size=n20) + 1j * rng.normal(size=n20)))
    x = oa.to_device(sc.coloured(n20, 9))
    px = np.full(16, 1 / 16)
    small = {
        "detector_ml_16qam": (lambda: oa.detector(r, 0.08, c16, rule="ML"), n20 * (16 + 16 + 8)),
        "detector_map_16qam": (lambda: oa.detector(r, 0.08, c16, px=px, rule="MAP"), n20 * (16 + 16 + 8)),
        "autocorr_16": (lambda: oa.autocorr(x, 16), n20 * 8),
        "autocorr_256": (lambda: oa.autocorr(x, 256), n20 * 8),
    }
    ew = {}
    for name, (fn, nbytes) in small.items():
        rec = dict(samples=n20, bytes=nbytes, device=timed(fn, 2, reps))
        rec["bytes_at_copy_bandwidth_us"] = nbytes / (bw.value * 1e9) * 1e6
        rec["call_over_bytes_at_copy_bandwidth"] = rec["device"]["median_ms"] * 1e3 / rec["bytes_at_copy_bandwidth_us"]
        ew[name] = rec
        print(name, json.dumps(rec), flush=True)
    ffe = None
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "siso_bench.json")))
        ffe = dict(source="profiles/siso_bench.json", serial_us_per_symbol=next(k["serial_us_per_symbol"] for k in rec["cases"] if k["kind"] == "ffe"))
    except (OSError, KeyError, ValueError, StopIteration):
        pass
    out = dict(tool="tools/bench_seqdet.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=info.compute_units, numpy=np.__version__, quick=bool(args.quick),
               method="2 warm-up calls, median of reps; host clock around synchronous device-resident calls (whole calls); forward_ms and "
                      "traceback_ms from device events in a second series; cpu_s: tests/emu/emu_seqdet.cpp built with g++ -O2, one core, one "
                      "column, its own clock around forward pass and traceback, the fastest of 3",
               measured_copy_GBs=bw.value, ffe=ffe, mlse=cases, elementwise=ew)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
