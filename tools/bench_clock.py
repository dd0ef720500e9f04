#!/usr/bin/env python3
"""Time the sampling-clock kernels on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Element-wise passes, device-resident, at 2^20 x 2 complex128 (32 MiB in): ``clockSamplingInterp`` (output rate 1 + 105e-6 of
the input's, so as many bytes out as in), the fused interpolate -> clip -> quantise pass of ``adc`` (no filters, no jitter), the
component quantizer of ``dac``, its min/max and the clip alone, each next to ``pbs`` at the same byte count in the same run (it reads
the (N, 2) field and writes two columns: 32 MiB in, 32 MiB out).  Bytes per second are the bytes the pass must move (input once,
output once; the interpolation's second neighbour comes from the lines its neighbours read) over the call time.

Clock recovery: ``gardnerClockRecovery`` at 2^16 and 2^18 input samples per column, 2 and 64 columns, complex64 in; microseconds
per output sample of one column (the columns run side by side) and the ratio of the 64-column call to the 2-column call.  The
comparator is the g++ loop of tests/emu/emu_clock.cpp on the same machine (its loop alone, one column after the other).

Method: inputs are uploaded once, 3 warm-up calls per case, then the median of the repetitions of a host clock around calls that
each end in a stream synchronise.

Writes profiles/clock_bench.json.   Usage: python tools/bench_clock.py [--out FILE] [--quick]
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
from opticommpy_amd import _lib, clock  # noqa: E402


class Param:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return dict(median_s=statistics.median(t), min_s=min(t), max_s=max(t), reps=reps)


def elementwise(reps):
    N = 1 << 20
    rng = np.random.default_rng(1)
    x = oa.to_device((rng.uniform(-1.2, 1.2, size=(N, 2)) + 1j * rng.uniform(-1.2, 1.2, size=(N, 2))))
    inFs = 64e9
    outFs = inFs * (1 + 105e-6)
    table = clock.quant_table(8, 1, -1)
    nbytes = x.nbytes
    cases = {
        "pbs": (lambda: oa.pbs(x, 0.3), 2 * nbytes),
        "clockSamplingInterp": (lambda: oa.clockSamplingInterp(x, inFs, outFs), 2 * nbytes),
        "adc_fused_pass": (lambda: clock._interp(x, inFs, outFs, _lib.CLOCK_COMPONENTS, clip=(-1, 1), quant=table), 2 * nbytes),
        "quantize_components": (lambda: clock._quantize(x, table), 2 * nbytes),
        "minmax": (lambda: clock._minmax(x), nbytes),
    }
    out = {}
    for rnd in range(3):                              # the cases interleaved, three rounds: one run, one clock state
        for name, (fn, moved) in cases.items():
            r = timed(fn, reps)
            r["bytes"] = moved
            r["bytes_per_s"] = moved / r["median_s"]
            out.setdefault(name, []).append(r)
    res = {}
    for name, rounds in out.items():
        best = min(rounds, key=lambda r: r["median_s"])
        res[name] = dict(best, rounds_median_s=[r["median_s"] for r in rounds])
    for name in res:
        res[name]["time_over_pbs"] = res[name]["median_s"] / res["pbs"]["median_s"]
    return dict(shape=[N, 2], dtype="complex128", cases=res)


def build_emu(tmp):
    exe = os.path.join(tmp, "emu_clock")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_clock.cpp"), "-o", exe])
    return exe


def emu_loop_seconds(exe, tmp, x, q):
    p = q["params"]
    I = np.zeros(16, dtype=np.int64)
    D = np.zeros(8, dtype=np.float64)
    I[:6], D[:2] = [p.n, p.lpad, p.Ln, p.nModes, p.dtype, p.nyquist], [p.kp, p.ki]
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        f.write(I.tobytes() + D.tobytes() + np.ascontiguousarray(x).tobytes())
    txt = subprocess.check_output([exe, "gardner", os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")],
                                  env=dict(os.environ, EMU_CLOCK_TIME="1")).decode()
    return float(txt.split()[1])


def gardner(reps, sizes):
    rng = np.random.default_rng(2)
    prm = Param(kp=1e-3, ki=1e-6, isNyquist=True, lpad=1, maxPPM=500)
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_emu(tmp)
        for n in sizes:
            per = {}
            for cols in (2, 64):
                t = np.arange(n)[:, None] * (1 + 300e-6) * 0.5
                x = (np.sinc(t % 1 - 0.5) * np.exp(2j * np.pi * rng.uniform(size=(1, cols))) + 0.05 * (rng.normal(size=(n, cols)) + 1j * rng.normal(size=(n, cols)))).astype(np.complex64)
                xd = oa.to_device(x)
                r = timed(lambda: oa.gardnerClockRecovery(xd, prm), reps)
                outs = oa.gardnerClockRecovery(xd, prm).shape[0]
                r.update(n=n, cols=cols, outputs_per_column=outs, us_per_output=1e6 * r["median_s"] / outs)
                if cols == 2:
                    s = emu_loop_seconds(exe, tmp, x, clock._prepare_gardner(x, prm))
                    r["cpu_loop_s_2_columns"] = s
                    r["cpu_us_per_output"] = 1e6 * s / (2 * outs)
                per[cols] = r
                rows.append(r)
            per[64]["time_over_2_columns"] = per[64]["median_s"] / per[2]["median_s"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clock_bench.json"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert oa.checkGPU(), "bench_clock.py needs a GPU"
    res = dict(device=oa.checkGPU() and _lib.load().ssf_version().decode(), elementwise=elementwise(5 if a.quick else 30),
               gardner=gardner(3 if a.quick else 7, (1 << 12,) if a.quick else (1 << 16, 1 << 18)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
