#!/usr/bin/env python3
"""Time ffe, dfe and volterra on the GPU at the settings of the reference's IM/DD notebook
(examples/test_equalizers_for_IMDD_transmission.ipynb): 5e5 PAM-4 symbols at 2 samples per symbol, nTrain = 1e5, ffe with 70 taps,
dfe with 70 + 15, volterra with 70 / 20 / 10 at order 3, in both training modes.  Runs on the GPU box only; reads nothing but this
repository.

What is timed is the whole device-resident call -- argument checks and tables on the host, the scale reductions, the kernels, the
upload and download of the coefficients and the synchronise -- with a host clock around calls that each end in a stream
synchronise: 2 warm-up calls per case, then the median of the repetitions.

Per equalizer:
    fulltime          every symbol through the serial kernel: call time / N is the latency per serially processed symbol
    data-aided        the serial kernel up to nTrain, the frozen kernel behind it (dfe: the serial kernel throughout)
    serial-only       the data-aided call with the frozen kernel switched off (sisoeq._FROZEN, a switch of this tool): the ratio
                      serial-only / data-aided is what the frozen kernel buys at this size
    all-frozen        nTrain = 0: the whole signal through the frozen kernel, which gives its symbols per second (call overhead
                      and the scale reductions included)
    cpu               tests/emu/emu_siso.cpp built with g++ -O2 on one core of the same box, its own clock around the walk (the same
                      per-symbol bodies looped over 64 emulated lanes), for the data-aided case
For comparison the file repeats mimoAdaptEqualizer's recorded latency per symbol update from profiles/eq_bench.json.

Writes profiles/siso_bench.json.   Usage: python tools/bench_siso.py [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import pathlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import opticommpy_amd as oa  # noqa: E402
import siso_cases as sc  # noqa: E402
from opticommpy_amd import _lib, sisoeq  # noqa: E402

SPS, M = 2, 4
SETTINGS = {
    "ffe": dict(nTaps=70, mu=2e-3),
    "dfe": dict(nTapsFF=70, nTapsFB=15, mu=2e-3),
    "volterra": dict(n1Taps=70, n2Taps=20, n3Taps=10, order=3, mu=3e-2),
}


def make(nsym, seed):
    """Noisy PAM-4 at 2 samples per symbol through a short channel with a small square-law term, DC removed."""
    rng = np.random.default_rng(seed)
    table = sc.pam_table(M)
    tx = table[rng.integers(0, M, size=nsym)]
    x = np.convolve(np.repeat(tx, SPS), [0.2, 0.6, 0.2], mode="same")
    x = x + 0.25 * np.roll(x, SPS) - 0.08 * np.roll(x, -SPS)
    x = x + 0.08 * x ** 2
    x = (x - np.mean(x)) * 0.7
    return x + rng.normal(size=x.shape) * np.sqrt(np.mean(x ** 2) * 10 ** (-2.6)), tx


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def symbol_errors(y, tx, tail):
    table = sc.pam_table(M)
    dec = np.argmin(np.abs(y[-tail:, None] - table[None, :]), axis=1)
    sent = np.argmin(np.abs(tx[len(y) - tail:len(y), None] - table[None, :]), axis=1)
    return float(np.mean(dec != sent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "siso_bench.json"))
    ap.add_argument("--quick", action="store_true", help="5e4 symbols, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_siso.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    tmp = pathlib.Path(tempfile.mkdtemp(prefix="bench_siso_"))
    exe = sc.build_emu(tmp / "emu_siso")
    nsym, nTrain = (50_000, 10_000) if args.quick else (500_000, 100_000)
    reps = 3 if args.quick else 5
    x, tx = make(nsym, 77)
    xd, txd = oa.to_device(x), oa.to_device(tx)
    cases = []
    for kind, setting in SETTINGS.items():
        def prm(mode, train=nTrain):
            return sc.Param(SpS=SPS, M=M, constType="pam", nTrain=train, trainingMode=mode, prec=np.float64, **setting)

        def run(p):
            return sc.call(oa, kind, xd, txd, p)

        case = dict(kind=kind, symbols=nsym, nTrain=nTrain, SpS=SPS, M=M, settings=setting, reps=reps,
                    coefficients=sisoeq._prepare(kind, x, tx, prm("data-aided"))["ncoef"])
        t, tmin, tmax = timed(lambda: run(prm("fulltime")), 2, reps)
        case.update(fulltime_call_s=t, fulltime_min_s=tmin, fulltime_max_s=tmax, serial_us_per_symbol=1e6 * t / nsym, R=sisoeq.last_call["R"])
        assert sisoeq.last_call["serial_symbols"] == nsym and sisoeq.last_call["parallel_symbols"] == 0
        # data-aided with and without the frozen kernel, alternating
        da, so = [], []
        for r in range(2 + reps):
            for frozen, ts in ((True, da), (False, so)):
                sisoeq._FROZEN = frozen
                try:
                    t0 = time.perf_counter()
                    out = run(prm("data-aided"))
                    dt = time.perf_counter() - t0
                finally:
                    sisoeq._FROZEN = True
                if frozen:
                    split = (sisoeq.last_call["serial_symbols"], sisoeq.last_call["parallel_symbols"])
                    y = out[0].get()
                else:
                    assert sisoeq.last_call["parallel_symbols"] == 0
                    y_serial = out[0].get()
                if r >= 2:
                    ts.append(dt)
        case.update(data_aided_call_s=statistics.median(da), data_aided_min_s=min(da), data_aided_max_s=max(da),
                    serial_only_call_s=statistics.median(so), serial_only_min_s=min(so), serial_only_max_s=max(so),
                    serial_only_over_data_aided=statistics.median(so) / statistics.median(da), serial_symbols=split[0], parallel_symbols=split[1],
                    frozen_vs_serial_rel_l2=sc.rel_l2(y, y_serial), ser_last_20000=symbol_errors(y, tx, 20_000))
        if kind != "dfe":
            t0, t0min, t0max = timed(lambda: run(prm("data-aided", 0)), 2, reps)
            assert sisoeq.last_call["parallel_symbols"] == nsym
            case.update(all_frozen_call_s=t0, all_frozen_min_s=t0min, all_frozen_max_s=t0max, frozen_symbols_per_s=nsym / t0)
        emu = sc.run_emu(exe, tmp, kind, x, tx, prm("data-aided"))
        walked = emu[3]["serial_symbols"] + emu[3]["parallel_symbols"]
        case.update(cpu_emu_s=emu[3]["seconds"], cpu_us_per_symbol=1e6 * emu[3]["seconds"] / walked, cpu_over_gpu=emu[3]["seconds"] / case["data_aided_call_s"],
                    cpu_vs_gpu_rel_l2=sc.rel_l2(y, emu[0]))
        cases.append(case)
        print(json.dumps(case), flush=True)
    eq = None
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "eq_bench.json")))
        us = [c["us_per_symbol"] for c in rec["cases"]]
        eq = dict(source="profiles/eq_bench.json", us_per_symbol_update_min=min(us), us_per_symbol_update_max=max(us))
    except (OSError, KeyError, ValueError):
        pass
    out = dict(tool="tools/bench_siso.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=info.compute_units, numpy=np.__version__, quick=bool(args.quick),
               method="2 warm-up calls, median of reps; host clock around synchronous device-resident calls (whole calls: host checks, scale "
                      "reductions, kernels, coefficient upload and download); data-aided and serial-only calls alternate; cpu_emu_s: "
                      "tests/emu/emu_siso.cpp built with g++ -O2, one core, its own clock around the walk",
               mimoAdaptEqualizer=eq, cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
