#!/usr/bin/env python3
"""Time the array layer of DeviceArray on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Whole calls on DeviceArrays (allocation from the pool, launch, the engine's synchronise) at (2^20, 2) complex128 and at 2^16 rows:
2 warm-up calls, then the median of 21 with a host clock.  Per operation:

    bytes          what the operation has to read and write
    gbs            bytes / median time
    of_copy        gbs over the copy bandwidth `ssf_device_copy_bandwidth` measures IN THE SAME RUN (16 MiB in, 16 MiB out per launch)
    host_ms        the host route on the same box: .get(), the numpy operation, to_device (what a notebook had to do before)

Writes profiles/array_bench.json.   Usage: python tools/bench_array.py [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib  # noqa: E402

REPS, WARMUP = 21, 2


def timed(fn):
    for _ in range(WARMUP):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * statistics.median(ts), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts))


def operations(n):
    """name -> (device call, numpy call, bytes moved) on x (n, 2) complex128, y alike, sq (1024, 1024) complex128."""
    ind = np.arange(0, n, 3)
    e = 16
    ops = {
        "slice_contiguous": (lambda x, y, s: x[1000:-1000], lambda x, y, s: x[1000:-1000].copy(), 2 * (n - 2000) * 2 * e),
        "slice_step2": (lambda x, y, s: x[::2], lambda x, y, s: x[::2].copy(), 2 * (n // 2) * 2 * e),
        "column_select": (lambda x, y, s: x[:, 1], lambda x, y, s: x[:, 1].copy(), 2 * n * e),
        "take": (lambda x, y, s: x[ind], lambda x, y, s: x[ind], 2 * len(ind) * 2 * e),
        "transpose_n_by_2": (lambda x, y, s: x.T, lambda x, y, s: np.ascontiguousarray(x.T), 2 * n * 2 * e),
        "transpose_1024_sq": (lambda x, y, s: s.T, lambda x, y, s: np.ascontiguousarray(s.T), 2 * 1024 * 1024 * e),
        "add": (lambda x, y, s: x + y, lambda x, y, s: x + y, 3 * n * 2 * e),
        "complex_multiply": (lambda x, y, s: x * y, lambda x, y, s: x * y, 3 * n * 2 * e),
        "scalar_scale": (lambda x, y, s: 0.5 * x, lambda x, y, s: 0.5 * x, 2 * n * 2 * e),
        "abs2": (lambda x, y, s: x.abs2() if isinstance(x, oa.DeviceArray) else np.abs(x) ** 2, None, n * 2 * (e + 8)),
        "astype_c64": (lambda x, y, s: x.astype(np.complex64), lambda x, y, s: x.astype(np.complex64), n * 2 * (e + 8)),
        "sum": (lambda x, y, s: x.sum(), lambda x, y, s: x.sum(), n * 2 * e),
        "std": (lambda x, y, s: x.std(), lambda x, y, s: x.std(), 2 * n * 2 * e),
        "argmax": (lambda x, y, s: (x.real.argmax() if isinstance(x, oa.DeviceArray) else x.real.argmax()), None, n * 2 * e + 2 * n * 2 * 8),
        "freqShift": (lambda x, y, s: oa.freqShift(x, 1e9, 64e9) if isinstance(x, oa.DeviceArray) else x * np.exp(2j * np.pi * 1e9 * np.arange(len(x)) / 64e9)[:, None],
                      None, 2 * n * 2 * e),
    }
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "array_bench.json"))
    a = ap.parse_args()
    assert oa.checkGPU(), "bench_array.py needs a GPU"
    lib = _lib.load()
    bw = C.c_double()
    assert lib.ssf_device_copy_bandwidth(0, 16 << 20, 50, C.byref(bw)) == 0
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, C.byref(info))
    res = dict(device=info.name.decode(), arch=info.arch.decode(), copy_bandwidth_gbs=bw.value, reps=REPS, warmup=WARMUP, numpy=np.__version__, sizes={})
    rng = np.random.default_rng(0)
    sq = rng.standard_normal((1024, 1024)) + 1j * rng.standard_normal((1024, 1024))
    sqd = oa.to_device(sq)
    for n in (1 << 20, 1 << 16):
        x = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
        y = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
        xd, yd = oa.to_device(x), oa.to_device(y)
        rows = {}
        for name, (dev_fn, host_fn, nbytes) in operations(n).items():
            host_fn = host_fn or dev_fn
            t = timed(lambda: dev_fn(xd, yd, sqd))

            def host_route():
                if name == "transpose_1024_sq":
                    r = host_fn(x, y, sqd.get())
                else:
                    r = host_fn(xd.get(), yd.get() if name in ("add", "complex_multiply") else y, sq)
                return oa.to_device(r) if isinstance(r, np.ndarray) and r.ndim else r
            h = timed(host_route)
            gbs = nbytes / (t["median_ms"] * 1e-3) / 1e9
            rows[name] = dict(t, bytes=nbytes, gbs=gbs, of_copy=gbs / bw.value, host_ms=h["median_ms"], speedup=h["median_ms"] / t["median_ms"])
            print(f"n = {n:8d}  {name:20s} {t['median_ms']:8.3f} ms  {gbs:8.1f} GB/s  {100 * gbs / bw.value:5.1f} % of copy   host route {h['median_ms']:8.3f} ms")
        res["sizes"][str(n)] = rows
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("copy bandwidth", bw.value, "GB/s ->", a.out)


if __name__ == "__main__":
    main()
