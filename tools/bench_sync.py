#!/usr/bin/env python3
"""Time the sequence synchronisation on the GPU: device-resident ``symbolSync`` ('amp' and 'real', two modes, two samples per
symbol) at 2^16 and 2^20 symbols.  Runs on the GPU box only; reads nothing but this repository.

Next to every whole-call time
    transforms_s   the call's batched transforms alone (the sequences forward, the correlations back, the second round of 'real')
                   on the engine's own buffers and plans, device events around 20 rounds (``ssf_sync_transform_time``): the
                   floor the kernels add to
    host_route_s   what a user does without the device path: ``.get()`` of the received signal, the reference's algorithm with
                   numpy and scipy.signal.correlate on the host, ``to_device`` of the aligned symbols (timed once per case, after a small call that takes scipy's set-up)
    kernels        the bytes every kernel of engine_sync.hip moves, computed from the shapes, and the time they take at the
                   8 TB/s of HBM: the least these kernels could take, not a measured kernel time

Method: inputs are uploaded once, 3 warm-up calls per case, then the median of the repetitions of a host clock around calls that
each end in a stream synchronise.

Writes profiles/sync_bench.json.   Usage: python tools/bench_sync.py [--out FILE] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib  # noqa: E402

HBM_BYTES_PER_S = 8e12
MODES, SPS = 2, 2


def make(n, seed):
    """16-QAM in two modes, swapped, shifted and turned, repeated to two samples per symbol, noise of 0.05 per quadrature."""
    rng = np.random.default_rng(seed)
    table = oa.grayMapping(16, "qam").astype(np.complex128)
    table /= np.sqrt(np.mean(np.abs(table) ** 2))
    tx = table[rng.integers(0, 16, size=(n, MODES))]
    sym = np.stack([np.roll(tx[:, 1], 1234) * np.exp(0.2j), np.roll(tx[:, 0], -77) * np.exp(1j * (np.pi / 2 + 0.15))], axis=1)
    rx = np.repeat(sym, SPS, axis=0)
    rx[1::2] *= 0.6
    rx += (rng.normal(size=rx.shape) + 1j * rng.normal(size=rx.shape)) * 0.05
    return rx, tx


def host_symbol_sync(rx, tx, SpS, mode):
    """optic/dsp/core.py:552-675 with numpy and scipy on the host (decimate: core.py:435-491)."""
    rx = rx.copy()
    delays = [int(np.argmax(np.var(rx[:, k].reshape(-1, SpS), axis=0))) for k in range(rx.shape[1])]
    rx = np.stack([np.roll(rx[:, k], -delays[k])[::SpS] for k in range(rx.shape[1])], axis=1)
    nModes = rx.shape[1]
    corr = np.zeros((nModes, nModes))
    rot = np.ones((nModes, nModes), dtype=np.complex64)
    delay = np.zeros(nModes)

    def centred(v):
        a = np.abs(v)
        return a - np.mean(a)

    def finddelay(x, y):
        return np.argmax(np.abs(signal.correlate(x, y))) - x.shape[0] + 1

    if mode == "amp":
        for n in range(nModes):
            for m in range(nModes):
                corr[m, n] = np.max(np.abs(signal.correlate(centred(tx[:, m]), centred(rx[:, n]))))
        swap = np.argmax(corr, axis=0)
        tx = tx[:, swap]
        for k in range(nModes):
            delay[k] = finddelay(centred(tx[:, k]), centred(rx[:, k]))
    else:
        for n in range(nModes):
            for m in range(nModes):
                crr = signal.correlate(np.real(tx[:, m]), np.real(rx[:, n]))
                cir = signal.correlate(np.imag(tx[:, m]), np.real(rx[:, n]))
                pr, pi = crr[np.argmax(np.abs(crr))], cir[np.argmax(np.abs(cir))]
                corr[m, n] = max(abs(pr), abs(pi))
                rot[m, n] = (1 if pr > 0 else -1) if abs(pr) > abs(pi) else (-1j if pi > 0 else 1j)
        swap = np.argmax(corr, axis=0)
        tx = tx[:, swap]
        for k in range(nModes):
            tx[:, k] = rot[k, swap[k]] * tx[:, k]
            delay[k] = finddelay(np.real(tx[:, k]), np.real(rx[:, k]))
            cii = signal.correlate(np.imag(tx[:, k]), np.imag(rx[:, k]))
            if cii[np.argmax(np.abs(cii))] < 0:
                tx[:, k] = tx[:, k].conj()
    for k in range(nModes):
        tx[:, k] = np.roll(tx[:, k], -int(delay[k]))
    return tx


def shapes(n, mode):
    """(L, sequences, first-round correlations, second-round correlations) of one call (sync_kernels.h)."""
    lags = 2 * n - 1
    L = 4
    while L < lags:
        L <<= 1
    if mode == "amp":
        return L, 2 * MODES, MODES * ((MODES + 1) // 2), 0
    return L, 3 * MODES, MODES * MODES, MODES


def kernel_bytes(n, mode):
    """Bytes each kernel of one call reads and writes, from the shapes alone (complex128 everywhere; decimate left out)."""
    L, nseq, slots, slots2 = shapes(n, mode)
    lags, c = 2 * n - 1, 16
    b = {"memset": nseq * L * c,
         "prepare": 2 * (n * MODES * c) + (nseq * n * c),
         "center": (2 * MODES * n * 2 * c) if mode == "amp" else 0,
         "product": (slots + slots2) * L * c + (slots * (3 if mode == "amp" else 2) + slots2 * 2) * L * c,
         "peaks": (slots + slots2) * lags * c,
         "gather": 2 * n * MODES * c}
    b["transforms_once"] = 2 * (nseq + slots + slots2) * L * c        # one read and one write per transform: their own floor
    return b


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def transforms_alone(lib, n, mode, rounds=20):
    L, nseq, slots, slots2 = shapes(n, mode)
    s = C.c_double()
    _lib.raise_for(lib, None, lib.ssf_sync_transform_time(0, L, nseq, slots, slots2, rounds, C.byref(s)))
    return s.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bench.json"))
    ap.add_argument("--quick", action="store_true", help="2^16 symbols only, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_sync.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    cases = []
    for log2n in ((16,) if args.quick else (16, 20)):
        n = 1 << log2n
        rx, tx = make(n, 700 + log2n)
        rxd, txd = oa.to_device(rx), oa.to_device(tx)
        reps = 5 if args.quick else (30 if log2n == 16 else 10)
        for mode in ("amp", "real"):
            t, tmin, tmax = timed(lambda: oa.symbolSync(rxd, txd, SPS, mode), 3, reps)
            out, rec = oa.symbolSync(rxd, txd, SPS, mode, return_info=True)
            host_symbol_sync(rx[:4096], tx[:2048], SPS, mode)               # (scipy's first call is set-up)
            t0 = time.perf_counter()
            ref = oa.to_device(host_symbol_sync(rxd.get(), txd.get(), SPS, mode))
            host_s = time.perf_counter() - t0
            same = bool(np.array_equal(out.get(), ref.get()))
            L, nseq, slots, slots2 = shapes(n, mode)
            case = dict(log2_symbols=log2n, modes=MODES, SpS=SPS, mode=mode, reps=reps, transform_length=L, sequences=nseq,
                        correlations=slots + slots2, call_s=t, call_s_min=tmin, call_s_max=tmax, symbols_per_s=MODES * n / t,
                        host_route_s=host_s, speedup_over_host_route=host_s / t, equals_host_route=same,
                        delay=rec.delay.tolist(), swap=rec.swap.tolist())
            ft = transforms_alone(lib, n, mode)
            case.update(transforms_s=ft, kernels_launches_and_host_s=t - ft)
            kb = kernel_bytes(n, mode)
            case["kernels"] = {k: dict(bytes=v, hbm_floor_s=v / HBM_BYTES_PER_S) for k, v in kb.items()}
            own = sum(v for k, v in kb.items() if k != "transforms_once")
            case["own_kernels_hbm_floor_s"] = own / HBM_BYTES_PER_S
            cases.append(case)
            print(json.dumps(case), flush=True)
    outd = dict(tool="tools/bench_sync.py", command="python tools/bench_sync.py" + (" --quick" if args.quick else ""),
                device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"), numpy=np.__version__,
                method="3 warm-up calls, median of reps; host clock around synchronous calls; device-resident inputs",
                hbm_bytes_per_s=HBM_BYTES_PER_S, cases=cases)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(outd, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
