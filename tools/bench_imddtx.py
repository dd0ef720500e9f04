#!/usr/bin/env python3
"""Time the IM/DD transmitter and the AWGN channel on one GPU.  Runs on the GPU box only; reads nothing but this repository.

What is timed is the whole device-resident call -- argument checks and draws on the host, uploads of what the host draws, the
launches and the synchronise the call ends in -- with a host clock: warm-up calls per case, then the median, minimum and maximum
of the repetitions.

    pamTransmitter   device_output=True at the IM/DD notebook's settings (PAM-4, 16 samples per symbol, NRZ, 1e5 bits) and at
                     2^20 samples; for comparison simpleWDMTx with one channel at the same N, pulse and constellation (the same
                     filter; it waits for the host between its launches; seeded and unseeded, because a seeded one-mode call also draws the
                     laser walk's normals on the host), and the host route: the same arithmetic in numpy on
                     this box followed by to_device.  The symbol draw on the host is part of each of the three.
    awgn, mzm, upsample, voa   on DeviceArrays of 2^20 samples: call time against the time their bytes take at the copy bandwidth
                     measured in the same run (ssf_device_copy_bandwidth), and numpy on the same box.

Writes profiles/imddtx_bench.json.   Usage: python tools/bench_imddtx.py [--out FILE] [--quick]
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
sys.path[:0] = [ROOT]

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib  # noqa: E402
from opticommpy_amd.wdm_tx import _symbol_source  # noqa: E402


def param(**kw):
    p = oa.parameters()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * statistics.median(ts), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=reps)


def host_mzm(Ei, u, Vpi, Vb, ER):
    erLin = 10 ** (ER / 10)
    g = 2 * np.sqrt(erLin) / (erLin + 1)
    ph = ((u + Vb) / 2 / Vpi) * np.pi
    return np.sqrt(1 + g) * (Ei / 2) * np.exp(1j * ph) + np.sqrt(1 - g) * (Ei / 2) * np.exp(-1j * ph)


def host_pam(nBits, SpS, seed):
    """pamTransmitter's arithmetic at its defaults in numpy (the reference's own sequence of array operations), then the upload."""
    symb = _symbol_source(nBits // 2, 4, "pam", "uniform", 0, seed)
    up = np.zeros(len(symb) * SpS)
    up[::SpS] = symb
    pulse = oa.pulseShape(param(pulseType="nrz", SpS=SpS))
    sig = signal.fftconvolve(up, pulse, mode="same")
    sig = 3 * sig / np.max(np.abs(sig))
    E = host_mzm(1.0, 0.25 * sig, 3, -1.5, 80)
    E = np.sqrt(1e-3 * 10 ** (-3 / 10)) * E / np.sqrt(np.mean(E * np.conj(E)).real)
    return oa.to_device(E)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imddtx_bench.json"))
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert oa.checkGPU(), "this tool measures on a GPU"
    oa.set_device(0)
    lib = _lib.load()
    warm, reps = (1, 3) if a.quick else (3, 21)
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, C.byref(info))
    rec = dict(device=info.name.decode(), arch=info.arch.decode(), warmup=warm, reps=reps, numpy=np.__version__,
               clock="host perf_counter around calls that end in a stream synchronise")

    n20 = 1 << 20
    bw = C.c_double(0.0)
    assert lib.ssf_device_copy_bandwidth(0, 16 * n20, 50, C.byref(bw)) == 0
    rec["measured_copy_GBs"] = bw.value
    rec["measured_copy_note"] = "burst copy kernel, 16 MiB read + 16 MiB written per launch, no arithmetic"

    # ---- pamTransmitter
    pam = {}
    for name, nBits in (("notebook", 100000), ("n2^20", 2 * (n20 // 16))):
        N = nBits // 2 * 16
        row = dict(nBits=nBits, N=N, M=4, SpS=16, pulseType="nrz")
        row["pamTransmitter"] = timed(lambda: oa.pamTransmitter(param(nBits=nBits, seed=5), device_output=True), warm, reps)
        row["simpleWDMTx_one_channel"] = timed(lambda: oa.simpleWDMTx(param(
            M=4, constType="pam", nBits=nBits, SpS=16, pulseType="nrz", nChannels=1, nPolModes=1, seed=5, prgsBar=False), device_output=True), warm, reps)
        # (with a seed and one mode simpleWDMTx also draws the laser walk's N - 1 normals on the host, to leave numpy's stream where
        #  the reference leaves it; without a seed and with zero linewidth it draws the symbols only)
        row["simpleWDMTx_one_channel_unseeded"] = timed(lambda: oa.simpleWDMTx(param(
            M=4, constType="pam", nBits=nBits, SpS=16, pulseType="nrz", nChannels=1, nPolModes=1, prgsBar=False), device_output=True), warm, reps)
        row["pamTransmitter_unseeded"] = timed(lambda: oa.pamTransmitter(param(nBits=nBits), device_output=True), warm, reps)
        row["host_numpy_then_to_device"] = timed(lambda: host_pam(nBits, 16, 5), warm, max(3, reps // 3))
        row["symbol_draw_on_host"] = timed(lambda: _symbol_source(nBits // 2, 4, "pam", "uniform", 0, 5), warm, reps)
        for k in ("pamTransmitter", "pamTransmitter_unseeded", "simpleWDMTx_one_channel", "simpleWDMTx_one_channel_unseeded", "host_numpy_then_to_device"):
            row[k]["ns_per_sample"] = 1e6 * row[k]["median_ms"] / N
        pam[name] = row
    rec["pamTransmitter"] = pam

    # ---- element-wise calls at 2^20 samples
    rng = np.random.default_rng(1)
    x = rng.standard_normal(n20) + 1j * rng.standard_normal(n20)
    u = rng.uniform(-4, 4, n20)
    xd, ud, ucd = oa.to_device(x), oa.to_device(u), oa.to_device(u.astype(np.complex128))
    xs = oa.to_device(x[:n20 // 16])
    pz = param(Vpi=2, Vb=-1, ER=60)
    pa = param(snr=15, seed=3)
    s = np.sqrt(np.mean(np.abs(x) ** 2) / 10 ** 1.5 / 2)

    def np_awgn():
        np.random.seed(3)
        return x + (np.random.normal(0, s, n20) + 1j * np.random.normal(0, s, n20))

    def np_up():
        o = np.zeros(n20, dtype=np.complex128)
        o[::16] = x[:n20 // 16]
        return o
    cases = {
        # name: (device call, numpy call, bytes the algorithm moves)
        "awgn_complex128": (lambda: oa.awgn(xd, pa), np_awgn, 16 * n20 + 16 * n20 + 16 * n20),          # power pass reads, noise pass reads and writes
        "mzm_float64_drive": (lambda: oa.mzm(1.0, ud, pz), lambda: host_mzm(1.0, u, 2, -1, 60), 8 * n20 + 16 * n20),
        "mzm_complex128_drive": (lambda: oa.mzm(1.0, ucd, pz), lambda: host_mzm(1.0, u.astype(np.complex128), 2, -1, 60), 16 * n20 + 16 * n20),
        "upsample_16_to_2^20": (lambda: oa.upsample(xs, 16), np_up, n20 + 16 * n20),
        "voa_complex128": (lambda: oa.voa(xd, 3.0), lambda: x * 10 ** (-3.0 / 20), 32 * n20),
    }
    ew = {}
    for name, (fd, fh, nbytes) in cases.items():
        r = dict(samples=n20, bytes=nbytes, device=timed(fd, warm, reps), numpy=timed(fh, 1, max(3, reps // 3)))
        r["bytes_at_copy_bandwidth_us"] = nbytes / (bw.value * 1e9) * 1e6
        r["call_over_bytes_at_copy_bandwidth"] = r["device"]["median_ms"] * 1e3 / r["bytes_at_copy_bandwidth_us"]
        r["numpy_over_device"] = r["numpy"]["median_ms"] / r["device"]["median_ms"]
        ew[name] = r
    rec["elementwise"] = ew
    rec["note"] = ("call times include the host side of each call (checks, allocation from the pool, the device seed) and its final "
                   "synchronise; a kernel's own time is not separated here")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
