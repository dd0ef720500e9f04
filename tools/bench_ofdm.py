#!/usr/bin/env python3
"""Time ``modulateOFDM`` and ``demodulateOFDM`` on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Cases (64-QAM, pilots 0.52 (max Re + j max Im), the received signal is the transmit signal at one sample per symbol):
  notebook     256 carriers, G 4, SpS 2, 4 pilots, null [128], 1000 frames: examples/test_ofdm.ipynb
  large        1024 carriers x 1024 frames, G 16, SpS 2, 8 pilots
  rocfft       1000 carriers, G 16, SpS 2, 8 pilots, 1000 frames: no power of two, the rocFFT route
  notebook via rocFFT   the notebook's setting with the rocFFT route asked for: the two routes side by side

Per case and function: call_s, the median over the repetitions of (a host clock around INNER device-resident calls, each ending in
a stream synchronise) / INNER, for complex128 in and out and for complex64; ideal_s_at_8TBps, the bytes the call must move (the
input once, the output once) over the data sheet's 8 TB/s; host_route_s, the same result by way of the host on the same box:
``.get()``, the numpy restatement vectorised over the frames (tests/ofdm_restatement.py frame by frame is the reference's loop;
this is the fastest numpy a user would write), ``to_device``.

Writes profiles/ofdm_bench.json.   Usage: python tools/bench_ofdm.py [--out FILE] [--quick] [--rehearse]
(--rehearse: no GPU needed; builds every case at a few frames and checks the host route against tests/ofdm_restatement.py,
 times nothing;
 --trace CASE: that case alone in complex128, 200 calls of each function, as the workload of `rocprofv3 --kernel-trace --stats`,
 whose database tools/rocpd_stats.py summarises: the kernel times of DESIGN.md 4.14)
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib, ofdm  # noqa: E402

import ofdm_restatement as rs  # noqa: E402

HBM_PEAK = 8.0e12
INNER = 50

CASES = {
    "notebook": dict(Nfft=256, G=4, SpS=2, npilots=4, frames=1000, route="auto"),
    "large": dict(Nfft=1024, G=16, SpS=2, npilots=8, frames=1024, route="auto"),
    "rocfft": dict(Nfft=1000, G=16, SpS=2, npilots=8, frames=1000, route="auto"),
    "notebook via rocFFT": dict(Nfft=256, G=4, SpS=2, npilots=4, frames=1000, route="rocfft"),
}


class Param:
    pass


def build(c, frames):
    const = oa.grayMapping(64, "qam").astype(np.complex128)
    const = const / np.sqrt(np.mean(np.abs(const) ** 2))
    p = Param()
    p.Nfft, p.G, p.SpS = c["Nfft"], c["G"], c["SpS"]
    p.pilot = 0.52 * (np.max(const.real) + 1j * np.max(const.imag))
    p.pilotCarriers = np.int64(np.linspace(0, c["Nfft"] - 1, c["npilots"]))
    p.nullCarriers = np.array([c["Nfft"] // 2], dtype=np.int64)
    p.returnChannel = False
    Ni = c["Nfft"] - c["npilots"] - 1
    symb = const[np.random.default_rng(1).integers(0, 64, size=frames * Ni)]
    return p, symb


def host_modulate(symb, p, plan):
    """modulateOFDM in numpy, all frames at once."""
    F = len(symb) // plan["Ni"]
    V = np.zeros((F, plan["Ns"]), dtype=np.complex64)
    V[:, plan["data"]] = symb.reshape(F, -1)
    V[:, plan["pilots"]] = p.pilot
    pad = (p.Nfft * (p.SpS - 1)) // 2
    X = np.fft.fftshift(np.pad(V.astype(np.complex128), ((0, 0), (pad, pad))), axes=1)
    x = np.fft.ifft(X, axis=1) * np.sqrt(p.SpS * p.Nfft)
    return np.concatenate((x[:, x.shape[1] - p.SpS * p.G:], x), axis=1).ravel()


def host_demodulate(sig, p, plan):
    """demodulateOFDM in numpy, all frames at once (the pilots' magnitudes and angles averaged before the lines are drawn)."""
    F = len(sig) // (p.Nfft + p.G)
    Y = np.fft.fftshift(np.fft.fft(sig.reshape(F, -1)[:, p.G:], axis=1), axes=1) / np.sqrt(p.Nfft)
    est = Y[:, plan["pilots"]] / p.pilot
    c = np.arange(plan["Ns"], dtype=np.float64)
    H = rs.line_through(plan["pilots"], np.abs(est).mean(axis=0), c) * np.exp(1j * rs.line_through(plan["pilots"], np.angle(est).mean(axis=0), c))
    return (Y / H)[:, plan["data"]].ravel()


def timed(fn, warmup, reps, inner=INNER):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ts.append((time.perf_counter() - t0) / inner)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ofdm_bench.json"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--trace", default="", help="a case's name: run it alone (under a kernel trace), time nothing")
    a = ap.parse_args()
    if a.rehearse:
        for name, c in CASES.items():
            p, symb = build(c, 3)
            plan = ofdm._prepare_mod(symb, p)["plan"]
            kw = dict(Nfft=p.Nfft, G=p.G, pilot=p.pilot, SpS=p.SpS, pilotCarriers=p.pilotCarriers, nullCarriers=p.nullCarriers)
            tx = host_modulate(symb, p, plan)
            want = rs.modulate(symb, **kw)
            assert np.max(np.abs(tx - want)) <= 1e-12 * np.max(np.abs(want)), name
            rx = np.sqrt(p.SpS) * tx[::p.SpS]
            dem, want = host_demodulate(rx, p, plan), rs.demodulate(rx, **kw)[0]
            assert np.max(np.abs(dem - want)) <= 1e-9 * np.max(np.abs(want)), name
            print(f"{name}: host route agrees with the restatement")
        return
    assert oa.checkGPU(), "bench_ofdm.py measures on a GPU"
    if a.trace:
        c = CASES[a.trace]
        p, symb = build(c, c["frames"])
        sd = oa.to_device(symb)
        tx = oa.modulateOFDM(sd, p, dtype=np.complex128, _route=c["route"])
        rd = oa.to_device(np.sqrt(p.SpS) * tx.get()[::p.SpS])
        for _ in range(200):
            oa.modulateOFDM(sd, p, dtype=np.complex128, _route=c["route"])
        for _ in range(200):
            oa.demodulateOFDM(rd, p, _route=c["route"])
        return
    warmup, reps = (2, 3) if a.quick else (5, 9)
    res = dict(device=_lib.load().ssf_version().decode(), inner=INNER, reps=reps, hbm_peak=HBM_PEAK, cases={})
    for name, c in CASES.items():
        p, symb = build(c, c["frames"])
        plan = ofdm._prepare_mod(symb, p)["plan"]
        entry = dict(c, Ni=plan["Ni"], samples_tx=c["frames"] * p.SpS * (p.Nfft + p.G))
        for dt in (np.complex128, np.complex64):
            tag = np.dtype(dt).name
            sd = oa.to_device(symb.astype(dt))
            tx = oa.modulateOFDM(sd, p, dtype=dt, _route=c["route"])
            rx_h = (np.sqrt(p.SpS) * tx.get()[::p.SpS]).astype(dt)
            rd = oa.to_device(rx_h)
            med, lo, hi = timed(lambda: oa.modulateOFDM(sd, p, dtype=dt, _route=c["route"]), warmup, reps)
            m = dict(call_s=med, min_s=lo, max_s=hi, ideal_s_at_8TBps=(sd.nbytes + tx.nbytes) / HBM_PEAK)
            m["host_route_s"], _, _ = timed(lambda: oa.to_device(host_modulate(sd.get(), p, plan).astype(dt)), 1, 3, 1)
            entry[f"modulate_{tag}"] = m
            out = oa.demodulateOFDM(rd, p, _route=c["route"])
            med, lo, hi = timed(lambda: oa.demodulateOFDM(rd, p, _route=c["route"]), warmup, reps)
            d = dict(call_s=med, min_s=lo, max_s=hi, ideal_s_at_8TBps=(rd.nbytes + out.nbytes) / HBM_PEAK)
            d["host_route_s"], _, _ = timed(lambda: oa.to_device(host_demodulate(rd.get(), p, plan).astype(dt)), 1, 3, 1)
            entry[f"demodulate_{tag}"] = d
            # what is timed is right: against the host route
            err = np.max(np.abs(out.get() - host_demodulate(rx_h, p, plan))) / np.max(np.abs(out.get()))
            d["rel_err_vs_host_route"] = float(err)
            assert err <= (1e-9 if dt is np.complex128 else 1e-5), (name, tag, err)
            print(f"{name} {tag}: modulate {m['call_s'] * 1e6:.1f} us (ideal {m['ideal_s_at_8TBps'] * 1e6:.2f}, host route "
                  f"{m['host_route_s'] * 1e6:.0f}), demodulate {d['call_s'] * 1e6:.1f} us (ideal {d['ideal_s_at_8TBps'] * 1e6:.2f}, host route "
                  f"{d['host_route_s'] * 1e6:.0f})", flush=True)
        res["cases"][name] = entry
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
