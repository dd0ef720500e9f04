#!/usr/bin/env python3
"""Time the soft-decision FEC functions on the GPU: ``decodeLDPC`` on a graph of DVB-S2 rate-4/5 dimensions with the global engine
and on the 802.11n 648-bit table with the LDS engine, and ``calcLLR`` at 2^20 symbols.  Runs on the GPU box only; reads nothing but
this repository.

The DVB-S2 tables of the reference are not part of this repository (2.6 MB each).  The large graph here is SYNTHETIC: seeded,
n = 64 800 variables, m = 12 960 checks, the degree profile of the DVB-S2 rate-4/5 code -- 6 480 variables of degree 11, 45 360 of
degree 3, the 12 960 parity variables on a staircase (degree 2, the last one 1), 16 information edges and 2 parity edges per check
-- with the information edges dealt to the checks by a seeded permutation (an edge dealt twice to one check is one edge).  Its
decoding threshold is not the standard's; the work per iteration is.

Settings: 30 codewords (the all-zero codeword over BPSK), maxIter = 50, SPA and MSA, float32 and float64, at two noise levels: one
where every codeword converges early and one where none does.  The second runs all 50 iterations and is the throughput figure.
Both are timed with syncEvery = 0 (no host read of the flags; converged codewords are skipped on the device, the launches go on)
and with syncEvery = 5 (the host reads the flags every 5 iterations and stops launching when all are set).  The 648-bit table runs with 30 and with 1 024 codewords on the LDS engine.

An edge update is one edge of one codeword in one iteration (a check update and a variable update of its message):
edge_updates = E x the iterations every codeword ran (lastIter + 1; one more on the global engine, whose check update runs once
speculatively after convergence, is not counted).  bytes_per_edge_update is what the global engine's layout moves per edge update
when nothing is served from a cache twice: two reads and two writes of the message, the edge's two graph indices (int32) and its
variable's decision byte.  implied_GBps = edge updates/s x that; share_of_hbm_peak divides by the 8 TB/s of the data sheet.  A batch
of 30 codewords (28 MB of float32 messages) sits inside the 256 MB Infinity Cache, so that share states how far the call is from
what memory alone would allow, not a measured HBM traffic.

The comparator is the same box's CPU: tests/emu/emu_fec.cpp (g++ -O2, the same node bodies, one thread), 2 codewords at the noise
level where none converges, scaled per codeword.  The reference's numba build does not run without numba.

Method: inputs are uploaded once; 2 warm-up calls per case, then the median of the repetitions of a host clock around calls that
each end in a stream synchronise.  Every figure is the time of a whole call: argument checks, the digest of H, launches, the
download of frameErrors and lastIter, the synchronise.

Writes profiles/fec_bench.json.   Usage: python tools/bench_fec.py [--out FILE] [--quick]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib, fec  # noqa: E402

import fec_cases as fc  # noqa: E402

HBM_PEAK = 8.0e12
NWORDS, MAX_ITER = 30, 50


class Param:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


def dvbs2_like(seed=1):
    """The synthetic graph of the module docstring as a fec.CSR."""
    n, m = 64800, 12960
    k = n - m
    rng = np.random.default_rng(seed)
    deg = np.r_[np.full(6480, 11), np.full(k - 6480, 3)]
    sockets = rng.permutation(np.repeat(np.arange(k), deg))
    assert sockets.size == 16 * m
    rows = np.r_[np.repeat(np.arange(m), 16), np.arange(m), np.arange(1, m)]
    cols = np.r_[sockets, k + np.arange(m), k + np.arange(m - 1)]
    return fec._csr_from_pairs(rows, cols, (m, n))


def llrs_for(n, ncw, snr_dB, seed):
    rng = np.random.default_rng(seed)
    s2 = 10 ** (-snr_dB / 10)
    return (2 * (1 + np.sqrt(s2) * rng.normal(size=(ncw, n))) / s2)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def decode_case(label, H, E, x, alg, prec, engine, reps, syncEvery=0):
    prm = Param(H=H, alg=alg, maxIter=MAX_ITER, prec=np.dtype(prec).type, engine=engine, syncEvery=syncEvery)
    xd = oa.to_device(x.astype(prec))
    _, _, fail, last = oa.decodeLDPC(xd, prm, transposed=True, returnIter=True)
    t, tmin, tmax = timed(lambda: oa.decodeLDPC(xd, prm, transposed=True), 2, reps)
    ncw, w = x.shape[0], np.dtype(prec).itemsize
    updates = float(E) * float(np.sum(last.astype(np.int64) + 1))
    bpe = 4 * w + 8 + 1
    case = dict(case=label, alg=alg, prec=prec, engine=engine, syncEvery=syncEvery, codewords=ncw, n=int(x.shape[1]), edges=int(E),
                maxIter=MAX_ITER, reps=reps, call_s=t, call_s_min=tmin, call_s_max=tmax, frame_errors=int(fail.sum()),
                lastIter_min=int(last.min()), lastIter_max=int(last.max()), edge_updates=updates, edge_updates_per_s=updates / t,
                codewords_per_s=ncw / t, info="an edge update: one edge of one codeword in one iteration")
    if engine == "global":
        case.update(bytes_per_edge_update=bpe, implied_GBps=updates / t * bpe / 1e9, share_of_hbm_peak=updates / t * bpe / HBM_PEAK)
    print(json.dumps(case), flush=True)
    return case


def emu_seconds(exe, tmp, x, prm, engine):
    q = fc.write_emu_ldpc(os.path.join(tmp, "in.bin"), x, prm, engine, transposed=True)
    out = subprocess.check_output([exe, "time", os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin"), "1"])
    last = fc.read_emu_ldpc(os.path.join(tmp, "out.bin"), q)[3]
    return float(out.decode().split()[0]), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fec_bench.json"))
    ap.add_argument("--quick", action="store_true", help="float32 only, few repetitions (rehearsal)")
    args = ap.parse_args()
    if not oa.checkGPU():
        raise SystemExit("bench_fec.py needs a GPU: nothing is measured without one")
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    reps = 3 if args.quick else 7
    precs = ("float32",) if args.quick else ("float32", "float64")
    cases, cpu, llr = [], [], []

    H = dvbs2_like()
    E = H.nnz
    dc, dv = np.diff(H.indptr), np.bincount(H.indices, minlength=H.shape[1])
    graph = dict(n=H.shape[1], m=H.shape[0], edges=E, check_degree_max=int(dc.max()), check_degree_mean=float(dc.mean()),
                 var_degree_max=int(dv.max()), synthetic=True, lds_bytes_float32=_lib.fec_lds_bytes(E, H.shape[1], "float32"))
    SNR_EASY, SNR_HARD = 6.5, 3.0
    easy, hard = llrs_for(H.shape[1], NWORDS, SNR_EASY, 11), llrs_for(H.shape[1], NWORDS, SNR_HARD, 12)
    for prec in precs:
        for alg in ("SPA", "MSA"):
            for every in (0, 5):
                cases.append(decode_case(f"dvbs2-like, snr {SNR_HARD} dB (below threshold)", H, E, hard, alg, prec, "global", reps, every))
            for every in (0, 5):
                cases.append(decode_case(f"dvbs2-like, snr {SNR_EASY} dB (above threshold)", H, E, easy, alg, prec, "global", reps, every))
    H648 = oa.readAlist(fc.ALIST_648)
    for ncw in (30, 1024):
        x = llrs_for(648, ncw, 1.0, 13)
        for prec in precs:
            for alg in ("SPA", "MSA"):
                cases.append(decode_case("802.11n 648b R1/2, snr 1.0 dB (below threshold)", H648, H648.nnz, x, alg, prec, "lds", reps))
        if not args.quick:
            cases.append(decode_case("802.11n 648b R1/2, snr 1.0 dB (below threshold)", H648, H648.nnz, x, "SPA", "float32", "global", reps))

    tmp = tempfile.mkdtemp(prefix="bench_fec_")
    exe = os.path.join(tmp, "emu_fec")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_fec.cpp"), "-o", exe])
    for label, Hc, x, engine in (("dvbs2-like", H, hard[:2], "global"), ("802.11n 648b R1/2", H648, llrs_for(648, 30, 1.0, 13), "lds")):
        for alg in ("SPA", "MSA"):
            prm = Param(H=Hc, alg=alg, maxIter=MAX_ITER, prec=np.float32)
            s, last = emu_seconds(exe, tmp, x.astype(np.float32), prm, engine)
            updates = float(Hc.nnz) * float(np.sum(last.astype(np.int64) + 1))
            c = dict(case=label, alg=alg, prec="float32", codewords=int(x.shape[0]), cpu_emu_s=s, cpu_s_per_codeword=s / x.shape[0],
                     cpu_edge_updates_per_s=updates / s, walk=engine)
            cpu.append(c)
            print(json.dumps(c), flush=True)

    for M in (16, 64, 256):
        rng = np.random.default_rng(M)
        raw = oa.grayMapping(M, "qam")
        bitMap = oa.demodulateGray(raw, M, "qam").reshape(-1, int(np.log2(M)))
        const = (raw / np.sqrt(np.mean(np.abs(raw) ** 2))).astype(np.complex128)
        nsym = 1 << 20
        s2 = 10 ** (-(8 + 3 * np.log2(M)) / 10)
        rx = const[rng.integers(0, M, size=nsym)] + np.sqrt(s2 / 2) * (rng.normal(size=nsym) + 1j * rng.normal(size=nsym))
        rxd = oa.to_device(rx)
        px = np.ones(M) / M
        t, tmin, tmax = timed(lambda: oa.calcLLR(rxd, s2, const, bitMap, px), 2, reps)
        c = dict(M=M, symbols=nsym, call_s=t, call_s_min=tmin, call_s_max=tmax, symbols_per_s=nsym / t, llrs_per_s=nsym * np.log2(M) / t,
                 exp_per_s=nsym * M / t)
        llr.append(c)
        print(json.dumps(c), flush=True)

    out = dict(tool="tools/bench_fec.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=info.compute_units, numpy=np.__version__, synthetic_graph=graph,
               method="2 warm-up calls, median of reps; host clock around synchronous device-resident calls (whole-call times); "
                      "edge_updates = E x sum over codewords of (lastIter + 1); share_of_hbm_peak = edge updates/s x bytes_per_edge_update "
                      "/ 8 TB/s (data sheet), the bytes the layout moves with no cache reuse; cpu_emu_s: tests/emu/emu_fec.cpp built with "
                      "g++ -O2, one thread, its own clock around the decode",
               decode=cases, cpu=cpu, calc_llr=llr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
