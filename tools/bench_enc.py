#!/usr/bin/env python3
"""Time ``encodeLDPC`` and ``modulateGray`` on the GPU.  Runs on the GPU box only; reads nothing but this repository.

Encoder cases, each in both orientations (``(N, k)`` codeword-major with ``transposed=True``, and the reference's ``(k, N)``):
  dvbs2-like   the synthetic graph of tools/bench_fec.py (n = 64 800, m = 12 960, 16 information edges per check), 30 codewords:
               the accumulator kernel, one workgroup per codeword
  648 R1/2     the committed 802.11n table through the generator matrix (G 324 x 648), 30 and 1 024 codewords: the dense kernel
  ar4ja 1280   the AR4JA table of tests/golden/enc through G (1 024 x 1 408, cropped to 1 280), 30 and 1 024 codewords
  floor        the 648 table with one codeword: a call that is all overhead (checks, the digest of the plan, one launch, one
               synchronise)
``modulateGray`` at 2^20 symbols of 16-, 64- and 256-QAM.

Per case: call_s, the median over the repetitions of (a host clock around INNER device-resident calls, each ending in a stream
synchronise) / INNER; ideal_s_at_8TBps, the bytes the call must move (the message bytes in, the codeword bytes out, the matrix
once) over the data sheet's 8 TB/s; host_route_s, the same result by way of the host on the same box: ``.get()``, a bit-packed
numpy encoder (64-bit words, the same GF(2) products and XOR scan), ``to_device``.  The first call of a code also runs the
elimination on the host (par2gen); it is reported once as first_call_s and is not part of call_s.

Writes profiles/enc_bench.json.   Usage: python tools/bench_enc.py [--out FILE] [--quick] [--rehearse]
(--rehearse: no GPU needed; builds every case and checks the host route against tests/enc_restatement.py, times nothing;
 --trace KIND [--codewords N] [--kN]: one case alone, 200 calls, as the workload of `rocprofv3 --kernel-trace --stats`, whose
 database tools/rocpd_stats.py summarises: the kernel times of DESIGN.md 4.13)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import opticommpy_amd as oa  # noqa: E402
from opticommpy_amd import _lib, fec  # noqa: E402

import bench_fec  # noqa: E402
import enc_cases as ec  # noqa: E402
import enc_restatement as er  # noqa: E402
import fec_cases as fc  # noqa: E402

HBM_PEAK = 8.0e12
INNER = 50


def popcount_parity(x):
    """Parity of every 64-bit word."""
    if hasattr(np, "bitwise_count"):
        return (np.bitwise_count(x) & 1).astype(np.uint8)
    return (np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=(-1, -2)) & 1).astype(np.uint8)


def host_encode(plan, bits_Nk, n_out):
    """The packed-numpy encoder of the host route: (N, k) bytes in, (N, n_out) bytes out."""
    N, k = bits_Nk.shape
    if plan["form"] == _lib.ENC_DENSE:
        msg = fec._pack_words(bits_Nk)                                   # (N, W)
        P = np.concatenate(plan["blocks"], axis=0)                      # (rows, W)
        par = np.empty((N, P.shape[0]), dtype=np.uint8)
        step = max(1, (1 << 22) // max(1, P.size))                      # codewords per slab: about 32 MiB of products
        for a in range(0, N, step):
            par[a:a + step] = popcount_parity(np.bitwise_xor.reduce(msg[a:a + step, None, :] & P[None, :, :], axis=2))
        cw = np.concatenate((bits_Nk, par), axis=1) if plan["systematic"] else par
        return np.ascontiguousarray(cw[:, :n_out])
    indptr, indices = plan["indptr"], plan["indices"]
    gathered = np.concatenate((bits_Nk[:, indices], np.zeros((N, 1), dtype=np.uint8)), axis=1)
    par = np.bitwise_xor.reduceat(gathered, np.minimum(indptr[:-1], gathered.shape[1] - 1), axis=1)
    par[:, np.diff(indptr) == 0] = 0                                    # reduceat returns an element for an empty segment
    return np.concatenate((bits_Nk, np.bitwise_xor.accumulate(par, axis=1)), axis=1)[:, :n_out]


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


def codes():
    """name -> (fresh parameter object factory, k)."""
    Hd = bench_fec.dvbs2_like()
    g = ec.load("g_ar4ja_1280")
    return {
        "dvbs2-like 64800 R4/5 (synthetic)": (lambda: ec.Param(mode="DVBS2", n=64800, H=Hd), 64800 - 12960),
        "802.11n 648b R1/2": (lambda: ec.Param(mode="IEEE_802.11nD2", n=648, H=oa.readAlist(fc.ALIST_648)), 324),
        "ar4ja 1280b R4/5": (lambda: ec.Param(mode="AR4JA", n=1280, H=ec.H_of(g)), 1024),
    }


def plan_bytes(plan):
    if plan["form"] == _lib.ENC_DENSE:
        return sum(b.nbytes for b in plan["blocks"])
    return plan["indptr"].nbytes + plan["indices"].nbytes


def encoder_case(label, make_param, k, N, transposed, reps, rehearse):
    rng = np.random.default_rng(N + k)
    msgs = rng.integers(0, 2, size=(N, k)).astype(np.uint8)
    x = msgs if transposed else np.ascontiguousarray(msgs.T)
    prm = make_param()
    t0 = time.perf_counter()
    q = fec._prepare_encode(x, prm, transposed)
    prepare_first = time.perf_counter() - t0
    plan, n_out = q["plan"], q["n_out"]
    host = host_encode(plan, msgs, n_out)
    case = dict(case=label, codewords=N, k=k, n=n_out, transposed=bool(transposed), form="dense" if plan["form"] == _lib.ENC_DENSE else "sparse",
                rows=plan["m1"] + plan["m2"], host_prepare_first_s=prepare_first)
    if rehearse:
        if plan["form"] == _lib.ENC_DENSE:
            want = er.encode_generator(prm.G, msgs.T, True, n_out) if N * k < 2e6 else None
        else:
            ptr, idx = plan["indptr"], plan["indices"]                  # (the dense A of this graph would be 670 MB: one codeword, row by row)
            par = np.array([np.bitwise_xor.reduce(msgs[0, idx[ptr[i]:ptr[i + 1]]]) for i in range(plan["m1"])], dtype=np.uint8)
            want = np.concatenate((msgs[0], np.bitwise_xor.accumulate(par)))[:, None]
            host = host[:1]
        assert want is None or np.array_equal(host.T, want), label
        print(json.dumps(dict(case, rehearsed=True)), flush=True)
        return case
    xd = oa.to_device(x)
    t0 = time.perf_counter()
    first = oa.encodeLDPC(xd, make_param(), transposed=transposed)
    case["first_call_s"] = time.perf_counter() - t0
    got = first.get()
    assert np.array_equal(got if transposed else got.T, host), label
    t, tmin, tmax = timed(lambda: oa.encodeLDPC(xd, prm, transposed=transposed), 2, reps)

    def route():
        b = xd.get()
        cw = host_encode(plan, b if transposed else np.ascontiguousarray(b.T), n_out)
        return oa.to_device(cw if transposed else np.ascontiguousarray(cw.T))

    th, _, _ = timed(route, 1, max(2, reps // 2), inner=1 if N * k > 1e6 else 5)
    nbytes = N * k + N * n_out + plan_bytes(plan)
    case.update(reps=reps, inner=INNER, call_s=t, call_s_min=tmin, call_s_max=tmax, codewords_per_s=N / t, coded_bits_per_s=N * n_out / t,
                bytes=nbytes, ideal_s_at_8TBps=nbytes / HBM_PEAK, share_of_hbm_peak=nbytes / HBM_PEAK / t, host_route_s=th, launches=1)
    print(json.dumps(case), flush=True)
    return case


def trace(kind, N, transposed, calls=200):
    """One case alone, `calls` device-resident calls after two warm-up calls: the workload of a kernel trace
    (``rocprofv3 --kernel-trace --stats -- python tools/bench_enc.py --trace 648 --codewords 1024``; tools/rocpd_stats.py)."""
    if kind == "mod":
        M = N                                                           # (--codewords carries M here)
        bd = oa.to_device(np.random.default_rng(M).integers(0, 2, size=(1 << 20) * int(np.log2(M))).astype(np.uint8))
        fn = lambda: oa.modulateGray(bd, M, "qam")                     # noqa: E731
    else:
        label = [k for k in codes() if k.startswith({"648": "802.11n", "dvbs2": "dvbs2", "ar4ja": "ar4ja"}[kind])][0]
        make_param, k = codes()[label]
        msgs = np.random.default_rng(N + k).integers(0, 2, size=(N, k)).astype(np.uint8)
        xd, prm = oa.to_device(msgs if transposed else np.ascontiguousarray(msgs.T)), make_param()
        fn = lambda: oa.encodeLDPC(xd, prm, transposed=transposed)     # noqa: E731
    for _ in range(calls + 2):
        fn()
    print(f"traced {kind} {N} transposed={transposed}: {calls + 2} calls")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", default="", help="dvbs2 | 648 | ar4ja | mod: run that case alone (under a kernel trace), time nothing")
    ap.add_argument("--codewords", type=int, default=30, help="--trace: the batch (for mod: M)")
    ap.add_argument("--kN", action="store_true", help="--trace: the reference's (k, N) orientation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enc_bench.json"))
    ap.add_argument("--quick", action="store_true", help="few repetitions (rehearsal on the GPU)")
    ap.add_argument("--rehearse", action="store_true", help="no GPU: build every case, check the host route, time nothing")
    args = ap.parse_args()
    if not args.rehearse and not oa.checkGPU():
        raise SystemExit("bench_enc.py needs a GPU: nothing is measured without one")
    if args.trace:
        return trace(args.trace, args.codewords, not args.kN)
    reps = 3 if args.quick else 7
    enc, mod = [], []
    for label, (make_param, k) in codes().items():
        for N in ((30,) if label.startswith("dvbs2") else (30, 1024)):
            for transposed in (True, False):
                enc.append(encoder_case(label, make_param, k, N, transposed, reps, args.rehearse))
    label = "802.11n 648b R1/2"
    enc.append(encoder_case(label + " (floor: one codeword)", codes()[label][0], 324, 1, True, reps, args.rehearse))
    if args.rehearse:
        print("rehearsal passed: nothing measured")
        return
    for M in (16, 64, 256):
        b = int(np.log2(M))
        nsym = 1 << 20
        bits = np.random.default_rng(M).integers(0, 2, size=nsym * b).astype(np.uint8)
        bd = oa.to_device(bits)
        assert np.array_equal(oa.modulateGray(bd, M, "qam").get(), er.modulate(bits, M, "qam").astype(np.complex128))
        t, tmin, tmax = timed(lambda: oa.modulateGray(bd, M, "qam"), 2, reps, inner=20)
        table = oa.grayMapping(M, "qam").astype(np.complex128)
        weights = 1 << np.arange(b - 1, -1, -1)

        def route():
            return oa.to_device(table[bd.get().reshape(-1, b) @ weights])

        th, _, _ = timed(route, 1, 3, inner=1)
        nbytes = nsym * b + nsym * 16 + M * 16
        c = dict(M=M, symbols=nsym, reps=reps, inner=20, call_s=t, call_s_min=tmin, call_s_max=tmax, symbols_per_s=nsym / t, bytes=nbytes,
                 ideal_s_at_8TBps=nbytes / HBM_PEAK, share_of_hbm_peak=nbytes / HBM_PEAK / t, host_route_s=th, launches=1)
        mod.append(c)
        print(json.dumps(c), flush=True)
    lib = _lib.load()
    info = _lib.DeviceInfo()
    lib.ssf_device_info(0, info)
    out = dict(tool="tools/bench_enc.py", device=info.name.decode(errors="replace"), arch=info.arch.decode(errors="replace"),
               compute_units=info.compute_units, numpy=np.__version__,
               method="2 warm-up calls, then the median over reps of (host clock around `inner` device-resident calls, each ending in a "
                      "stream synchronise) / inner: whole-call times (argument checks, the comparison of H with the matrices seen last, "
                      "the digest of the plan, one launch, the synchronise).  ideal_s_at_8TBps = (message bytes + codeword bytes + the "
                      "matrix once) / 8 TB/s (data sheet); the arrays of every case but the 2^20-symbol mapper fit in the Infinity Cache, "
                      "so the share says how far a call is from what memory alone would allow, not a measured HBM traffic.  "
                      "host_route_s: .get(), a bit-packed numpy encoder (or table[index]), to_device, on the same box.  "
                      "first_call_s includes the host elimination (par2gen) and the upload of the matrices; the floor case is a call "
                      "that is all overhead.",
               encode=enc, modulate=mod)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
