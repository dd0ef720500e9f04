#!/usr/bin/env python3
"""bench.py -- SSFM steps/s on MI355X for BASELINE.json's configurations.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 1|2|3|4|5] [--dump-outputs DIR] [--full]

A plain run does what the headline figure needs and nothing else: it sets up, warms up, times the K steps, writes the outputs if
--dump-outputs is given and prints the result line.  --full adds, after the timed steps and outside them, everything else this
file measures or checks: the parity gate of the run (CPU oracle with its cpu_baseline, or a reference-generated fixture), the
per-kernel HIP-event pass, the measured copy ceiling of the roofline and, for the default configuration on one GPU, the "also"
legs (configs 3, 2 out of cache, 4, 5, 1 x 16, the receiver chain, the reference notebook's benchmark).  --parity, --cpu-steps,
--no-cpu-baseline, --no-kernel-times and --no-also choose among those and mean nothing without --full.

--dump-outputs DIR: the output field of every unit after the K timed steps, as DIR/unit<u>.npy (float64 / float32 [real, imag]
pairs; at most 64 MB in all, a fixed seeded sample of sample positions beyond that -- dump_outputs).  The inputs are seeded: the
same arguments give the same inputs, so two builds can be compared output for output.

One "step" = one pass of `while z_current < Lspan` (reference optic/models/channels.py:387; the inner `for` of
ssfm, :219).  The timed region runs EXACTLY K steps per unit with every input already resident in HBM (uploads
before, downloads after), bracketed by a barrier on both sides; the time is the MAX over ranks.

  config 2 (default, BASELINE's headline; at N > 1 one independent field per GPU, seeds 2, 3, ...: weak scaling):
            manakovSSF, 2-pol, N = 2^20 complex128, hz 0.08, 8.4 dBm
  config 1: ssfm, N = 2^16 complex128, hz 0.5, 0 dBm, seed 1
  config 3: manakovSSF, N = 2^22 complex64 (+ prec complex64), hz 0.08, 8.4 dBm, seed 3
  config 4: 16 independent config-2 units, seeds 100..115, launch powers 8.4 + arange(-8, 0, 0.5) dB, split in
            contiguous blocks over the ranks (16 / 8 / 4 / 2 units per GPU): strong scaling (--config 4 or
            SSF_BENCH_CONFIG=4; not the default because the driver's scaling curve needs the N = 1 workload at every N)
  config 5: 8 units (seeds 200..207): forward config-2 leg, then manakovDBP over the same span chained on the
            device (--dbp-hz, default 0.08 km: the bandwidth-relevant setting; the notebook's is 10 km)

N > 1: the driver starts one process per GPU (torchrun is only the process launcher); the ranks meet through RCCL bound
inside libssf_hip.so (opticommpy_amd.mgpu.RcclComm): the parameter block is broadcast from rank 0, rank 0 synthesises the
inputs of ALL units and scatters them (ncclSend / ncclRecv), barriers and the max-over-ranks time are all-reduces, the
per-unit output checksums are all-gathered.  No per-step communication.  Units of a rank run on two
lanes (plan + stream + host thread each) so that one unit's row launches overlap the other's column launches.

Prints ONE JSON line on rank 0; with --full, exits non-zero if the in-run parity check against the CPU oracle fails.
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FS = 512e9


def synth_field(N, ncols, seed, p_dbm, dtype=np.complex128):
    """SURVEY.md 8d input recipe: band-limited complex Gaussian, each column P/2."""
    rng = np.random.default_rng(seed)
    E = (rng.normal(size=(N, ncols)) + 1j * rng.normal(size=(N, ncols))) / np.sqrt(2)
    F = np.fft.fft(E, axis=0)
    F[N // 4: 3 * N // 4, :] = 0
    E = np.fft.ifft(F, axis=0)
    p_lin = 10 ** (p_dbm / 10) * 1e-3
    E = E * np.sqrt((p_lin / 2) / np.mean(np.abs(E) ** 2, axis=0))
    return E.astype(dtype)


def synth_unit(N, ncols, seed, p_dbm, dtype, nfields=1, via_c64=False):
    """(ncols, N) SoA block of one unit; nfields > 1 (ssfm): row f is the field of seed + f; via_c64: complex64 samples cast up
    (the input of the reference's complex128 run in tests/golden/wl_cfg3_n22.npz)"""
    if via_c64:
        return np.ascontiguousarray(synth_field(N, ncols, seed, p_dbm, np.complex64).T).astype(dtype)
    if nfields > 1:
        return np.ascontiguousarray(np.concatenate([synth_field(N, 1, seed + f, p_dbm, dtype).T for f in range(nfields)], axis=0))
    return np.ascontiguousarray(synth_field(N, ncols, seed, p_dbm, dtype).T)


def workload(cfg, log2n, prec, world):
    """-> dict(model, log2n, prec, hz, units=[(seed, dBm)], dbp, scaling, text)"""
    w = dict(model="manakov", log2n=20, prec="c128", hz=0.08, dbp=False, scaling="weak")
    if cfg == 1:
        w.update(model="nlse", log2n=16, hz=0.5, units=[(1 + r, 0.0) for r in range(world)],
                 text="ssfm config-1: 1-pol N=2^16 complex128, hz=0.5 km, 0 dBm, amp=None, 1 independent field per GPU")
    elif cfg == 2:
        w.update(units=[(2 + r, 8.4) for r in range(world)],
                 text="manakovSSF config-2: 2-pol N=2^20 complex128, hz=0.08 km fixed, 8.4 dBm, amp=ideal, 1 independent field per GPU")
    elif cfg == 3:
        w.update(log2n=22, prec="c64", units=[(3 + r, 8.4) for r in range(world)],
                 text="manakovSSF config-3 shape: 2-pol N=2^22 complex64 (prec complex64), hz=0.08 km fixed, 8.4 dBm, amp=ideal, "
                      "K steps of one span (the full configuration is 10 spans x 1001 steps), 1 independent field per GPU")
    elif cfg == 4:
        w.update(units=[(100 + u, 8.4 - 8.0 + 0.5 * u) for u in range(16)], scaling="strong",
                 text="manakovSSF config-4: 16 independent 2-pol N=2^20 complex128 units (seeds 100..115, launch powers "
                      "0.4..7.9 dBm in 0.5 dB steps), hz=0.08 km, amp=ideal, contiguous blocks of 16/G units per GPU, two lanes per GPU")
    elif cfg == 5:
        w.update(units=[(200 + u, 8.4) for u in range(8)], scaling="strong", dbp=True,
                 text="config-5: 8 independent 2-pol N=2^20 complex128 units (seeds 200..207, 8.4 dBm): manakovSSF forward "
                      "(hz 0.08, amp=ideal) then manakovDBP over the same span, chained in device memory, 8/G units per GPU")
    else:
        raise SystemExit("unknown --config")
    if log2n:
        w["log2n"] = log2n
        w["text"] += " [--log2n %d]" % log2n
    if prec:
        w["prec"] = prec
        w["text"] += " [--prec %s]" % prec
    return w


def make_params(lib_mod, w, steps, direction=1, hz=None):
    cp = lib_mod.Params()
    hz = hz or w["hz"]
    cp.model = lib_mod.MODEL_NLSE if w["model"] == "nlse" else lib_mod.MODEL_MANAKOV
    cp.direction = direction
    cp.Fs, cp.Fc, cp.alpha, cp.D, cp.gamma = FS, 193.1e12, 0.2, 16.0, 1.3
    if w["model"] == "nlse":
        cp.Lspan = steps * hz                    # floor(Lspan / hz) passes of the inner loop (channels.py:213)
        cp.amp = lib_mod.AMP_NONE
    else:
        cp.Lspan = (steps - 0.5) * w["hz"]       # exactly `steps` passes of the while loop (the last one is half a step)
        cp.amp = lib_mod.AMP_IDEAL
    cp.Nspans, cp.hz, cp.maxIter, cp.tol = 1, hz, 10, 1e-5
    cp.nlprMethod, cp.maxNlinPhaseRot, cp.NF = 0, 2e-2, 4.5
    cp.n_save, cp.save_spans = 0, None
    return cp


def oracle_run(w, E, n, dtype):
    from oracle import ssf_oracle as orc
    p = orc.parameters()
    p.Fs, p.Fc, p.alpha, p.D, p.gamma = FS, 193.1e12, 0.2, 16, 1.3
    p.prgsBar, p.prec = False, dtype
    tr = {}
    t0 = time.perf_counter()
    if w["model"] == "nlse":
        p.Ltotal = p.Lspan = n * w["hz"]
        p.hz, p.amp = w["hz"], None
        ref = orc.ssfm(E[:, 0].copy(), p, trace=tr).reshape(-1, 1)
        tr["iterations"] = 0
    else:
        p.Ltotal = p.Lspan = (n - 0.5) * w["hz"]
        p.hz, p.maxIter, p.tol, p.nlprMethod, p.amp, p.saveSpanN = w["hz"], 10, 1e-5, False, "ideal", []
        ref = orc.manakovSSF(E, p, trace=tr)
    return ref, time.perf_counter() - t0, tr


def unit_checksum(out, seed=4242):
    """(power, projection) of one unit's output (rows, N): sum |E|^2 and |sum_rn E[r, n] q[r, n]| with a seeded
    unit-variance complex vector q -- the power alone cannot tell two units of equal launch power apart."""
    o = out.astype(np.complex128)
    rng = np.random.default_rng(seed)
    q = (rng.normal(size=o.shape) + 1j * rng.normal(size=o.shape)) / np.sqrt(2)
    return float(np.sum(np.abs(o) ** 2)), float(np.abs(np.vdot(q, o)))


def free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(n):
    """--gpus N without a launcher: start the N ranks ourselves (one process per GPU, the environment torchrun would
    export, a fresh private directory for the RCCL rendezvous file) and relay rank 0's JSON line."""
    import shutil
    import subprocess
    import tempfile
    tmp = tempfile.mkdtemp(prefix="ssf_bench_")
    port = str(free_port())
    nonce = "%s-%d-%.6f" % (port, os.getpid(), time.time())       # ONE job identity for all ranks (mgpu.RcclComm._nonce)
    procs = []

    def die_with_parent():                                      # a killed launcher must not leave ranks behind
        try:
            C.CDLL("libc.so.6").prctl(1, 9)                      # PR_SET_PDEATHSIG, SIGKILL
        except Exception:
            pass
    try:
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=port, SSF_RCCL_ID_FILE=os.path.join(tmp, "rccl.id"),
                       SSF_RCCL_NONCE=nonce,
                       HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, preexec_fn=die_with_parent))
        chunks = []
        rd = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
        rd.start()
        failed_at = None
        while any(p.poll() is None for p in procs):             # a rank that dies leaves the others in a collective:
            if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
                failed_at = time.time()
            if failed_at is not None and time.time() - failed_at > 10.0:
                break                                           # ... give them ten seconds, then end the run
            time.sleep(0.05)
        for p in procs:
            if p.poll() is None:
                p.kill()
        rcs = [p.wait() for p in procs]
        rd.join(5.0)
        out0 = b"".join(chunks).decode(errors="replace")
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        shutil.rmtree(tmp, ignore_errors=True)
    sys.stdout.write(out0)
    sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc]
    if bad:
        sys.stderr.write("bench.py --gpus %d: rank(s) failed: %s\n" % (n, bad))
        sys.exit(1)
    sys.exit(0)



def measure(env, cfg, m):
    """One configuration: synthesise / scatter the inputs, warm up, time EXACTLY m.steps steps per unit, gather the per-unit
    checksums, and (rank 0) build the record with the roofline and, under m.full, the per-kernel pass, the copy probe and the
    parity leg m.parity asks for.
    -> (rec or None, ok)"""
    lib, _lib, mgpu, comm, comm_name = env.lib, env._lib, env.mgpu, env.comm, env.comm_name
    rank, world, local_rank = env.rank, env.world, env.local_rank
    w = workload(cfg, m.log2n, m.prec, world)
    if m.nfields > 1:
        assert w["model"] == "nlse" and world == 1
        w["text"] += " [%d independent fields as the rows of ONE plan: every launch carries all of them]" % m.nfields
    w = mgpu.bcast_object(comm, w, 0)                           # "broadcast of the parameter block"
    N = 1 << w["log2n"]
    dtype = np.complex128 if w["prec"] == "c128" else np.complex64
    prec = _lib.SSF_C128 if w["prec"] == "c128" else _lib.SSF_C64
    s = 16 if w["prec"] == "c128" else 8
    ncols = m.nfields if w["model"] == "nlse" else 2
    engine = {"auto": 0, "rocfft": 1, "fused": 2}[m.engine]
    U = len(w["units"])
    mine = list(mgpu.shard_range(U, world, rank))

    # ---- inputs: rank 0 synthesises every unit and scatters (weak-scaling configs: every rank makes its own field)
    fields = {}
    if w["scaling"] == "strong" and comm is not None and world > 1:
        for r in range(world):
            for u in mgpu.shard_range(U, world, r):
                if rank == 0:
                    E = synth_unit(N, ncols, *w["units"][u], dtype)
                    if r == 0:
                        fields[u] = E
                    else:
                        comm.send(E, r)
                elif rank == r:
                    fields[u] = comm.recv(np.empty((ncols, N), dtype=dtype), 0)
    else:
        for u in mine:
            fields[u] = synth_unit(N, ncols, *w["units"][u], dtype, m.nfields, getattr(m, "samples_c64", False))

    # ---- the inputs are device-resident before anything is timed: one HBM copy per unit, from which every run (warm-up,
    # timed, profiling, parity) re-initialises its plan by a device copy -- no PCIe transfer (and no idle GPU) between the
    # warm-up steps and the timed ones
    dev_in = {}
    host_in = bool(os.environ.get("SSF_BENCH_HOST_INPUT"))     # (A/B switch: re-upload from host memory before every run, as rounds 1-2 did)
    t_h2d0 = time.perf_counter()                                # (what there is to measure beside the compute time of a
    for u in mine:                                              #  sharded run is the host-side transfer of inputs and results)
        if host_in:
            dev_in[u] = fields[u].ctypes.data_as(C.c_void_p)
            continue
        q = C.c_void_p()
        _lib.raise_for(lib, None, lib.ssf_device_malloc(local_rank, fields[u].nbytes, C.byref(q)))
        _lib.raise_for(lib, None, lib.ssf_device_memcpy(local_rank, q, fields[u].ctypes.data_as(C.c_void_p), fields[u].nbytes))
        dev_in[u] = q
    h2d_ms = (time.perf_counter() - t_h2d0) * 1e3
    h2d_bytes = 0 if host_in else sum(fields[u].nbytes for u in mine)

    # ---- one plan per unit (its field stays resident in HBM), units dealt to the lanes alternately
    plans = {}
    for u in mine:
        h = C.c_void_p()
        _lib.raise_for(lib, None, lib.ssf_plan_create(local_rank, N, ncols, prec, engine, C.byref(h)))
        plans[u] = h
    lanes = max(1, min(m.lanes, len(mine)))
    if lanes > 1:                                               # the plans of a rank share its GPU: no phase priorities (ssf.h)
        for h in plans.values():
            lib.ssf_plan_set_lanes(h, lanes)
    lane_units = [mine[i::lanes] for i in range(lanes)]

    def run_unit(u, steps, stats):
        h = plans[u]
        st = _lib.Stats()
        cp = make_params(_lib, w, steps)
        rc = lib.ssf_execute(h, C.byref(cp), 1, 1, None, C.byref(st), None)              # synchronous at return
        if rc == 0 and w["dbp"]:
            cpb = make_params(_lib, w, steps, direction=-1, hz=m.dbp_hz)
            rc = lib.ssf_execute(h, C.byref(cpb), 1, 1, None, C.byref(st), None)         # chained: the field never leaves HBM
        stats[u] = (rc, st)

    def run_all(steps, sync=True):
        for u in mine:
            _lib.raise_for(lib, plans[u], lib.ssf_upload(plans[u], dev_in[u]))
        stats = {}
        if comm is not None and sync:
            comm.barrier()
        t0 = time.perf_counter()
        if lanes == 1:
            for u in mine:
                run_unit(u, steps, stats)
        else:
            th = [threading.Thread(target=lambda us=us: [run_unit(u, steps, stats) for u in us]) for us in lane_units]
            for t in th:
                t.start()
            for t in th:
                t.join()
        t1 = time.perf_counter()
        for u in mine:
            _lib.raise_for(lib, plans[u], stats[u][0])
        return t1 - t0, {u: stats[u][1] for u in mine}

    if m.warmup > 0:
        run_all(m.warmup)
    dt_local, sts = run_all(m.steps)
    steps_local = sum(int(st.steps) for st in sts.values())
    fwd_steps = m.steps * len(mine)
    assert steps_local >= fwd_steps and (w["dbp"] or steps_local == fwd_steps), (steps_local, fwd_steps)
    dt = dt_local
    steps_total = steps_local
    if comm is not None:
        dt = float(comm.allreduce(np.array([dt_local]), "max")[0])
        steps_total = int(round(comm.allreduce(np.array([float(steps_local)]), "sum")[0]))
        comm.barrier()

    # results: per-unit checksum, all-gathered ("gather of results only")
    outs = {}
    t_d2h0 = time.perf_counter()
    for u in mine:
        o = np.empty_like(fields[u])
        _lib.raise_for(lib, plans[u], lib.ssf_download(plans[u], o.ctypes.data_as(C.c_void_p)))
        outs[u] = o
    d2h_ms = (time.perf_counter() - t_d2h0) * 1e3
    d2h_bytes = sum(o.nbytes for o in outs.values())
    if getattr(m, "dump_outputs", None):
        dump_outputs(m.dump_outputs, outs, U)
    xfer = np.array([[h2d_ms, d2h_ms, dt_local * 1e3, float(h2d_bytes), float(d2h_bytes)]])
    xfer_all = comm.allgather(xfer)[:, 0, :] if comm is not None else xfer
    per = max(len(mgpu.shard_range(U, world, r)) for r in range(world))
    cs = np.zeros((per, 3))
    for i, u in enumerate(mine):
        cs[i] = unit_checksum(outs[u]) + (float(sts[u].iterations),)
    if comm is not None:
        allcs = comm.allgather(cs)
        checksums = [[float(x) for x in allcs[r][i]] for r in range(world) for i in range(len(mgpu.shard_range(U, world, r)))]
    else:
        checksums = [[float(x) for x in c] for c in cs[:len(mine)]]

    rec = None
    ok = True
    if rank == 0:
        u0 = mine[0]
        st0 = sts[u0]
        bytes_local = sum(float(st.bytes_algorithmic) for st in sts.values())
        if len(mine) == 1:                                      # HIP events on the plan stream around the K timed steps
            dev_s = st0.device_ms * 1e-3
            timing = "HIP events around the K timed steps on the plan stream"
        else:                                                   # several units on concurrent lanes: wall time of the rank
            dev_s = dt_local
            timing = "wall time of rank 0's timed region (its %d units run on %d concurrent lanes)" % (len(mine), lanes)
        achieved = bytes_local / dev_s / 1e9
        it_step = sum(int(st.iterations) for st in sts.values()) / max(steps_local, 1)
        rec = {
            "metric": "SSFM steps/sec (%d-pol, 2^%d samples)" % (1 if w["model"] == "nlse" else 2, w["log2n"]),
            "value": steps_total * m.nfields / dt, "unit": "steps/s" if m.nfields == 1 else "field-steps/s",
            "n_gpus": world, "steps": m.steps, "warmup": m.warmup,
            "ms_per_step": dt / m.steps * 1e3, "higher_is_better": True, "scaling": w["scaling"],
            "vs_baseline": None, "dtype": "f64" if s == 16 else "f32", "data": "synthetic",
            "config": {"workload": w["text"], "baseline_config": cfg, "engine": _lib.ENGINE_NAMES[st0.engine],
                       "pipeline": _lib.PIPELINE_NAMES.get(lib.ssf_plan_pipeline(plans[u0]), "?"),
                       "units_total": U, "units_per_gpu": len(mine), "lanes_per_gpu": lanes,
                       "unit_steps_total": steps_total, "iterations_per_step": it_step,
                       # per rank, outside the timed region: inputs host -> HBM before the first run, results HBM -> host after the
                       # timed one (pinned double-buffered staging, ssf_copy.h), beside that rank's timed compute time
                       "h2d_ms": [float(x) for x in xfer_all[:, 0]], "d2h_ms": [float(x) for x in xfer_all[:, 1]],
                       "compute_ms": [float(x) for x in xfer_all[:, 2]],
                       "h2d_GBs": [float(b / max(t, 1e-9) / 1e6) for t, b in zip(xfer_all[:, 0], xfer_all[:, 3])],
                       "d2h_GBs": [float(b / max(t, 1e-9) / 1e6) for t, b in zip(xfer_all[:, 1], xfer_all[:, 4])],
                       "transforms_per_step": sum(int(st.transforms) for st in sts.values()) / max(steps_local, 1)},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                         "kernel": "whole step pipeline of one GPU (rank 0): " + timing,
                         "algorithmic_bytes_per_step": bytes_local / max(steps_local, 1),
                         "device_ms_per_step": dev_s * 1e3 / max(steps_local, 1),
                         "note": "the working set of a 2^20 complex128 field (184 MiB) fits the 256 MiB Infinity Cache: the "
                                 "'HBM' figure of config 2 is partly an Infinity-Cache figure; configs with N >= 2^21 "
                                 "(complex128) / 2^22 run out of it (out-of-cache fraction of the same complex128 kernels: "
                                 "python bench.py --log2n 22, profiles/r3_c2_out_of_cache.json)"},
            "comm": comm_name, "rccl_ranks": world if comm is not None and comm_name.startswith("RCCL") else 0,
            "unit_checksums": checksums,          # per unit: [sum |E|^2, |<q, E>|, iterations] with a seeded random vector q
        }

        # per-kernel timing pass (HIP events around every launch; separate from the headline run because the events
        # themselves cost a few microseconds per launch)
        if m.full and not m.no_kernel_times and w["model"] == "manakov" and lib.ssf_set_profiling(plans[u0], 1) == 0:
            nprof = min(m.steps, 200)
            _lib.raise_for(lib, plans[u0], lib.ssf_upload(plans[u0], dev_in[u0]))
            stp = {}
            run_unit(u0, nprof, stp)
            kt = _lib.KernelTimes()
            lib.ssf_get_kernel_times(plans[u0], C.byref(kt))
            lib.ssf_set_profiling(plans[u0], 0)
            bytes_per_launch = 2 * s * N * ncols                 # one transform-equivalent per row
            kernels = {}
            # the final column stage only transforms backwards (it observes the field; the spectrum it read stays): half a
            # transform-equivalent per row; every other launch is one
            for name, ms, n, frac_tr in (("row", kt.row_ms, kt.row_n, 1.0), ("col", kt.col_ms, kt.col_n, 1.0),
                                         ("col_H", kt.col_h_ms, kt.col_h_n, 1.0), ("col_ADV", kt.col_adv_ms, kt.col_adv_n, 1.0),
                                         ("col_FIN", kt.col_fin_ms, kt.col_fin_n, 0.5)):
                if n:
                    avg_us = ms / n * 1e3
                    gbs = frac_tr * bytes_per_launch / (avg_us * 1e-6) / 1e9
                    kernels[name] = {"launches": int(n), "avg_us": avg_us, "total_ms": ms,
                                     "algorithmic_bytes_per_launch": frac_tr * bytes_per_launch,
                                     "achieved_GBs": gbs, "frac": gbs / HBM_PEAK_GBS}
            kernels["what"] = {"row": "k_row: convergence decision + FFT.H.IFFT of the rows",
                               "col": "all launches of the Manakov column stage (k_col / k_col_pk: inverse + forward column transforms "
                                      "around the time-domain work), averaged; launches whose stage the state did not ask for included",
                               "col_H": "stage-specialised kernel: half-dispersed field out, first rotation (+ the rare stages)",
                               "col_ADV": "stage-specialised kernel: a non-final iterate -> the next one (phases, convergence sums)",
                               "col_FIN": "stage-specialised kernel: the final iterate, observed and stored (inverse transform only)"}
            kernels["profiled_steps"] = int(stp[u0][1].steps)
            kernels["outlier_launches_left_out"] = int(kt.outliers)   # (events more than 8 x their class median apart: a held-up stream)
            names = [k for k in ("row", "col_H", "col_ADV", "col_FIN") if k in kernels] if "col_ADV" in kernels else [k for k in ("row", "col") if k in kernels]
            if names:                                            # the kernel with the largest share of the device time
                dom = max(names, key=lambda k: kernels[k]["total_ms"])
                tot = sum(kernels[k]["total_ms"] for k in names)
                kernels["dominant"] = {"name": dom, "share_of_kernel_time": kernels[dom]["total_ms"] / tot if tot else None,
                                       "avg_us": kernels[dom]["avg_us"], "achieved_GBs": kernels[dom]["achieved_GBs"],
                                       "frac": kernels[dom]["frac"]}
            rec["roofline"]["kernels"] = kernels
        # measured memory ceiling on this box: a kernel with the row stage's memory shape and no arithmetic
        probe = C.c_double(0.0)
        probe_bytes = max(65536, (2 * s * N) // 65536 * 65536)
        if m.full and lib.ssf_device_copy_bandwidth(local_rank, probe_bytes, 50, C.byref(probe)) == 0:
            rec["roofline"]["measured_copy_GBs"] = probe.value
            rec["roofline"]["frac_of_measured_copy"] = achieved / probe.value
            rec["roofline"]["measured_copy_note"] = ("burst copy kernel, %d MiB read + %d MiB written per launch, no arithmetic"
                                                     % (probe_bytes >> 20, probe_bytes >> 20))
        traffic_file = os.path.join(ROOT, "profiles", "traffic_bytes_per_step.json")
        if os.path.exists(traffic_file) and not m.log2n and not m.prec:
            try:
                t = json.load(open(traffic_file)).get("config%d" % cfg)
                if t and t.get("engine") == _lib.ENGINE_NAMES[st0.engine]:
                    # PMC-measured HBM-side bytes per unit-step (separate rocprofv3 passes, see profiles/), NOT measured in this
                    # run: scaled from the profiled iteration count to this run's (linear in 1 + iterations/step)
                    scale = (1.0 + it_step) / (1.0 + t["iterations_per_step"])
                    rec["roofline"]["traffic"] = t["bytes_per_step"] * scale
                    rec["roofline"]["traffic_profiled"] = t["bytes_per_step"] * scale       # (the key earlier rounds used)
                    rec["roofline"]["traffic_ratio"] = t["bytes_per_step"] * scale / (bytes_local / max(steps_local, 1))
                    rec["roofline"]["traffic_source"] = ("profiles/traffic_bytes_per_step.json[config%d] (%s: rocprofv3 --pmc FETCH_SIZE / "
                                                         "WRITE_SIZE, %d unit-steps at %.2f it/step)"
                                                         % (cfg, t.get("source", "?"), t["steps"], t["iterations_per_step"]))
            except Exception:
                pass

        # ---- parity gate of the run: the CPU oracle (+ cpu_baseline on one GPU), or a reference-generated fixture
        parity = m.parity if m.full else "none"              # (a plain run: the headline figure only)
        if parity == "oracle":
            n = m.cpu_steps or {16: 100, 20: 16, 22: 6}.get(w["log2n"], 8)
            if world > 1:
                n = min(n, 4)
            n = max(2, n)
            E0 = np.ascontiguousarray(fields[u0].T)
            ref, tc, tr = oracle_run(w, E0[:, :1] if w["model"] == "nlse" else E0, n, dtype)
            was_dbp, w["dbp"] = w["dbp"], False
            _lib.raise_for(lib, plans[u0], lib.ssf_upload(plans[u0], dev_in[u0]))
            stp = {}
            run_unit(u0, n, stp)
            w["dbp"] = was_dbp
            got = np.empty_like(fields[u0])
            _lib.raise_for(lib, plans[u0], lib.ssf_download(plans[u0], got.ctypes.data_as(C.c_void_p)))
            got = got[:1] if w["model"] == "nlse" else got
            err = float(np.linalg.norm(got.T.astype(np.complex128) - ref) / np.linalg.norm(ref))
            gate = 1e-10 if s == 16 else 5e-4
            it_gpu, it_cpu = int(stp[u0][1].iterations), int(tr.get("iterations", 0))
            ok = bool(err <= gate) and (s != 16 or it_gpu == it_cpu)
            rec["parity"] = {"rel_l2_vs_oracle": err, "steps": n, "iterations_gpu": it_gpu, "iterations_oracle": it_cpu,
                             "gate": gate, "ok": ok}
            if world == 1 and m.nfields == 1:
                cpu_model = "unknown"
                try:
                    for line in open("/proc/cpuinfo"):
                        if line.startswith("model name"):
                            cpu_model = line.split(":", 1)[1].strip()
                            break
                except OSError:
                    pass
                rec["cpu_baseline"] = {"value": n / tc, "unit": "steps/s", "cores": 1, "kind": "port",
                                       "sample": "%d steps of unit 0's field (numpy oracle, single thread; %d cores available; %s; numpy %s)"
                                                 % (n, os.cpu_count(), cpu_model, np.__version__),
                                       "iterations_per_step": it_cpu / n}
                rec["speedup_vs_cpu"] = rec["value"] / (n / tc)
        elif parity == "fixture_cfg3":
            # tests/golden/wl_cfg3_n22.npz: the REFERENCE on config 3's own field (2^22, seed 3) for six steps, complex128 and
            # complex64 (tools/gen_golden.py cfg3): decimated output + a seeded projection of the whole output
            z = np.load(os.path.join(ROOT, "tests", "golden", "wl_cfg3_n22.npz"))
            fc = json.loads(str(z["cfg"]))
            n, dec, tag = int(fc["steps"]), int(fc["dec"]), "128" if s == 16 else "64"
            _lib.raise_for(lib, plans[u0], lib.ssf_upload(plans[u0], dev_in[u0]))
            stp = {}
            run_unit(u0, n, stp)
            got = np.empty_like(fields[u0])
            _lib.raise_for(lib, plans[u0], lib.ssf_download(plans[u0], got.ctypes.data_as(C.c_void_p)))
            o = got.T.astype(np.complex128)
            ref_dec = z["out128_dec"].astype(np.complex128)
            err = float(np.linalg.norm(o[::dec] - ref_dec) / np.linalg.norm(ref_dec))
            rng = np.random.default_rng(4242)
            r = (rng.normal(size=o.shape[0]) + 1j * rng.normal(size=o.shape[0])) / np.sqrt(2)
            perr = float(np.max(np.abs(o.T @ r - z["out128_proj"])) / np.sqrt(np.sum(z["out128_power"])))
            gate = 1e-10 if s == 16 else 5e-4
            it_gpu, it_ref = int(stp[u0][1].iterations), int(np.sum(z["iters" + tag]))
            ok = bool(err <= gate and perr <= 10 * gate) and it_gpu == it_ref
            rec["parity"] = {"rel_l2_vs_reference_c128": err, "projection_err": perr, "steps": n, "iterations_gpu": it_gpu,
                             "iterations_reference": it_ref, "gate": gate, "ok": ok,
                             "what": "reference-generated fixture tests/golden/wl_cfg3_n22.npz (decimated output + seeded projection)"}
        elif parity == "fixture_units":
            # tests/golden/wl_units45_n20.npz: every unit of configs 4 / 5 through the REFERENCE for eight steps
            z = np.load(os.path.join(ROOT, "tests", "golden", "wl_units45_n%d.npz" % w["log2n"]))
            fc = json.loads(str(z["cfg"]))
            n = int(fc["steps"])
            _dt, sts8 = run_all(n, sync=False)
            worst = 0.0
            its_ok = True
            refc, refit = (z["c5"], z["c5_iterations"].sum(axis=1)) if w["dbp"] else (z["c4"], z["c4_iterations"])
            for u in mine:
                o = np.empty_like(fields[u])
                _lib.raise_for(lib, plans[u], lib.ssf_download(plans[u], o.ctypes.data_as(C.c_void_p)))
                pw, pr = unit_checksum(o)
                worst = max(worst, abs(pw / refc[u][0] - 1.0), abs(pr - abs(complex(refc[u][1], refc[u][2]))) / np.sqrt(refc[u][0]))
                its_ok = its_ok and int(sts8[u].iterations) == int(refit[u])
            ok = bool(worst <= 1e-9) and its_ok
            rec["parity"] = {"worst_unit_checksum_err": worst, "units": len(mine), "steps": n, "iterations_match": its_ok,
                             "gate": 1e-9, "ok": ok,
                             "what": "every unit's (sum |E|^2, |<q,E>|, iterations) against the reference-generated fixture wl_units45"}
        if not ok:
            rec["value"] = None                              # a wrong result is not a benchmark result
    for h in plans.values():
        lib.ssf_plan_destroy(h)
    for q in ([] if host_in else dev_in.values()):
        lib.ssf_device_free(local_rank, q)
    return rec, ok


DUMP_LIMIT_BYTES = 64_000_000                                   # all of DIR, .npy headers included


def dump_outputs(d, outs, n_units, seed=4242):
    """--dump-outputs DIR: what the timed path returned in its last step, one DIR/unit<u>.npy per unit of this rank: the (rows, N)
    complex field as float64 / float32 (rows, N, 2) pairs [real, imag].  Everything when all n_units fit in 64 MB; otherwise the
    same fixed, seeded, sorted sample of sample positions in every unit (DIR/sample_index.npy, float64), sized to the budget."""
    os.makedirs(d, exist_ok=True)
    o0 = next(iter(outs.values()))
    rows, N = o0.shape
    per_sample = rows * o0.itemsize                             # bytes of one sample position (all rows, real + imaginary)
    keep = min(N, (DUMP_LIMIT_BYTES - 4096 * (n_units + 1)) // (per_sample * max(1, n_units) + 8))
    idx = None
    if keep < N:
        idx = np.sort(np.random.default_rng(seed).choice(N, size=keep, replace=False))
        np.save(os.path.join(d, "sample_index.npy"), idx.astype(np.float64))
    for u, o in outs.items():
        a = o if idx is None else o[:, idx]
        np.save(os.path.join(d, "unit%d.npy" % u), np.ascontiguousarray(a).view(a.real.dtype).reshape(a.shape + (2,)))


def also_configs(env, args):
    """The other single-GPU configurations BASELINE.json names, measured in the same run after the headline (VERDICT round 3,
    item 3): each with its own short parity gate, reported under one extra key.  Budget: about a minute."""
    out = {}

    def leg(key, cfg, **kw):
        m = argparse.Namespace(**vars(args))
        m.nfields, m.parity, m.log2n, m.prec, m.cpu_steps, m.no_kernel_times = 1, "oracle", 0, "", 0, False
        m.dump_outputs = None                                    # (--dump-outputs: the headline configuration only)
        for k, v in kw.items():
            setattr(m, k, v)
        t0 = time.perf_counter()
        try:
            rec, ok = measure(env, cfg, m)
            rl = rec["roofline"]
            out[key] = {"workload": rec["config"]["workload"], "value": rec["value"], "unit": rec["unit"], "steps": m.steps,
                        "warmup": m.warmup, "ms_per_step": rec["ms_per_step"], "dtype": rec["dtype"],
                        "iterations_per_step": rec["config"]["iterations_per_step"],
                        "roofline_frac": rl["frac"], "achieved_GBs": rl["achieved"],
                        "kernels": {k: {"avg_us": v["avg_us"], "frac": v["frac"]} for k, v in rl.get("kernels", {}).items()
                                    if isinstance(v, dict) and "avg_us" in v},
                        "parity": rec.get("parity"), "wall_s": time.perf_counter() - t0}
        except Exception as e:                                   # an extra leg never takes the headline line down
            out[key] = {"error": "%s: %s" % (type(e).__name__, e)}

    leg("config3", 3, steps=100, warmup=20, parity="fixture_cfg3")
    leg("config2_out_of_cache_2^22", 3, steps=50, warmup=10, prec="c128", parity="fixture_cfg3", samples_c64=True)
    leg("config4_one_gpu_two_lanes", 4, steps=20, warmup=5, parity="fixture_units", no_kernel_times=True)
    leg("config5_one_gpu_two_lanes", 5, steps=20, warmup=5, parity="fixture_units", no_kernel_times=True)
    leg("config1_16_fields_per_launch", 1, steps=100, warmup=20, nfields=16, no_kernel_times=True)
    try:
        out["rx_chain_2^20"] = rx_chain_leg()
    except Exception as e:
        out["rx_chain_2^20"] = {"error": "%s: %s" % (type(e).__name__, e)}
    try:
        out["reference_notebook"] = notebook_leg()
    except Exception as e:
        out["reference_notebook"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


def rx_chain_leg(reps=10):
    """SURVEY.md 8f ranks 1 and 3 behind the channel, device-resident: pdmCoherentReceiver -> firFilter (1024-tap matched filter)
    -> decimate 16 -> 2 -> edc (800 km) on a 2 x 2^20 field that sits in HBM (one upload before, one download after the timed
    region), against the REFERENCE's output of the same chain (tests/golden/wl_rx_chain_n20.npz, tools/gen_golden.py
    rx_chain20).  Algorithmic bytes: every stage reads its input and writes its output once (receiver 48 + 32 B per sample,
    filter 32 + 32, decimation 32 + 4, compensation 4 + 4)."""
    import opticommpy_amd as oa
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import synth_field
    z = np.load(os.path.join(ROOT, "tests", "golden", "wl_rx_chain_n20.npz"))
    c = json.loads(str(z["cfg"]))

    def bag(cls, kw):
        p = cls()
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    N = int(c["synth"][0])
    E = synth_field(*[int(c["synth"][0]), int(c["synth"][1]), int(c["synth"][2]), float(c["synth"][3])])
    lo = oa.basicLaserModel(bag(oa.parameters, c["lo"]))        # (seeded: the reference's own draws)
    pulse = oa.pulseShape(bag(oa.parameters, c["ps"]))
    Ed, Ld = oa.to_device(E), oa.to_device(lo)

    def chain():
        s = oa.pdmCoherentReceiver(Ed, Ld, bag(oa.parameters, c["fe"]), bag(oa.parameters, c["pd"]))
        s = oa.firFilter(pulse, s)
        s = oa.decimate(s, bag(oa.parameters, c["dec"]))
        return oa.edc(s, bag(oa.parameters, c["edc"]))
    def chain1():                                                     # the same four stages as ONE library call (ssf_rx_chain)
        return oa.pdmCoherentReceiverChain(Ed, Ld, bag(oa.parameters, c["fe"]), bag(oa.parameters, c["pd"]), pulse,
                                           bag(oa.parameters, c["dec"]), bag(oa.parameters, c["edc"]))
    d = int(c["d"])
    rng = np.random.default_rng(4242)
    r = None
    res = {}
    for name, fn in (("four_calls", chain), ("one_call", chain1)):
        out = fn().get()                                              # warm-up + the parity check
        if r is None:
            r = (rng.normal(size=out.shape[0]) + 1j * rng.normal(size=out.shape[0])) / np.sqrt(2)
        err = float(np.linalg.norm(out[::d] - z["out_dec"]) / np.linalg.norm(z["out_dec"]))
        perr = float(np.max(np.abs(out.T @ r - z["out_proj"])) / np.sqrt(np.sum(z["out_power"])))
        t0 = time.perf_counter()
        for _ in range(reps):
            o = fn()
        o.get()[:1]                                                   # (the calls are synchronous at return; one small read to be sure)
        res[name] = ((time.perf_counter() - t0) / reps, err, perr)
    dt4 = res["four_calls"][0]
    dt, err, perr = res["one_call"]
    err, perr = max(err, res["four_calls"][1]), max(perr, res["four_calls"][2])
    alg = N * (80 + 64 + 36 + 8)
    return {"workload": "pdmCoherentReceiver (polarisation rotation + delay, ideal photodiodes) -> firFilter 1024 taps -> decimate 16 -> 2 -> "
                        "edc 800 km, 2 x 2^20 complex128 samples resident in HBM; ms_per_chain: the four stages as ONE library call "
                        "(pdmCoherentReceiverChain / ssf_rx_chain), ms_per_chain_four_calls: the reference's four functions one after the other",
            "ms_per_chain": dt * 1e3, "ms_per_chain_four_calls": dt4 * 1e3, "samples_per_s": N / dt,
            "algorithmic_bytes": alg, "achieved_GBs": alg / dt / 1e9, "roofline_frac": alg / dt / 1e9 / HBM_PEAK_GBS, "reps": reps,
            "parity": {"rel_l2_vs_reference": err, "projection_err": perr, "gate": 1e-9, "ok": bool(err <= 1e-9 and perr <= 1e-8),
                       "what": "the reference's own output of this chain (reference-generated fixture wl_rx_chain_n20)"}}


NB_SETTLE_S = float(os.environ.get("SSF_BENCH_NB_SLEEP", "0.3"))


def _slow_call_profiler():
    """Diagnostic (SSF_BENCH_PROFILE_SLOW=1): cProfile around a timed call of the notebook leg; the profile is printed to stderr when
    the call took more than three times its device time (round 6: about one run in four shows ~70 ms of host time in ONE of the
    two calls at 200 000 samples)."""
    if not os.environ.get("SSF_BENCH_PROFILE_SLOW"):
        return lambda *a: None
    import cProfile
    import io
    import pstats
    pr = cProfile.Profile()
    pr.enable()

    def done(what, N, wall, lr):
        pr.disable()
        if wall * 1e3 > 3.0 * float(lr.get("device_ms", 0.0)) + 5.0:
            buf = io.StringIO()
            pstats.Stats(pr, stream=buf).sort_stats("tottime").print_stats(12)
            print("[notebook leg] slow %s call at N = %d: %.1f ms wall, %.1f ms device\n%s" % (what, N, wall * 1e3, float(lr.get("device_ms", 0.0)),
                                                                                         buf.getvalue()), file=sys.stderr)
    return done


def notebook_leg(sizes=(200_000, 800_000, 2_000_000), sample_km=12.0):
    """The reference's own published GPU benchmark (/root/reference/examples/benchmarck_GPU_processing.ipynb cells 8 - 10:
    `manakovSSF_GPU(sigWDM_Tx, paramCh)` timed with time.time() around the call, numpy in / numpy out): one 16-QAM channel,
    2 polarisations, RRC 4096 taps, SpS 4 at 32 GBd (Fs = 128 GS/s), -2 dBm, Ltotal 500 / Lspan 50 km, ADAPTIVE step
    (nlprMethod True, maxNlinPhaseRot 2e-2, maxIter 5, tol 1e-5, amp = the default 'edfa'), complex128, signal lengths
    2e5 / 8e5 / 2e6 samples (the notebook's 5e4 / 2e5 / 5e5 symbols; its 17.5 - 25 x over the CPU is quoted for > 1e6 samples).
    Per length: the wall time of the call as the notebook takes it, the same call on DeviceArrays, steps / iterations / pipeline,
    and -- CPU baseline + parity -- the numpy oracle on the first `sample_km` km of the same field with amp='ideal' (a handful of
    adaptive steps; a step's CPU time does not depend on its size) against the package on the same span."""
    import gc
    import opticommpy_amd as oa
    from oracle import ssf_oracle as orc

    def bag(cls, **kw):
        q = cls()
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    legs = {}
    for N in sizes:
        tx = bag(oa.parameters, M=16, Rs=32e9, SpS=4, nBits=int(N), pulseType="rrc", nFilterTaps=4096, pulseRollOff=0.01,
                 powerPerChannel=-2, nChannels=1, Fc=193.1e12, laserLinewidth=100e3, wdmGridSpacing=37.5e9, nPolModes=2,
                 seed=int(N) % 9973, prgsBar=False)
        sig = oa.simpleWDMTx(tx)[0]
        assert sig.shape == (N, 2), sig.shape

        def ch(**kw):
            return bag(oa.parameters, **dict(dict(Ltotal=500, Lspan=50, alpha=0.2, D=16, gamma=1.3, Fc=193.1e12, hz=0.5, maxIter=5,
                                                  tol=1e-5, nlprMethod=True, maxNlinPhaseRot=2e-2, prgsBar=False, Fs=32e9 * 4, seed=11), **kw))
        oa.manakovSSF(sig, ch(Ltotal=50))                           # plan, kernels, clocks: one span, untimed
        # The host arrays of the earlier legs are freed HERE, and the GPU queue is given a moment afterwards: in about one run of the
        # driver's command in three, the first GPU submission after those frees waited 70 - 80 ms (inside ssf_execute, before the
        # stream reached the spans' first event: device time 10.5 ms as always; polling waits change nothing; with this pause 0 of 8
        # runs -- profiles/r6_final2_notebook_slow_call.txt).  Not part of the call the notebook times.  Best of two calls besides;
        # both times are reported (wall_s_*_each).
        gc.collect()
        time.sleep(NB_SETTLE_S)
        t_np_each, xfer = [], []                                     # xfer: [path, host-side segments in ms] of every timed call (last_run["host_ms"])
        for _ in range(2):
            prof = _slow_call_profiler()
            t0 = time.perf_counter()
            out = oa.manakovSSF(sig, ch())                           # the notebook's timed statement
            t_np_each.append(time.perf_counter() - t0)
            xfer.append(["numpy", {k: round(float(v), 3) for k, v in oa.last_run.get("host_ms", {}).items()}])
            prof("numpy", N, t_np_each[-1], oa.last_run)
        t_np = min(t_np_each)
        lr = dict(oa.last_run)
        sig_d = oa.to_device(sig)
        oa.manakovSSF(sig_d, ch(Ltotal=50))                         # (the device-array path's own first call, untimed like the one above)
        gc.collect()
        time.sleep(NB_SETTLE_S)
        t_dev_each = []
        for _ in range(2):
            prof = _slow_call_profiler()
            t0 = time.perf_counter()
            out_d = oa.manakovSSF(sig_d, ch())
            t_dev_each.append(time.perf_counter() - t0)
            xfer.append(["device", {k: round(float(v), 3) for k, v in oa.last_run.get("host_ms", {}).items()}])
            prof("device", N, t_dev_each[-1], oa.last_run)
        t_dev = min(t_dev_each)
        lr_d = dict(oa.last_run)
        assert out.shape == (N, 2) and np.all(np.isfinite(out)) and isinstance(out_d, oa.DeviceArray)
        # CPU sample + parity on the first kilometres (deterministic amplifier)
        pc = bag(orc.parameters, Ltotal=sample_km, Lspan=sample_km, alpha=0.2, D=16, gamma=1.3, Fc=193.1e12, hz=0.5, maxIter=5,
                 tol=1e-5, nlprMethod=True, maxNlinPhaseRot=2e-2, prgsBar=False, Fs=32e9 * 4, amp="ideal", saveSpanN=[])
        tr = {}
        t0 = time.perf_counter()
        ref = orc.manakovSSF(sig, pc, trace=tr)
        t_cpu = time.perf_counter() - t0
        got = oa.manakovSSF(sig, ch(Ltotal=sample_km, Lspan=sample_km, amp="ideal", saveSpanN=[]), _trace=True)
        it_gpu = [int(x) for x in oa.last_run["iters"]]
        err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        n_cpu = len(tr["iters"])
        cpu_rate = n_cpu / t_cpu
        ok = bool(err <= 1e-10) and it_gpu == [int(x) for x in tr["iters"]]
        steps = int(lr["steps"])
        legs[str(N)] = {
            "samples": int(N), "pipeline": lr.get("pipeline"), "steps": steps, "iterations": int(lr["iterations"]),
            "wall_s_numpy_in_numpy_out": t_np, "steps_per_s_numpy_in_numpy_out": steps / t_np,
            "wall_s_device_resident": t_dev, "steps_per_s_device_resident": int(lr_d["steps"]) / t_dev,
            "timing": "best of two calls, %.1f s after the earlier legs' host arrays were freed" % NB_SETTLE_S, "wall_s_numpy_in_numpy_out_each": t_np_each, "wall_s_device_resident_each": t_dev_each,
            "host_ms_each": xfer,
            "device_ms": float(lr.get("device_ms", 0.0)),
            "algorithmic_GBs": float(lr.get("bytes_algorithmic", 0.0)) / max(float(lr.get("device_ms", 0.0)), 1e-9) / 1e6,
            "cpu_oracle": {"steps_per_s": cpu_rate, "steps": n_cpu, "seconds": t_cpu, "cores": 1,
                           "sample": "first %.0f km of the same field, amp='ideal' (numpy oracle, 1 thread)" % sample_km},
            "speedup_vs_cpu_oracle_per_step": (steps / t_np) / cpu_rate,
            "parity": {"rel_l2_vs_oracle": err, "steps": n_cpu, "iterations_equal": it_gpu == [int(x) for x in tr["iters"]],
                       "gate": 1e-10, "ok": ok}}
        del sig_d, out_d
        oa.models.release_plans()
    return {"workload": "reference notebook benchmarck_GPU_processing.ipynb cell 10: manakovSSF, 1 x 16-QAM channel, 2-pol, Fs 128 GS/s, "
                        "-2 dBm, 10 x 50 km, adaptive step (maxNlinPhaseRot 2e-2, maxIter 5), amp='edfa' (device ASE), complex128",
            "published": "GPU (cupy) 17.5 - 25 x the CPU at > 1e6 samples (Colab; notebook text below cell 13)", "lengths": legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--config", default=os.environ.get("SSF_BENCH_CONFIG", "2"), help="1 | 2 (default) | 3 | 4 | 5")
    ap.add_argument("--log2n", type=int, default=0, help="experiments: override the configuration's length")
    ap.add_argument("--prec", default="", choices=["", "c128", "c64"], help="experiments: override the precision")
    ap.add_argument("--dbp-hz", type=float, default=0.08)
    ap.add_argument("--lanes", type=int, default=int(os.environ.get("SSF_MGPU_LANES", "2")))
    ap.add_argument("--engine", default=os.environ.get("SSF_ENGINE", "auto"))
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run what the headline figure does not need: the parity gate (with the CPU baseline), "
                         "the per-kernel pass, the copy-bandwidth probe and the 'also' legs; the options below down to --parity choose among those")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=0, help="steps of the CPU oracle leg (0: sized for ~10-20 s)")
    ap.add_argument("--no-kernel-times", action="store_true", help="skip the per-kernel HIP-event pass")
    ap.add_argument("--no-also", action="store_true", help="headline configuration only (no 'also' legs)")
    ap.add_argument("--parity", default="", help="parity leg: oracle (default) | fixture_cfg3 | fixture_units | none")
    ap.add_argument("--notebook", action="store_true", help="only the reference notebook's benchmark (notebook_leg), as one JSON line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed (every unit's output field) as DIR/unit<u>.npy")
    args = ap.parse_args()

    if args.notebook:
        print(json.dumps({"reference_notebook": notebook_leg()}), flush=True)
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:       # no launcher: be one (a launcher's environment wins)
        self_launch(args.gpus)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if os.environ.get("SSF_BENCH_DEVICE") == "mod":            # (test knob: more ranks than GPUs -- rank r on device r % count)
        from opticommpy_amd import _lib as _l0
        local_rank = local_rank % max(1, _l0.load().ssf_device_count())
    elif "SSF_BENCH_DEVICE" in os.environ:                     # (test knob: several ranks against one GPU)
        local_rank = int(os.environ["SSF_BENCH_DEVICE"])

    if rank > 0:                                               # only rank 0 reports: nothing of the other ranks (RCCL's
        devnull = os.open(os.devnull, os.O_WRONLY)             # version banner comes through C stdio at exit) may follow
        os.dup2(devnull, 1)                                    # rank 0's JSON line on the launcher's merged stdout
    from opticommpy_amd import _lib, mgpu
    lib = _lib.load()
    if lib.ssf_device_count() <= 0:
        raise SystemExit("bench.py needs a GPU: no HIP device visible (there is no CPU fallback)")

    comm, comm_name = None, "none (single process)"
    if world > 1 or os.environ.get("SSF_BENCH_FORCE_COMM"):    # (the env var exercises the RCCL path on one GPU)
        if os.environ.get("SSF_BENCH_COMM") == "gloo":          # (explicit opt-in, tests: N ranks against one GPU,
            sys.path.insert(0, os.path.join(ROOT, "tests"))     #  which RCCL refuses)
            from comm_gloo import GlooComm
            comm = GlooComm()
            comm_name = "torch.distributed gloo stand-in (SSF_BENCH_COMM=gloo)"
        else:                                                   # RCCL or nothing: a failure here fails the run
            comm = mgpu.RcclComm.from_env(device=local_rank)
            comm_name = "RCCL via libssf_hip.so (ssf_comm_*)"

    env = argparse.Namespace(lib=lib, _lib=_lib, mgpu=mgpu, comm=comm, comm_name=comm_name, rank=rank, world=world, local_rank=local_rank)
    m = argparse.Namespace(**vars(args))
    m.nfields, m.parity = 1, (args.parity or ("none" if args.no_cpu_baseline else "oracle"))
    rec, ok = measure(env, int(args.config), m)
    if rec is not None and args.full and world == 1 and int(args.config) == 2 and not (args.log2n or args.prec or args.no_also):
        rec["also"] = also_configs(env, args)
    if comm is not None:
        flag = comm.allreduce(np.array([0.0 if ok else 1.0]), "max")     # rank 0 arrives after its extra passes
        ok = flag[0] == 0.0
        comm.close()
    if rec is not None:
        # the JSON line is the LAST thing on stdout: RCCL prints a version banner through C stdio, which would
        # otherwise be flushed after it at exit
        try:
            C.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(rec), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
