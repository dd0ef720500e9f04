"""More than one rank over the product's communicator: RCCL bound inside libssf_hip.so (csrc/comm_rccl.hip).

On any box with two or more GPUs these tests are the first (and then regular) executions of ncclSend / ncclRecv / ncclAllGather / ncclBroadcast / ncclAllReduce
between devices in this project (missing item 1) -- with W = min(devices, 4) ranks, so a box with four or more
GPUs runs the 4-rank shape of the driver's scaling runs; at most four rank processes, so that with the
test process itself no more than five processes hold a GPU (a shared GPU machine allows six).  The single-process entry point
(test_ssf_mgpu_run_on_every_device) still drives up to eight devices.  No SSF_BENCH_DEVICE / SSF_BENCH_COMM overrides: rank r
drives GPU r.  Unit definition: examples/test_NLC_withDBP_WDM_transmission.ipynb:660-675 (one independent field per
launch power); coupling: optic/models/channels.py:394, 517-519.

RCCL refuses two ranks on one device, so on a one-GPU box the same rank shapes meet over the gloo stand-in (tests/comm_gloo.py,
the SSF_BENCH_COMM=gloo / SSF_BENCH_DEVICE=mod switches of bench.py), rank r on device r % count, and only what needs RCCL itself
(the communicator's name, device pointers handed to the collectives, the device-side coupling of the fused pipeline) is left out."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ndev():
    try:
        from opticommpy_amd import _lib
        return int(_lib.load().ssf_device_count())
    except Exception:
        return 0


NDEV = _ndev()
RCCL = NDEV >= 2                                  # RCCL refuses two ranks on one device: one GPU -> the gloo stand-in
pytestmark = pytest.mark.gpu
DEVICES = max(2, min(NDEV, 8))                 # devices of the single-process test: GPUs of the box, at most eight
MAX_RANKS = 4                                     # rank processes: at most four (with the test process, five holding a GPU)
W = min(DEVICES, MAX_RANKS)                       # ranks = GPUs of the box, at most four


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _spawn(script_text, tmp_path, world=None, timeout=900):
    world = world or W
    script = tmp_path / "worker.py"
    script.write_text(script_text)
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ, **({} if RCCL else {"SSF_TEST_COMM": "gloo"}))
        env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SSF_ROOT=ROOT, SSF_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1",
                   SSF_RCCL_ID_FILE=str(tmp_path / "rccl.id"), SSF_RCCL_NONCE="test-%d" % port, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=timeout)
        assert p.returncode == 0, out.decode(errors="replace")[-3000:]


def _comm_env():
    """bench.py's switches for a one-GPU box: every rank on device r % count, over the gloo stand-in."""
    return {} if RCCL else dict(SSF_BENCH_DEVICE="mod", SSF_BENCH_COMM="gloo")


def _check_comm(rec, ranks):
    if RCCL:
        assert rec["comm"].startswith("RCCL") and rec["rccl_ranks"] == ranks
    else:
        assert rec["comm"].startswith("torch.distributed gloo") and rec["rccl_ranks"] == 0


def _rank_counts():
    return sorted({2, W} | ({4} if W >= 4 else set()))


@pytest.mark.parametrize("ranks", _rank_counts())
@pytest.mark.parametrize("cfg,units", [("4", 16), ("5", 8)])
def test_bench_ranks_over_rccl_configs_4_and_5(ranks, cfg, units):
    """bench.py --gpus N --config 4 / 5 as the driver runs them: rccl_ranks == N, rank 0 synthesises and scatters all units
    (ncclSend / ncclRecv), checksums all-gathered (ncclAllGather): every unit is the reference's."""
    from test_round3 import _bench, _check_units_against_the_reference
    r, rec = _bench(["--gpus", str(ranks), "--config", cfg, "--steps", "8", "--warmup", "2", "--log2n", "16", "--no-kernel-times", "--full"],
                    _comm_env())
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    assert rec["n_gpus"] == ranks
    _check_comm(rec, ranks)
    assert rec["config"]["units_total"] == units and rec["config"]["units_per_gpu"] == units // ranks and rec["scaling"] == "strong"
    _check_units_against_the_reference(rec, cfg, 16)
    assert rec["parity"]["ok"] and rec["value"] > 0


@pytest.mark.parametrize("ranks", _rank_counts())
def test_bench_ranks_over_rccl_weak_scaling(ranks):
    from test_round3 import _bench
    r, rec = _bench(["--gpus", str(ranks), "--steps", "6", "--warmup", "2", "--log2n", "16", "--no-kernel-times", "--full"], _comm_env())
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    _check_comm(rec, ranks)
    assert rec["n_gpus"] == ranks and rec["scaling"] == "weak" and len(rec["unit_checksums"]) == ranks
    assert rec["config"]["unit_steps_total"] == 6 * ranks and rec["parity"]["ok"]


SHARDED = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["SSF_ROOT"]); sys.path.insert(0, os.path.join(os.environ["SSF_ROOT"], "tests"))
import opticommpy_amd as oa
from opticommpy_amd import mgpu, models
from helpers import synth_field, make_param
rank, W = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
GLOO = os.environ.get("SSF_TEST_COMM") == "gloo"                  # (one GPU: every rank on it, over the gloo stand-in)
if GLOO:
    from comm_gloo import GlooComm
    from opticommpy_amd import _lib
    oa.set_device(rank % max(1, _lib.load().ssf_device_count()))
    comm = GlooComm()
else:
    oa.set_device(rank)
    comm = mgpu.RcclComm.from_env(device=rank)
assert comm.world == W
comm.barrier()
assert comm.allreduce(np.array([float(rank + 1)]), "sum").tolist() == [W * (W + 1) / 2.0]
assert comm.allreduce(np.array([float(rank)]), "max").tolist() == [W - 1.0]
a = np.arange(4096, dtype=np.complex128) * (1 + 1j)
got = comm.bcast(a.copy() if rank == 0 else np.zeros_like(a), 0)
assert np.array_equal(got, a)
if not GLOO:
    d = oa.to_device(a if rank == 0 else np.zeros_like(a))        # device pointers go to RCCL as they are
    comm.bcast(d, 0)
    assert np.array_equal(d.get(), a)
ag = comm.allgather(np.full(8, float(rank)))
assert all(ag[r].tolist() == [float(r)] * 8 for r in range(W))
# independent units: rank 0 holds everything, inputs are scattered, results gathered on the root
U = 2 * W + 1
cfg = dict(Fs=512e9, Fc=193.1e12, alpha=0.2, D=16, gamma=1.3, maxIter=10, tol=1e-5, prgsBar=False, Ltotal=2, Lspan=1, hz=0.25,
           nlprMethod=False, amp="ideal", saveSpanN=[])
fields = [synth_field(1 << 13, 2, 100 + u, 8.4 - 0.5 * u) for u in range(U)] if rank == 0 else None
outs = mgpu.run_sharded(fields, make_param(oa.parameters, cfg) if rank == 0 else None, comm=comm, root=0, gather="root")
if rank == 0:
    np.save(os.path.join(os.environ["SSF_OUT"], "sharded.npy"), np.stack(outs))
# a coupled K = W batch, one pair per rank (the partial sums / maxima of every rank all-gathered on the plans' streams).
# complex64 FIRST, on fresh plans: the packed-pair core is created inside the first execute and must inherit the
# communicator attached before it (advisor, round 4: the first complex64 coupled call used to run uncoupled)
E = np.concatenate([synth_field(4096, 2, 11 + r, 3.0 + 9.0 * r / max(W - 1, 1)) for r in range(W)], axis=1)
cfgc = dict(cfg, Ltotal=8, Lspan=4, hz=0.5, nlprMethod=True, maxNlinPhaseRot=1e-2)
for call in range(2):
    out32 = mgpu.run_coupled(np.ascontiguousarray(E[:, 2 * rank: 2 * rank + 2]).astype(np.complex64),
                             make_param(oa.parameters, dict(cfgc, prec="complex64")), comm)
    assert (GLOO or models.last_run["pipeline"] == "fused-device") and out32.dtype == np.complex64
    np.save(os.path.join(os.environ["SSF_OUT"], f"steps32_call{call}_rank{rank}.npy"), np.array([models.last_run["steps"], models.last_run["iterations"]]))
np.save(os.path.join(os.environ["SSF_OUT"], f"coupled32_rank{rank}.npy"), out32)
out = mgpu.run_coupled(np.ascontiguousarray(E[:, 2 * rank: 2 * rank + 2]), make_param(oa.parameters, cfgc), comm)
np.save(os.path.join(os.environ["SSF_OUT"], f"coupled_rank{rank}.npy"), out)
np.save(os.path.join(os.environ["SSF_OUT"], f"steps_rank{rank}.npy"), np.array([models.last_run["steps"], models.last_run["iterations"]]))
assert GLOO or models.last_run["pipeline"] == "fused-device"     # device-side coupling (ssf_set_coupling_comm), host out of the loop
# ... and the host-driven engine with the reducer callback (what other lengths and the gloo stand-in use)
oa.set_engine("rocfft")
out_h = mgpu.run_coupled(np.ascontiguousarray(E[:, 2 * rank: 2 * rank + 2]), make_param(oa.parameters, cfgc), comm)
oa.set_engine("auto")
np.save(os.path.join(os.environ["SSF_OUT"], f"coupled_host_rank{rank}.npy"), out_h)
comm.close()
'''


def test_run_sharded_and_run_coupled_over_rccl_on_every_device(tmp_path):
    from helpers import make_param, rel_l2, synth_field
    from oracle import ssf_oracle as orc
    _spawn(SHARDED, tmp_path)
    cfg = dict(Fs=512e9, Fc=193.1e12, alpha=0.2, D=16, gamma=1.3, maxIter=10, tol=1e-5, prgsBar=False, Ltotal=2, Lspan=1, hz=0.25,
               nlprMethod=False, amp="ideal", saveSpanN=[])
    outs = np.load(tmp_path / "sharded.npy")
    assert len(outs) == 2 * W + 1
    for u in range(2 * W + 1):
        ref = orc.manakovSSF(synth_field(1 << 13, 2, 100 + u, 8.4 - 0.5 * u), make_param(orc.parameters, cfg))
        assert rel_l2(outs[u], ref) <= 1e-10, u
    E = np.concatenate([synth_field(4096, 2, 11 + r, 3.0 + 9.0 * r / max(W - 1, 1)) for r in range(W)], axis=1)
    cfgc = dict(cfg, Ltotal=8, Lspan=4, hz=0.5, nlprMethod=True, maxNlinPhaseRot=1e-2)
    tr = {}
    ref = orc.manakovSSF(E, make_param(orc.parameters, cfgc), trace=tr)
    got = np.concatenate([np.load(tmp_path / f"coupled_rank{r}.npy") for r in range(W)], axis=1)
    assert rel_l2(got, ref) <= 1e-10
    got_h = np.concatenate([np.load(tmp_path / f"coupled_host_rank{r}.npy") for r in range(W)], axis=1)
    assert rel_l2(got_h, ref) <= 1e-10
    got32 = np.concatenate([np.load(tmp_path / f"coupled32_rank{r}.npy") for r in range(W)], axis=1)
    assert rel_l2(got32, ref) <= 5e-4
    for r in range(W):
        s = np.load(tmp_path / f"steps_rank{r}.npy")
        assert int(s[0]) == tr["steps"] and int(s[1]) == tr["iterations"]
        for call in range(2):                 # complex64: the first call on a fresh plan is coupled like the second (the single
            s32 = np.load(tmp_path / f"steps32_call{call}_rank{r}.npy")     # call's step count; its iteration total up to a flip)
            assert int(s32[0]) == tr["steps"] and abs(int(s32[1]) - tr["iterations"]) <= 2, (call, r, s32, tr["steps"], tr["iterations"])


def test_ssf_mgpu_run_on_every_device():
    """The single-process entry point (host threads per device inside the library): units over DEVICES device slots (slot d
    on device d % count: every GPU of the box, or two slots on a one-GPU box) are bit-equal to the same units on device 0 alone."""
    from helpers import synth_field
    from opticommpy_amd import _lib, mgpu
    N, U = 1 << 14, 2 * DEVICES + 2
    fields = np.stack([np.ascontiguousarray(synth_field(N, 2, 300 + u, 6.0 + 0.3 * u).T) for u in range(U)])
    cp = _lib.Params()
    cp.model, cp.direction = _lib.MODEL_MANAKOV, 1
    cp.Fs, cp.Fc, cp.alpha, cp.D, cp.gamma = 512e9, 193.1e12, 0.2, 16.0, 1.3
    cp.Lspan, cp.Nspans, cp.hz, cp.maxIter, cp.tol = 1.6, 1, 0.08, 10, 1e-5
    cp.nlprMethod, cp.maxNlinPhaseRot, cp.NF, cp.amp = 0, 2e-2, 4.5, _lib.AMP_IDEAL
    cp.n_save, cp.save_spans = 0, None
    two, st2 = mgpu.run_threads(fields, cp, [d % max(1, NDEV) for d in range(DEVICES)])
    one, st1 = mgpu.run_threads(fields, cp, [0])
    assert np.array_equal(two, one)
    assert [s["iterations"] for s in st2] == [s["iterations"] for s in st1]
