"""bench.py --dump-outputs DIR: what the timed path computed, written as float arrays within 64 MB (a fixed, seeded sample of
sample positions when the whole output is larger), the same from run to run."""
import os
import sys

import numpy as np
import pytest

from test_round3 import _bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _fields(n_units, N, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return {u: (rng.normal(size=(2, N)) + 1j * rng.normal(size=(2, N))).astype(dtype) for u in range(n_units)}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_output_is_written_whole_as_real_imag_pairs(tmp_path):
    outs = _fields(2, 4096, np.complex128)
    bench.dump_outputs(str(tmp_path), outs, 2)
    assert sorted(os.listdir(tmp_path)) == ["unit0.npy", "unit1.npy"]
    for u, o in outs.items():
        a = np.load(tmp_path / ("unit%d.npy" % u))
        assert a.dtype == np.float64 and a.shape == (2, 4096, 2)
        assert np.array_equal(a[..., 0] + 1j * a[..., 1], o)


@pytest.mark.parametrize("n_units,N,dtype,want", [(1, 1 << 22, np.complex64, np.float32), (16, 1 << 20, np.complex128, np.float64)])
def test_large_output_is_a_seeded_sample_within_64_mb(tmp_path, n_units, N, dtype, want):
    outs = _fields(n_units, N, dtype)
    bench.dump_outputs(str(tmp_path / "a"), outs, n_units)
    bench.dump_outputs(str(tmp_path / "b"), outs, n_units)
    assert _size(tmp_path / "a") <= 64_000_000
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "sample_index.npy"))      # fixed sample
    idx = idx.astype(np.int64)
    assert len(idx) < N and np.all(np.diff(idx) > 0)
    for u, o in outs.items():
        a = np.load(tmp_path / "a" / ("unit%d.npy" % u))
        assert a.dtype == want and a.shape == (2, len(idx), 2)
        assert np.array_equal(a[..., 0] + 1j * a[..., 1], o[:, idx])


@pytest.mark.gpu
def test_bench_dumps_the_timed_steps_output_identically_from_run_to_run(tmp_path):
    """Two runs with the same arguments: exactly K timed steps, ms_per_step reported, and bit-equal dumped outputs whose
    checksum is the one the run reports for its unit."""
    recs = []
    for run in ("a", "b"):
        r, rec = _bench(["--steps", "5", "--warmup", "2", "--log2n", "14", "--no-kernel-times", "--no-also",
                         "--dump-outputs", str(tmp_path / run)], timeout=600)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        recs.append(rec)
    for rec in recs:
        assert rec["steps"] == 5 and rec["config"]["unit_steps_total"] == 5 and rec["ms_per_step"] > 0
    a, b = np.load(tmp_path / "a" / "unit0.npy"), np.load(tmp_path / "b" / "unit0.npy")
    assert a.dtype == np.float64 and a.shape == (2, 1 << 14, 2) and np.array_equal(a, b)
    pw, pr = bench.unit_checksum(a[..., 0] + 1j * a[..., 1])
    assert pw == pytest.approx(recs[0]["unit_checksums"][0][0], rel=1e-12)
    assert pr == pytest.approx(recs[0]["unit_checksums"][0][1], rel=1e-12)


@pytest.mark.gpu
def test_a_plain_run_reports_the_headline_only_and_full_adds_the_rest():
    """Without --full: set-up, warm-up, the timed steps and the result line, whose headline keys are there -- no parity leg, no CPU
    baseline, no per-kernel pass, no copy probe, no "also" legs.  With --full (here at 2^14, where no "also" leg runs) they are back
    and the parity gate decides the exit status; the headline keys say the same in both."""
    plain_r, plain = _bench(["--gpus", "1", "--steps", "5", "--warmup", "2", "--log2n", "14"], timeout=600)
    full_r, full = _bench(["--gpus", "1", "--steps", "5", "--warmup", "2", "--log2n", "14", "--full"], timeout=600)
    assert plain_r.returncode == 0, plain_r.stderr.decode(errors="replace")[-2000:]
    assert full_r.returncode == 0, full_r.stderr.decode(errors="replace")[-2000:]
    for rec in (plain, full):
        assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["unit"] == "steps/s" and rec["higher_is_better"] is True
        assert rec["dtype"] == "f64" and rec["steps"] == 5 and rec["warmup"] == 2 and rec["config"]["unit_steps_total"] == 5
        assert rec["value"] == pytest.approx(1e3 / rec["ms_per_step"], rel=1e-9)
    assert plain["metric"] == full["metric"] and plain["unit_checksums"] == full["unit_checksums"]
    for key in ("parity", "cpu_baseline", "speedup_vs_cpu", "also"):
        assert key not in plain, key
    assert "kernels" not in plain["roofline"] and "measured_copy_GBs" not in plain["roofline"]
    assert full["parity"]["ok"] and full["cpu_baseline"]["value"] > 0
    assert full["roofline"]["kernels"]["profiled_steps"] == 5 and full["roofline"]["measured_copy_GBs"] > 0
