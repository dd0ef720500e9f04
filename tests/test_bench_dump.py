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
