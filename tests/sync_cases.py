"""Shared by the synchronisation tests: the fixtures tests/golden/sync/sync_*.npz (tools/gen_golden_sync.py), the bounds the test
files hold in common and the comparison of a result against recorded or restated decisions.

Bounds: the output equals the reference's (np.array_equal: a permutation, a product with 1, -1, 1j or -1j, a conjugation and a
roll are exact, and numpy's == takes -0.0 for 0.0); delay, swap, rot and conj are equal; corrMatrix is within 1e-9 of its largest
entry, the project's bound for double-precision receiver functions against reference fixtures.  A case qualifies with
margin >= 1e-6 (sync_restatement.decisions): the rounding of a double-precision transform is about 1e-13 at these sizes."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sync")
CASES = sorted(os.path.basename(p)[len("sync_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "sync_*.npz")))
EXPECTED_CASES = ["amp_1d_sps1", "amp_2pol", "amp_3modes_sps3", "amp_duplicate_column", "amp_swapped_c64", "amp_tx_longer", "real_conj",
                  "real_rotations", "real_swapped_quarter_turn"]
CHAIN_CASE = "chain_wdm"      # the notebook chain's record: no rx / tx / out of its own (tests/test_gpu_sync.py)
CORR_REL = 1e-9
MARGIN = 1e-6


def load(name):
    z = np.load(os.path.join(GOLDEN, f"sync_{name}.npz"))
    g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def projection(out, seed=4242):
    """A random projection of a large array, as tests/test_chain.py takes it (tools/gen_golden_sync.py: projection)."""
    rng = np.random.default_rng(seed)
    r = (rng.normal(size=out.shape[0]) + 1j * rng.normal(size=out.shape[0])) / np.sqrt(2)
    return np.asarray(out).astype(np.complex128).T @ r


def check_conditions(g):
    """The fixture cannot pass or fail by rounding (asserted by the generator, re-checked on the stored value)."""
    assert float(g["margin"]) >= MARGIN, (g["cfg"]["name"], float(g["margin"]))


def field(want, k):
    return want[k] if isinstance(want, dict) else getattr(want, k)


def compare(out, info, want_out, want, label, tx=None):
    """out, info of a call against the expected output and decisions (a fixture's dict or the restatement's namespace)."""
    want_out = np.asarray(want_out)
    assert isinstance(out, np.ndarray) and out.shape == want_out.shape and out.dtype == want_out.dtype, (label, out.shape, out.dtype)
    for k in ("delay", "swap", "rot", "conj"):
        got, ref = np.asarray(getattr(info, k)), np.asarray(field(want, k))
        assert got.shape == ref.shape and np.array_equal(got, ref), (label, k, got, ref)
    cm, ref = info.corrMatrix, np.asarray(field(want, "corrMatrix"), dtype=np.float64)
    assert cm.dtype == np.float64 and cm.shape == ref.shape, (label, cm.shape)
    err = float(np.max(np.abs(cm - ref)) / np.max(ref))
    print(f"{label}: corrMatrix error / largest entry {err:.2e}, delay {info.delay.tolist()}, swap {info.swap.tolist()}")
    assert err <= CORR_REL, (label, err)
    assert np.array_equal(out, want_out), (label, "output differs at", int(np.count_nonzero(out != want_out)), "of", out.size)
