#!/usr/bin/env python3
"""Generate the synchronisation fixtures tests/golden/sync/sync_*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_eq.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity), and
one for ``tqdm.notebook`` if that is missing.  No bytecode is written.

Each file holds
    rx, tx        the received signal at SpS samples per symbol and the transmitted symbols, as handed to symbolSync
    out           what the reference returns
    delay, swap, rot, conj, corrMatrix   the decisions the reference took, recovered from the correlations its own
                  scipy.signal.correlate calls returned (the call is wrapped; the reference is not edited): rot is the factor
                  applied to column k, rot[k, swap[k]] of its matrix
    margin        the smallest relative gap over every decision (tests/sync_restatement.py: decisions)
    cfg           JSON: sizes, mode, seed, what was done to every mode, numpy and scipy versions

Synthetic input: 16-QAM symbols of unit power; received mode n is transmitted mode src[n], circularly shifted by shift[n],
conjugated where conj[n] is set and turned by phase[n]; every symbol is repeated SpS times, the samples off the symbol's own
phase attenuated to 0.6; white noise of sigma = 0.05 per quadrature.

Condition asserted here and again by tests/sync_cases.py:check_conditions: margin >= 1e-6.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_sync.py [case ...]
"""
import importlib.util
import json
import os
import sys
import types

sys.dont_write_bytecode = True

_nb = types.ModuleType("numba")


def _identity_decorator(*a, **k):
    if len(a) == 1 and callable(a[0]) and not k:
        return a[0]
    return lambda f: f


_nb.njit = _nb.jit = _identity_decorator
_nb.prange = range
_nb_typed = types.ModuleType("numba.typed")
_nb_typed.List = list
_nb.typed = _nb_typed
sys.modules["numba"] = _nb
sys.modules["numba.typed"] = _nb_typed
if importlib.util.find_spec("tqdm") is None:
    _tq = types.ModuleType("tqdm")
    _tq.tqdm = lambda it, **k: it
    _tqn = types.ModuleType("tqdm.notebook")
    _tqn.tqdm = _tq.tqdm
    _tq.notebook = _tqn
    sys.modules["tqdm"] = _tq
    sys.modules["tqdm.notebook"] = _tqn
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(HERE, "..", "..", "reference")))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import numpy as np  # noqa: E402
import scipy  # noqa: E402

import optic.dsp.core as ref_core  # noqa: E402
from optic.comm.modulation import grayMapping as ref_gray  # noqa: E402

import sync_restatement as sr  # noqa: E402

OUT = os.path.join(HERE, "..", "tests", "golden", "sync")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py
SIGMA = 0.05
OFF_PHASE = 0.6
PI = np.pi

# name: n symbols (n_tx: transmitted, when it differs), modes (0 = 1-D), SpS, mode, and per received mode: src, shift, phase, conj
CASES = {
    "amp_2pol": dict(n=1000, modes=2, SpS=2, mode="amp", src=[0, 1], shift=[5, -17], phase=[0.7, -2.1], conj=[0, 0]),
    "amp_swapped_c64": dict(n=1000, modes=2, SpS=2, mode="amp", src=[1, 0], shift=[9, -4], phase=[1.3, 0.4], conj=[0, 0], tx_dtype="complex64"),
    "amp_1d_sps1": dict(n=4097, modes=0, SpS=1, mode="amp", src=[0], shift=[-123], phase=[2.5], conj=[0]),
    "amp_3modes_sps3": dict(n=600, modes=3, SpS=3, mode="amp", src=[1, 2, 0], shift=[3, -8, 20], phase=[0.3, 1.1, -0.9], conj=[0, 0, 0]),
    "amp_duplicate_column": dict(n=1000, modes=2, SpS=2, mode="amp", src=[0, 0], shift=[6, -11], phase=[0.2, 1.9], conj=[0, 0]),
    "amp_tx_longer": dict(n=700, n_tx=1000, modes=2, SpS=1, mode="amp", src=[0, 1], shift=[-12, 31], phase=[0.9, -0.5], conj=[0, 0]),
    "real_rotations": dict(n=1000, modes=2, SpS=2, mode="real", src=[0, 1], shift=[5, -17], phase=[0.2, PI / 2 + 0.15], conj=[0, 0]),
    "real_conj": dict(n=1000, modes=2, SpS=2, mode="real", src=[0, 1], shift=[7, -3], phase=[PI - 0.1, -PI / 2 + 0.1], conj=[1, 0]),
    "real_swapped_quarter_turn": dict(n=1000, modes=2, SpS=2, mode="real", src=[1, 0], shift=[5, -17], phase=[0.2, PI / 2 + 0.15],
                                      conj=[0, 0]),
}


def make_signal(c, seed):
    rng = np.random.default_rng(seed)
    cols, n, SpS = max(c["modes"], 1), c["n"], c["SpS"]
    n_tx = c.get("n_tx", n)
    table = ref_gray(16, "qam").astype(np.complex128)
    table /= np.sqrt(np.mean(np.abs(table) ** 2))
    tx = table[rng.integers(0, 16, size=(n_tx, cols))]
    sym = np.empty((n, cols), dtype=np.complex128)
    for k in range(cols):
        s = np.roll(tx[:, c["src"][k]], c["shift"][k])[:n]
        if c["conj"][k]:
            s = s.conj()
        sym[:, k] = s * np.exp(1j * c["phase"][k])
    gain = np.full(SpS, OFF_PHASE)
    gain[rng.integers(0, SpS)] = 1.0
    rx = (sym[:, None, :] * gain[None, :, None]).reshape(n * SpS, cols)
    rx = rx + (rng.normal(size=rx.shape) + 1j * rng.normal(size=rx.shape)) * SIGMA
    tx = tx.astype(c.get("tx_dtype", "complex128"))
    if c["modes"] == 0:
        rx, tx = rx[:, 0].copy(), tx[:, 0].copy()
    return rx, tx


def run_reference(rx, tx, SpS, mode):
    """The reference's result and the correlations its scipy calls returned, in call order."""
    corrs = []
    real_correlate = ref_core.signal.correlate

    def recording(*a, **k):
        corrs.append(np.array(real_correlate(*a, **k)))
        return corrs[-1]

    keep_rx, keep_tx = rx.copy(), tx.copy()
    shim = types.SimpleNamespace(**{k: getattr(ref_core.signal, k) for k in dir(ref_core.signal) if not k.startswith("__")})
    shim.correlate = recording
    ref_core.signal, saved = shim, ref_core.signal
    try:
        out = ref_core.symbolSync(rx, tx, SpS, mode)
    finally:
        ref_core.signal = saved
    assert np.array_equal(rx, keep_rx) and np.array_equal(tx, keep_tx)
    return out, corrs


def generate(name):
    c = CASES[name]
    cols = max(c["modes"], 1)
    first = 5000 + 100 * sorted(CASES).index(name)
    for seed in range(first, first + 50):
        rx, tx = make_signal(c, seed)
        out, corrs = run_reference(rx, tx, c["SpS"], c["mode"])
        info = sr.decisions(c["mode"], cols, len(tx), corrs)
        if info.margin >= 1e-6:
            break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 50}) meets margin >= 1e-6 (last {info.margin:.2e})")
    assert out.shape == tx.shape and out.dtype == tx.dtype
    # the recovered decisions reproduce the reference's output exactly
    t2 = tx.reshape(len(tx), cols)[:, info.swap]
    for k in range(cols):
        t2[:, k] = info.rot[k] * t2[:, k]
        if info.conj[k]:
            t2[:, k] = t2[:, k].conj()
        t2[:, k] = np.roll(t2[:, k], -int(info.delay[k]))
    assert np.array_equal(t2.reshape(tx.shape), out), name
    cfg = dict(c, name=name, seed=seed, input1D=c["modes"] == 0, rx_shape=list(rx.shape), tx_shape=list(tx.shape), tx_dtype=tx.dtype.name,
               rx_dtype=rx.dtype.name, sigma=SIGMA, off_phase=OFF_PHASE, numpy=np.__version__, scipy=scipy.__version__)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"sync_{name}.npz")
    np.savez_compressed(path, rx=rx, tx=tx, out=out, delay=info.delay, swap=info.swap, rot=info.rot, conj=info.conj,
                        corrMatrix=info.corrMatrix, margin=info.margin, cfg=json.dumps(cfg))
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size >> 10} KiB  seed {seed}  margin {info.margin:.2e}  delay {info.delay.tolist()}  swap {info.swap.tolist()}  "
          f"rot {info.rot.tolist()}  conj {info.conj.tolist()}", flush=True)


def projection(out, seed=4242):
    """A random projection of a large array (tests/test_chain.py: projection)."""
    rng = np.random.default_rng(seed)
    r = (rng.normal(size=out.shape[0]) + 1j * rng.normal(size=out.shape[0])) / np.sqrt(2)
    return np.asarray(out).astype(np.complex128).T @ r


def generate_chain():
    """The notebook chain's synchronisation: the reference's symbolSync(out, symbTx[:, :, chIndex], 2) on the `out` of
    tests/golden/chain_wdm_240k.npz, the symbols from the reference's simpleWDMTx with that fixture's transmitter settings.
    Holds delay, swap, corrMatrix, margin and a random projection of the aligned symbols, no large array."""
    from optic.models.tx import simpleWDMTx as ref_tx
    from optic.utils import parameters as ref_parameters
    z = np.load(os.path.join(OUT, "..", "chain_wdm_240k.npz"))
    cfg = json.loads(str(z["cfg"]))
    p = ref_parameters()
    for k, v in cfg["tx"].items():
        setattr(p, k, v)
    _, symbTx, _ = ref_tx(p)
    assert np.array_equal(symbTx[:64], z["symb_head"])
    tx = np.ascontiguousarray(symbTx[:, :, cfg["chIndex"]])
    out, corrs = run_reference(z["out"], tx, 2, "amp")
    info = sr.decisions("amp", 2, len(tx), corrs)
    assert info.margin >= 1e-6, info.margin
    path = os.path.join(OUT, "sync_chain_wdm.npz")
    np.savez_compressed(path, delay=info.delay, swap=info.swap, rot=info.rot, conj=info.conj, corrMatrix=info.corrMatrix, margin=info.margin,
                        out_proj=projection(out), out_head=out[:64].copy(),
                        cfg=json.dumps(dict(name="chain_wdm", SpS=2, mode="amp", chIndex=cfg["chIndex"], tx_shape=list(tx.shape),
                                            tx_dtype=tx.dtype.name, numpy=np.__version__, scipy=scipy.__version__)))
    print(f"chain_wdm: {os.path.getsize(path) >> 10} KiB  margin {info.margin:.2e}  delay {info.delay.tolist()}  swap {info.swap.tolist()}  "
          f"tx {tx.dtype}{tx.shape}", flush=True)


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES) + ["chain_wdm"]):
        generate_chain() if case == "chain_wdm" else generate(case)
