#!/usr/bin/env python3
"""Generate the freqShift fixtures tests/golden/array/*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository); never
on the GPU box.  As the other generators do, it registers a throw-away ``numba`` stub first (``njit`` = identity), so that
``optic.dsp.core.freqShift`` runs as the numpy code it is.  No bytecode is written.  Data only; every file stays under MAX_BYTES.

Files (every one carries cfg, a JSON string with deltaF, Fs and the numpy version):
    one_dim     x (4099,) complex128, deltaF > 0; y = freqShift(x, deltaF, Fs)
    two_modes   x (3001, 2) complex128, deltaF < 0; y[:, m] = freqShift(x[:, m], deltaF, Fs) per mode (the reference's own
                broadcasting of (n, 2) against the (n,) phasor does not run)
    far         x (20001,) complex128, deltaF < 0 and large: the last argument of the phasor lies beyond 1e6 rad

Conditions asserted here and re-asserted by tests/test_gpu_array.py, so that no fixture lets a test pass emptily: the shift moves
the signal by more than 1e-3 of its peak; the last argument of `far` exceeds 1e6 rad.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_array.py
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
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "reference")))

import numpy as np  # noqa: E402

import optic.dsp.core as ref_core  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "array")
MAX_BYTES = 1 << 20

CASES = {"one_dim": dict(shape=(4099,), deltaF=2.5e9, Fs=64e9, seed=1),
         "two_modes": dict(shape=(3001, 2), deltaF=-7.25e9, Fs=128e9, seed=2),
         "far": dict(shape=(20001,), deltaF=-31.9e9, Fs=4e9, seed=3)}


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, c in CASES.items():
        rng = np.random.default_rng(c["seed"])
        x = rng.standard_normal(c["shape"]) + 1j * rng.standard_normal(c["shape"])
        if x.ndim == 1:
            y = ref_core.freqShift(x, c["deltaF"], c["Fs"])
        else:
            y = np.stack([ref_core.freqShift(x[:, m].copy(), c["deltaF"], c["Fs"]) for m in range(x.shape[1])], axis=-1)
        assert y.dtype == np.complex128 and y.shape == x.shape
        assert np.max(np.abs(y - x)) > 1e-3 * np.max(np.abs(x))
        last = abs(2 * np.pi * c["deltaF"] * (len(x) - 1) / c["Fs"])
        assert last > (1e6 if name == "far" else 1.0), last
        cfg = dict(deltaF=c["deltaF"], Fs=c["Fs"], numpy=np.__version__, last_argument=last)
        path = os.path.join(OUT, name + ".npz")
        np.savez(path, x=x, y=y, cfg=json.dumps(cfg))
        assert os.path.getsize(path) <= MAX_BYTES, (name, os.path.getsize(path))
        print(f"{name}: {os.path.getsize(path)} bytes, last argument {last:.3e} rad")


if __name__ == "__main__":
    main()
