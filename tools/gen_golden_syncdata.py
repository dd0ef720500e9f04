#!/usr/bin/env python3
"""Generate the syncDataSequences / movingAverage / bert fixtures tests/golden/syncdata/*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_cpr.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity), and one
for ``tqdm.notebook`` if that is missing.  No bytecode is written.

<case>.npz (sync)   rx, tx, the reference's tx_ and symb, cfg (JSON: the parameters and what the case is for), and read off
                    tests/syncdata_restatement.py, which is held to the reference's output here: margin (symbolSync's decision
                    margin as tests/sync_restatement.decisions defines it), phase_margin, det_gap ('signal'), kept ('symbols'), padL
ma_*.npz            x, N (in cfg), y (the reference's movingAverage)
bert_*.npz          Irx, bits (empty where the reference draws them from ``seed``), BER, Q, errors, id_gap
closed_forms.npz    the reference's Qfunc and theoryBER at a grid of arguments

Every signal is a delayed, repeated, mildly noisy copy of the transmitted waveform, a few thousand samples long.  Conditions asserted
here and re-asserted by tests/syncdata_cases.py:check_conditions, so that no fixture lets a test pass emptily: margin >= 1e-6;
under 'signal' the two largest sampling-phase variances of decimate differ by >= 1e-9 (relative) and every detector decision has
>= 1e-6 between its two nearest points; no sample of bert lies within 1e-9 max |Irx| of Id.  A seed is searched (at most 40) until
the reference alone meets them.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_syncdata.py [case ...]
"""
import importlib.util
import json
import os
import sys
import types
import warnings

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

import optic.comm.metrics as ref_metrics  # noqa: E402
import optic.comm.modulation as ref_mod  # noqa: E402
import optic.dsp.core as ref_core  # noqa: E402
import optic.dsp.synchronization as ref_sync  # noqa: E402
from optic.utils import parameters as ref_parameters  # noqa: E402

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[1:1] = [_ROOT, os.path.join(_ROOT, "tests")]
import syncdata_cases as sc  # noqa: E402
import syncdata_restatement as rs  # noqa: E402

OUT = sc.GOLDEN
MAX_BYTES = 300000          # far below the largest fixture under tests/golden/ (sc.MAX_BYTES)
SIGMA = 0.02

# delay: in samples of rx, well away from half a period; swap / phase: what the channel does to the modes ('real' undoes quarter turns)
SYNC = {
    "pam4_symbols": dict(M=4, constType="pam", modes=0, reference="symbols", syncMode="amp", SpS=4, nTx=500, n_rx=3000, delay=137),
    "pam4_signal": dict(M=4, constType="pam", modes=0, reference="signal", syncMode="amp", SpS=2, nTx=1000, n_rx=3000, delay=311),
    "pam8_symbols_2modes": dict(M=8, constType="pam", modes=2, reference="symbols", syncMode="amp", SpS=2, nTx=700, n_rx=2500, delay=203),
    "qam16_symbols_amp": dict(M=16, constType="qam", modes=2, reference="symbols", syncMode="amp", SpS=2, nTx=600, n_rx=2100, delay=157,
                              swap=[1, 0]),
    "qam16_symbols_real": dict(M=16, constType="qam", modes=2, reference="symbols", syncMode="real", SpS=2, nTx=600, n_rx=2100, delay=157,
                               swap=[1, 0], turns=[1, 2]),
    "qam16_signal_amp": dict(M=16, constType="qam", modes=2, reference="signal", syncMode="amp", SpS=2, nTx=600, n_rx=2100, delay=91,
                             swap=[1, 0]),
    "qam16_signal_real": dict(M=16, constType="qam", modes=2, reference="signal", syncMode="real", SpS=2, nTx=600, n_rx=2100, delay=91,
                              turns=[3, 0]),
    "qam16_c64": dict(M=16, constType="qam", modes=2, reference="symbols", syncMode="amp", SpS=2, nTx=600, n_rx=2100, delay=157,
                      dtype="complex64"),
    "short_rx": dict(M=4, constType="pam", modes=0, reference="symbols", syncMode="amp", SpS=2, nTx=800, n_rx=1100, delay=97),
    "exact_multiple": dict(M=4, constType="pam", modes=0, reference="signal", syncMode="amp", SpS=2, nTx=600, n_rx=2400, delay=171),
    "ook_symbols": dict(M=2, constType="ook", modes=0, reference="symbols", syncMode="amp", SpS=2, nTx=700, n_rx=2000, delay=119),
}
MA = {
    "ma_odd": dict(n=1500, cols=2, N=45, dtype="complex128"),
    "ma_even": dict(n=1500, cols=1, N=500, dtype="float64"),
    "ma_long_window": dict(n=300, cols=3, N=701, dtype="float64"),
}
BERT = {
    "bert_given": dict(n=3000, given=True, seed=123),
    "bert_drawn": dict(n=2500, given=False, seed=77),
}


def _param(c):
    p = ref_parameters()
    p.SpS, p.reference, p.syncMode = c["SpS"], c["reference"], c["syncMode"]
    p.pulseType, p.rollOff, p.nFilterTaps = "rrc", 0.01, 1024
    p.constType, p.M = ("pam" if c["constType"] == "ook" else c["constType"]), c["M"]
    return p


def make_signal(c, seed):
    """(rx, tx): tx the symbols ('symbols') or the shaped waveform at SpS samples per symbol ('signal')."""
    rng = np.random.default_rng(seed)
    cols, SpS = max(c["modes"], 1), c["SpS"]
    if c["constType"] == "ook":
        table = np.array([0.0, 1.0])
    else:
        table = ref_mod.grayMapping(c["M"], c["constType"])
        table = (table / np.sqrt(np.mean(np.abs(table) ** 2))).astype(np.complex128 if c["constType"] != "pam" else np.float64)
    sym = table[rng.integers(0, len(table), size=(c["nTx"], cols))]
    pp = ref_parameters()
    pp.pulseType, pp.SpS, pp.nFilterTaps, pp.rollOff = ("rrc", SpS, 256, 0.1) if c["reference"] == "symbols" else ("nrz", SpS, 256, 0.1)
    pulse = ref_core.pulseShape(pp)
    reps = -(-c["n_rx"] // (c["nTx"] * SpS)) + 1
    wave = ref_core.firFilter(pulse, ref_core.upsample(np.tile(sym, (reps, 1)), SpS))
    tx = sym if c["reference"] == "symbols" else np.ascontiguousarray(wave[:c["nTx"] * SpS])
    if c["reference"] == "signal":             # a periodic waveform: the period's first samples continue its last ones
        wave = ref_core.firFilter(pulse, ref_core.upsample(np.tile(sym, (reps + 2, 1)), SpS))[c["nTx"] * SpS:]
        tx = np.ascontiguousarray(wave[:c["nTx"] * SpS])
    rx = np.roll(wave, c["delay"], axis=0)[:c["n_rx"]]
    rx = rx[:, c.get("swap", list(range(cols)))]
    if "turns" in c:
        rx = rx * (1j ** np.array(c["turns"]))[None, :]
    noise = rng.normal(size=rx.shape) * SIGMA
    if rx.dtype.kind == "c":
        noise = noise + 1j * rng.normal(size=rx.shape) * SIGMA
    rx = rx + noise
    dtype = c.get("dtype")
    if dtype:
        rx, tx = rx.astype(dtype), tx.astype(dtype)
    if c["modes"] == 0:
        rx, tx = rx[:, 0].copy(), tx[:, 0].copy()
    return np.ascontiguousarray(rx), np.ascontiguousarray(tx)


def generate_sync(name):
    c = SYNC[name]
    p = _param(c)
    first = 7000 + 100 * sorted(SYNC).index(name)
    why = ""
    for seed in range(first, first + 40):
        rx, tx = make_signal(c, seed)
        keep_rx, keep_tx = rx.copy(), tx.copy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tx_, symb = ref_sync.syncDataSequences(rx.copy(), tx.copy(), p)
        assert np.array_equal(rx, keep_rx) and np.array_equal(tx, keep_tx)
        r_tx, r_symb, info = sc.restate(rx, tx, p)
        try:
            sc.check_info(info, c["reference"])
        except AssertionError as e:
            why = f"conditions: {e}"
            continue
        break
    else:
        raise SystemExit(f"{name}: no seed in [{first}, {first + 40}) meets the conditions ({why})")
    # the restatement is held to the reference first
    tx_, symb = np.asarray(tx_), np.asarray(symb)
    # (single-precision input: the reference computes in single precision, 6e-8 per rounding through the filter's sum and two norms;
    #  its result is then compared at 1e-6 and the restatement, in double, is what the device is held to at 1e-9)
    ref_tol = 1e-6 if c.get("dtype") == "complex64" else sc.TOL
    e_tx, ok_tx = sc.close(r_tx, tx_.astype(r_tx.dtype), ref_tol)
    e_sy, ok_sy = sc.close(r_symb, symb.astype(r_symb.dtype), ref_tol)
    assert ok_tx and ok_sy, (name, e_tx, e_sy)
    if c["reference"] == "signal":
        assert np.array_equal(r_tx, tx_.astype(r_tx.dtype)), name
    period = len(tx) * (c["SpS"] if c["reference"] == "symbols" else 1)
    cfg = dict(c, name=name, kind="sync", seed=seed, ref_tol=ref_tol, pulseType="rrc", rollOff=0.01, nFilterTaps=1024, constType=p.constType, sigma=SIGMA,
               padded=bool(info.padL > 0), short=bool(period > len(rx)), zeros=bool(np.any(tx == 0)), numpy=np.__version__)
    save(name, cfg, rx=rx, tx=tx, tx_=tx_, symb=symb, margin=info.margin, phase_margin=info.phase_margin, det_gap=info.det_gap,
         kept=np.zeros(0, dtype=np.int64) if info.kept is None else info.kept, padL=info.padL)
    print(f"    seed {seed}  margin {info.margin:.2e}  phase {info.phase_margin:.2e}  gap {info.det_gap:.2e}  padL {info.padL}  kept "
          f"{None if info.kept is None else info.kept.tolist()}  restatement err tx_ {e_tx:.1e} symb {e_sy:.1e}  delay {info.sync.delay.tolist()}", flush=True)


def generate_ma(name):
    c = MA[name]
    rng = np.random.default_rng(8000 + sorted(MA).index(name))
    x = rng.normal(size=(c["n"], c["cols"]))
    if c["dtype"] == "complex128":
        x = x + 1j * rng.normal(size=x.shape)
    if c["cols"] == 1:
        x = x[:, 0].copy()
    y = ref_core.movingAverage(x.copy(), c["N"])
    e, ok = sc.close(rs.moving_average_direct(x, c["N"]), y, 1e-14)
    assert ok and y.shape == x.shape, (name, e)
    save(name, dict(c, name=name, kind="ma", long=c["N"] > c["n"], odd=c["N"] % 2, numpy=np.__version__), x=x, y=y)
    print(f"    restatement err {e:.1e}", flush=True)


def generate_bert(name):
    c = BERT[name]
    for seed in range(c["seed"], c["seed"] + 40):
        rng = np.random.default_rng(9000 + seed)
        if c["given"]:
            bits = rng.integers(0, 2, size=c["n"])
        else:
            np.random.seed(seed)
            bits = np.random.randint(2, size=c["n"])
        Irx = np.where(bits == 1, 1.0, 0.1) + rng.normal(size=c["n"]) * np.where(bits == 1, 0.22, 0.12)
        BER, Q = ref_metrics.bert(Irx.copy(), bits.copy() if c["given"] else None, seed=seed)
        r_ber, r_q, s = rs.bert(Irx, bits)
        if s.id_gap >= sc.ID_GAP and s.errors > 0:
            break
    else:
        raise SystemExit(f"{name}: no seed meets the conditions")
    assert round(BER * c["n"]) == s.errors and abs(Q - r_q) <= 1e-12 * abs(Q), (name, BER, r_ber, Q, r_q)
    save(name, dict(c, name=name, kind="bert", seed=seed, drawn=not c["given"], numpy=np.__version__), Irx=Irx,
         bits=bits.astype(np.int64) if c["given"] else np.zeros(0, dtype=np.int64), BER=BER, Q=Q, errors=s.errors, id_gap=s.id_gap)
    print(f"    seed {seed}  BER {BER:.4f}  Q {Q:.4f}  id_gap {s.id_gap:.1e}", flush=True)


def generate_closed_forms():
    """theoryBER and Qfunc of the reference at a grid of arguments."""
    x = np.array([-3.0, -0.5, 0.0, 0.3, 1.0, 2.5, 6.0])
    EbN0 = np.array([0.0, 4.0, 9.5, 14.0])
    rows = [(M, ct) for ct, Ms in (("qam", (4, 16, 64)), ("psk", (2, 4, 8)), ("pam", (2, 4, 8))) for M in Ms]
    ber = np.array([[ref_metrics.theoryBER(M, e, ct) for e in EbN0] for M, ct in rows])
    save("closed_forms", dict(name="closed_forms", kind="closed", rows=[[M, ct] for M, ct in rows], numpy=np.__version__), x=x,
         Q=np.array([ref_metrics.Qfunc(v) for v in x]), EbN0=EbN0, ber=ber)


def save(name, cfg, **arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, cfg=json.dumps(cfg), **arrays)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES <= sc.MAX_BYTES, (name, size)
    if cfg["kind"] != "closed":
        sc.check_conditions(sc.load(name))
    print(f"{name}: {size >> 10} KiB", flush=True)


if __name__ == "__main__":
    for nm in sys.argv[1:] or list(SYNC) + list(MA) + list(BERT) + ["closed_forms"]:
        if nm == "closed_forms":
            generate_closed_forms()
        else:
            (generate_sync if nm in SYNC else generate_ma if nm in MA else generate_bert)(nm)
