#!/usr/bin/env python3
"""Generate the link-metrics fixtures tests/golden/metrics/metrics_*.npz by IMPORTING THE REFERENCE.

Runs only in the build container (needs the reference checkout); never on the GPU box.  As tools/gen_golden.py does, it registers
a throw-away ``numba`` stub first (``njit`` = identity, ``prange`` = range): every ``@njit`` function on this path is a plain
numpy expression.  No bytecode is written.

Each file holds
    rx, tx        the arrays as they are handed to the functions (complex128 / complex64 / float64), shape as in cfg
    cfg           JSON: M, constType, snr_dB, seed, numpy version, demod_scale (re, im), ...
    px            prior probabilities (only for the shaped case)
    BER SER SNR GMI NGMI MI EVM EVM_blind            the reference's results, per mode
    BER_d ... EVM_blind_d                            the same on symbols [100 : n - 100]
    bits          demodulateGray(demod_scale * rx[:, 0]) (rx[0] for a (nModes, n) array), int8
    signalPower, pnorm_den, pnorm_head               signalPower(rx); sqrt(mean |rx|^2); the first 64 values of pnorm(rx)
    const_raw, const_norm, evm_table, Es, H          the reference's derived tables
    min_margin    smallest gap between the nearest and the second-nearest distance of any decision made on received symbols
                  (normalised rx for BER, blind EVM), in units of the raw table (point spacing 2)
    bit_errors    per mode
    clipped_wrong number of LLRs clipped to +-500 with the wrong sign (the clip case must have some)

Conditions asserted here so that the tests cannot pass emptily: >= 20 bit errors per mode, no NaN LLR, min_margin >= 1e-6, and for
the clip case clipped_wrong >= 1 and GMI < log2 M - 0.01.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_metrics.py [case ...]
"""
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
sys.path.insert(0, os.environ.get("OPTICOMMPY_REFERENCE", "/root/reference"))

import numpy as np  # noqa: E402

import optic.comm.metrics as ref_m  # noqa: E402
import optic.comm.modulation as ref_mod  # noqa: E402
from optic.dsp.core import pnorm as ref_pnorm, signalPower as ref_power  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "metrics")
DISCARD = 100
GAIN, PHASE = 0.7, 0.3

# name: (M, constType, snr_dB, log2 n, nModes (0 = 1-D input), extras, seed)
# The seeds are literals: the first eleven are what 1000 + (rank of the name among those eleven) gave when they were generated, and
# a new name must not move them.
CASES = {
    "qam16_12dB": (16, "qam", 12, 12, 2, {}, 1002),
    "qam64_18dB": (64, "qam", 18, 12, 2, {}, 1007),
    "qam256_24dB_1d": (256, "qam", 24, 12, 0, {}, 1006),
    "qpsk_8dB": (4, "psk", 8, 13, 1, {}, 1010),
    "psk8_12dB": (8, "psk", 12, 12, 2, {}, 1001),
    "pam4_12dB": (4, "pam", 12, 12, 2, {}, 1000),
    "qam64_shaped": (64, "qam", 18, 12, 2, {"shaping": 0.03}, 1009),
    "qam16_4modes": (16, "qam", 12, 12, 4, {}, 1003),
    "qam16_transposed": (16, "qam", 12, 12, 2, {"transposed": True}, 1005),
    "qam64_c64": (64, "qam", 18, 12, 2, {"dtype": "complex64"}, 1008),
    "qam16_clip": (16, "qam", 35, 14, 1, {"clip": True}, 1004),
    # label widths 1, 5, 7 and 10.  The SNRs are low enough that no likelihood sum of a high label bit underflows (the nearest
    # point with the other bit is half the constellation away) and that 2^11 symbols hold 20 bit errors.  bpsk_6dB: 6 dB in the
    # in-phase dimension that carries the signal, which is 3 dB against the complex noise drawn here.
    "bpsk_6dB": (2, "psk", 3, 11, 2, {}, 1011),
    "psk32": (32, "psk", 20, 11, 2, {}, 1012),
    "pam128": (128, "pam", 20, 11, 2, {}, 1013),
    "qam1024_1d": (1024, "qam", 24, 11, 0, {}, 1014),
}


def make_case(name):
    M, ct, snr, log2n, modes, extra, seed = CASES[name]
    rng = np.random.default_rng(seed)
    n, cols = 1 << log2n, max(modes, 1)
    const = ref_mod.grayMapping(M, ct)
    px = None
    if "shaping" in extra:
        px = np.exp(-extra["shaping"] * np.abs(const.astype(np.complex128)) ** 2)
        px = px / np.sum(px)
    pu = np.ones(M) / M if px is None else px
    Es = float(np.sum(np.abs(const) ** 2 * pu))
    idx = rng.choice(M, size=(n, cols), p=pu)
    real = ct == "pam"
    wide = np.float64 if real else np.complex128
    tx = const.astype(wide)[idx] / np.sqrt(Es)
    sigma2 = 10 ** (-snr / 10)
    if real:
        noise = rng.normal(size=(n, cols)) * np.sqrt(sigma2)
        chan = GAIN
    else:
        noise = (rng.normal(size=(n, cols)) + 1j * rng.normal(size=(n, cols))) * np.sqrt(sigma2 / 2)
        chan = GAIN * np.exp(1j * PHASE)
    rx = tx + noise
    if extra.get("clip"):
        # three received symbols moved onto the neighbouring constellation point: their clipped LLRs have the wrong sign
        step = 2 / np.sqrt(Es)
        moved = [i for i in range(n) if tx[i, 0].real < 0][:3]
        for i in moved:
            rx[i, 0] = tx[i, 0] + step + noise[i, 0]
    rx = rx * chan
    if modes == 0:
        rx, tx = rx[:, 0].copy(), tx[:, 0].copy()
    if extra.get("transposed"):
        rx, tx = np.ascontiguousarray(rx.T), np.ascontiguousarray(tx.T)
    if "dtype" in extra:
        rx, tx = rx.astype(extra["dtype"]), tx.astype(extra["dtype"])
    return dict(M=M, constType=ct, snr_dB=snr, seed=seed, px=px, rx=rx, tx=tx, Es=Es, chan=chan, clip=bool(extra.get("clip")),
                transposed=bool(extra.get("transposed")))


def columns(x):
    x = np.asarray(x)
    if x.ndim == 1:
        return x.reshape(-1, 1)
    return x.T if x.shape[1] > x.shape[0] else x


def reference_results(rx, tx, M, ct, px):
    """All functions on widened copies (the reference's GMI / MI write into their arguments)."""
    wide = np.complex128 if np.iscomplexobj(rx) else np.float64
    c = lambda a: np.array(a, dtype=wide, copy=True)   # noqa: E731
    kw = {} if px is None else {"px": px}
    BER, SER, SNR = ref_m.fastBERcalc(c(rx), c(tx), M, ct, **kw)
    GMI, NGMI = ref_m.monteCarloGMI(c(rx), c(tx), M, ct, **kw)
    MI = ref_m.monteCarloMI(c(rx), c(tx), M, ct, **kw)
    EVM = ref_m.calcEVM(c(rx), M, ct, symbTx=c(tx))
    EVMb = ref_m.calcEVM(c(rx), M, ct)
    return dict(BER=BER, SER=SER, SNR=SNR, GMI=GMI, NGMI=NGMI, MI=MI, EVM=EVM, EVM_blind=EVMb)


def conditions(rx, tx, M, ct, px, Es):
    """min_margin, bit errors per mode, NaN / clipped-wrong LLR counts, from the reference's own building blocks."""
    wide = np.complex128 if np.iscomplexobj(rx) else np.float64
    rxc, txc = columns(np.array(rx, dtype=wide)), columns(np.array(tx, dtype=wide))
    const = ref_mod.grayMapping(M, ct)
    b = int(np.log2(M))
    pu = np.ones(M) / M if px is None else px
    constN = const / np.sqrt(Es)
    bitMap = ref_mod.demodulateGray(const, M, ct).reshape(-1, b)
    margin, errors, nan_llr, clipped_wrong = np.inf, [], 0, 0

    def gap(symb, table):
        d = np.sort(np.abs(symb[:, None] - table[None, :].astype(wide)), axis=1)
        return float(np.min(d[:, 1] - d[:, 0]))

    for k in range(rxc.shape[1]):
        r, t = rxc[:, k].copy(), txc[:, k].copy()
        if ct in ("qam", "psk"):
            r = np.mean(t / r) * r
        r, t = ref_pnorm(r), ref_pnorm(t)
        margin = min(margin, gap(np.sqrt(Es) * r, const))
        brx = ref_mod.demodulateGray(np.sqrt(Es) * r, M, ct)
        btx = ref_mod.demodulateGray(np.sqrt(Es) * t, M, ct)
        errors.append(int(np.sum(brx != btx)))
        llr = ref_m.calcLLR(r, np.var(r - t), constN, bitMap, pu)
        nan_llr += int(np.sum(np.isnan(llr)))
        clipped_wrong += int(np.sum((llr == np.inf) & (btx == 1)) + np.sum((llr == -np.inf) & (btx == 0)))
    # blind EVM decides pnorm(symb) (joint over the modes) against pnorm(table); gap rescaled to raw-table units
    table = ref_pnorm(const)
    scale = float(np.abs(const[0]) / np.abs(table[0]))
    joint = ref_pnorm(np.array(rx, dtype=wide))
    for k in range(rxc.shape[1]):
        margin = min(margin, scale * gap(columns(joint)[:, k], table))
    return margin, errors, nan_llr, clipped_wrong


def generate(name):
    c = make_case(name)
    rx, tx, M, ct, px, Es = c["rx"], c["tx"], c["M"], c["constType"], c["px"], c["Es"]
    res = reference_results(rx, tx, M, ct, px)
    cut = (lambda a: a[:, DISCARD:-DISCARD]) if c["transposed"] else (lambda a: a[DISCARD:-DISCARD])
    res_d = reference_results(cut(rx), cut(tx), M, ct, px)
    margin, errors, nan_llr, clipped_wrong = conditions(rx, tx, M, ct, px, Es)
    margin_d = conditions(cut(rx), cut(tx), M, ct, px, Es)[0]
    margin = min(margin, margin_d)

    assert c["clip"] or min(errors) >= 20, (name, errors)
    assert nan_llr == 0, (name, nan_llr)
    assert margin >= 1e-6, (name, margin)
    if c["clip"]:
        assert clipped_wrong >= 1 and np.all(res["GMI"] < np.log2(M) - 0.01), (name, clipped_wrong, res["GMI"])

    wide = np.complex128 if np.iscomplexobj(rx) else np.float64
    first = np.array(rx[0] if c["transposed"] else columns(rx)[:, 0], dtype=wide)
    demod_scale = np.sqrt(Es) / c["chan"] / np.sqrt(np.mean(np.abs(tx) ** 2))
    bits = ref_mod.demodulateGray(demod_scale * first, M, ct)
    demod_margin = float(np.min(np.diff(np.sort(np.abs((demod_scale * first)[:, None] - ref_mod.grayMapping(M, ct)[None, :].astype(wide)),
                                                axis=1)[:, :2], axis=1)))
    assert demod_margin >= 1e-6, (name, demod_margin)
    rxw = np.array(rx, dtype=wide)
    const = ref_mod.grayMapping(M, ct)
    pu = np.ones(M) / M if px is None else px
    cfg = dict(name=name, M=M, constType=ct, snr_dB=c["snr_dB"], seed=c["seed"], numpy=np.__version__, discard=DISCARD,
               shape=list(rx.shape), dtype=rx.dtype.name, demod_scale=[float(np.real(demod_scale)), float(np.imag(demod_scale))],
               clip=c["clip"], shaped=px is not None)
    out = dict(rx=rx, tx=tx, cfg=json.dumps(cfg), bits=bits.astype(np.int8), signalPower=ref_power(rxw),
               pnorm_den=np.sqrt(np.mean(rxw * np.conj(rxw)).real), pnorm_head=ref_pnorm(rxw).reshape(-1)[:64],
               const_raw=const, const_norm=const / np.sqrt(Es), evm_table=ref_pnorm(const), Es=Es, H=float(np.sum(-pu * np.log2(pu))),
               min_margin=margin, bit_errors=np.array(errors), clipped_wrong=clipped_wrong)
    if px is not None:
        out["px"] = px
    out.update(res)
    out.update({k + "_d": v for k, v in res_d.items()})
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"metrics_{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 512 * 1024, (name, size)
    print(f"{name}: {size >> 10} KiB  BER {res['BER']}  GMI {res['GMI']}  MI {res['MI']}  EVM {res['EVM']} / {res['EVM_blind']}  "
          f"errors {errors}  margin {margin:.2e}  clipped-wrong {clipped_wrong}")


if __name__ == "__main__":
    for case in (sys.argv[1:] or list(CASES)):
        generate(case)
