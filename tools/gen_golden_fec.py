#!/usr/bin/env python3
"""Generate the soft-decision FEC fixtures tests/golden/fec/*.npz (and the ALIST text next to them) by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  As tools/gen_golden_eq.py does, it registers a throw-away ``numba`` stub first (``njit`` = identity,
``prange`` = ``range``, ``numba.typed.List`` = ``list``), and stubs for ``prettytable`` and ``tqdm`` where they are missing:
``sumProductAlgorithm`` and ``minSumAlgorithm`` are then the plain Python loops (0.2 s to 3 s per decode here).  The reference
needs scipy (``decodeLDPC`` takes a ``csr_matrix``); the package and its tests do not.  No bytecode is written.

Decoding fixtures ``ldpc_<case>.npz``, four codewords each, all-zero codeword over BPSK: ``llr = 2 y / sigma^2``,
``y = 1 + sigma randn``, ``sigma^2 = 10^(-snr_dB / 10)``:
    indptr, indices, shape   H as CSR;   n_   rows of llrs (n_ < n: the last n - n_ variables are punctured)
    llrs                     (n_, 4) float64, as handed to decodeLDPC
    out64, bits64, fail64, iter64     the reference's outputLLRs, decodedBits, frameErrors and lastIter with prec = float64
    out32, bits32, fail32, iter32     the same with prec = float32
    self_err                 per codeword, rel-L2 distance between out32 and out64
    amp                      per codeword, rel-L2 change of out64 when every input LLR is perturbed by a relative 4e-16 (random
                             signs), divided by 4e-16
    cfg                      JSON: alg, maxIter, prec (the precision the case is named for), snr_dB, seed, table, numpy version
``ldpc_graph_<table>.npz``: the edge maps check_offsets, var_offsets, var_edge_indices the reference builds at fec.py:388-411,
taken from the locals of its own run, with H's CSR.
``edge_msa_deg1.npz``, ``edge_spa_deg1.npz``: the fields of a decoding fixture but ``amp`` on a seeded irregular m = 12, n = 24 graph
with one check of degree 1 and one variable of degree 0, maxIter 6.  Asserted: the min-sum fixture holds an infinite posterior,
the two precisions agree on frameErrors, lastIter, the NaN positions and the bits elsewhere, codewords fail next to one that
converges after iteration 0.
``llr_<case>.npz``: rxSymb, sigma2, constSymb, bitMap, px and the reference's LLRs.

Conditions asserted here, re-asserted by tests/fec_cases.py:check_conditions, so that no fixture lets a test pass emptily:
amp <= 1e4 for every codeword; the float32 and float64 runs agree on frameErrors, lastIter and every decoded bit; over the set
there are converged and failed codewords and at least two values of lastIter; every case meets what its name promises (`want`
below); the calcLLR main cases are finite everywhere, the underflow case has +-inf and no NaN.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fec.py [case ...]
"""
import importlib.util
import json
import os
import shutil
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
if importlib.util.find_spec("prettytable") is None:
    _pt = types.ModuleType("prettytable")
    _pt.PrettyTable = type("PrettyTable", (), {})
    sys.modules["prettytable"] = _pt
if importlib.util.find_spec("tqdm") is None:
    _tq = types.ModuleType("tqdm")
    _tq.tqdm = lambda it, **k: it
    _tqn = types.ModuleType("tqdm.notebook")
    _tqn.tqdm = _tq.tqdm
    _tq.notebook = _tqn
    sys.modules["tqdm"] = _tq
    sys.modules["tqdm.notebook"] = _tqn
REFERENCE = os.environ.get("OPTICOMMPY_REFERENCE", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "reference"))
sys.path.insert(0, REFERENCE)

import numpy as np  # noqa: E402

import optic.comm.fec as ref_fec  # noqa: E402
import optic.comm.metrics as ref_metrics  # noqa: E402
from optic.comm.modulation import demodulateGray as ref_demod, grayMapping as ref_gray  # noqa: E402
from optic.dsp.core import pnorm as ref_pnorm  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "fec")
ALIST = os.path.join(REFERENCE, "optic", "comm", "ALIST")
MAX_BYTES = 282045          # the cap of tools/gen_golden_cpr.py
PERTURB = 4e-16
NWORDS = 4
TABLES = {"648": "LDPC_IEEE_802.11nD2_648b_R12.txt", "ar4ja": "LDPC_AR4JA_1280b_R45.txt"}
COMMITTED_ALIST = "648"     # the one ALIST text that is committed: data the reference reads

# name: table, n_ (None = n), alg, maxIter, prec the case is named for, snr_dB, first seed, want (what the seed search looks for)
CASES = {
    "msa_648_mixed": dict(table="648", alg="MSA", maxIter=8, prec="float64", snr=2.5, seed=1, want="mixed"),
    "spa_648_mixed": dict(table="648", alg="SPA", maxIter=8, prec="float64", snr=2.5, seed=1, want="mixed"),
    "spa_648_none": dict(table="648", alg="SPA", maxIter=8, prec="float64", snr=1.0, seed=1, want="none"),
    "msa_648_iter25": dict(table="648", alg="MSA", maxIter=25, prec="float64", snr=3.0, seed=1, want="all_differ"),
    "spa_648_iter25": dict(table="648", alg="SPA", maxIter=25, prec="float64", snr=3.0, seed=1, want="all_differ"),
    "spa_ar4ja_punct": dict(table="ar4ja", n_=1280, alg="SPA", maxIter=8, prec="float64", snr=4.5, seed=1, want="any"),
    "msa_ar4ja_punct": dict(table="ar4ja", n_=1280, alg="MSA", maxIter=8, prec="float64", snr=4.5, seed=1, want="any"),
    "msa_648_clip": dict(table="648", alg="MSA", maxIter=8, prec="float64", snr=2.5, seed=1, want="any", clip=True),
    "spa_648_f32": dict(table="648", alg="SPA", maxIter=8, prec="float32", snr=2.5, seed=11, want="mixed"),
}
LLR_CASES = {
    "qam16": dict(M=16, n=3000, snr=12.0, shaping=0.0, dtype="complex128", seed=5),
    "qam64_shaped": dict(M=64, n=2000, snr=12.0, shaping=0.6, dtype="complex64", seed=6),
    "qam16_underflow": dict(M=16, n=96, snr=32.0, shaping=0.0, dtype="complex128", seed=7),
}


class Param:
    pass


def read_table(key):
    return ref_fec.readAlist(os.path.join(ALIST, TABLES[key]))          # scipy csr_matrix


def reference_decode(H, llrs, alg, maxIter, prec):
    """(outputLLRs, decodedBits, frameErrors, lastIter) of the reference's decodeLDPC; lastIter is caught where the reference
    computes and only logs it."""
    caught = {}
    name = "sumProductAlgorithm" if alg == "SPA" else "minSumAlgorithm"
    inner = getattr(ref_fec, name)

    def wrapped(*a, **k):
        r = inner(*a, **k)
        caught["lastIter"] = np.array(r[1])
        return r

    p = Param()
    p.H, p.alg, p.maxIter, p.prec = H, alg, maxIter, np.dtype(prec).type
    keep = llrs.copy()
    setattr(ref_fec, name, wrapped)
    try:
        bits, out, fail = ref_fec.decodeLDPC(llrs, p)
    finally:
        setattr(ref_fec, name, inner)
    assert np.array_equal(llrs, keep)
    assert out.dtype == np.dtype(prec) and bits.dtype == np.int8 and fail.dtype == np.int8 and caught["lastIter"].dtype == np.uint32
    return out, bits, fail, caught["lastIter"]


def reference_edge_maps(H):
    """check_offsets, var_offsets and var_edge_indices as fec.py:388-411 builds them: the locals of a one-iteration run."""
    got = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "minSumAlgorithm":
            for k in ("check_offsets", "var_offsets", "var_edge_indices"):
                got[k] = np.array(frame.f_locals[k])

    p = Param()
    p.H, p.alg, p.maxIter, p.prec = H, "MSA", 1, np.float64
    sys.setprofile(prof)
    try:
        ref_fec.decodeLDPC(np.ones((H.shape[1], 1)), p)
    finally:
        sys.setprofile(None)
    return got


def rel_cols(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=0) / np.linalg.norm(b, axis=0)


def make_llrs(c, n_, seed):
    rng = np.random.default_rng(seed)
    sigma2 = 10 ** (-c["snr"] / 10)
    y = 1 + np.sqrt(sigma2) * rng.normal(size=(n_, NWORDS))
    llrs = 2 * y / sigma2
    if c.get("clip"):                                   # values beyond +-200 and exact zeros, a few dozen of each
        idx = rng.permutation(llrs.size)
        flat = llrs.reshape(-1)
        flat[idx[:40]] *= 60.0
        flat[idx[40:60]] = -250.0
        flat[idx[60:100]] = 0.0
        assert np.sum(np.abs(llrs) > 200) >= 20 and np.sum(llrs == 0) == 40
    return llrs


def meets(want, fail, it, maxIter):
    if want == "mixed":
        return 0 < fail.sum() < len(fail)
    if want == "none":
        return fail.sum() == len(fail)
    if want == "all_differ":
        return fail.sum() == 0 and len(set(it.tolist())) >= 2
    return True


def generate(name):
    c = CASES[name]
    H = read_table(c["table"])
    m, n = H.shape
    n_ = c.get("n_") or n
    for seed in range(c["seed"], c["seed"] + 60):
        llrs = make_llrs(c, n_, seed)
        out64, bits64, fail64, iter64 = reference_decode(H, llrs, c["alg"], c["maxIter"], "float64")
        if meets(c["want"], fail64, iter64, c["maxIter"]):
            break
    else:
        raise SystemExit(f"{name}: no seed in [{c['seed']}, {c['seed'] + 60}) gives '{c['want']}'")
    out32, bits32, fail32, iter32 = reference_decode(H, llrs, c["alg"], c["maxIter"], "float32")
    signs = np.random.default_rng(seed + 1000).integers(0, 2, size=llrs.shape) * 2 - 1
    outp = reference_decode(H, llrs * (1 + PERTURB * signs), c["alg"], c["maxIter"], "float64")[0]
    self_err, amp = rel_cols(out32, out64), rel_cols(outp, out64) / PERTURB
    assert np.all(amp <= 1e4), (name, amp)
    assert np.array_equal(fail32, fail64) and np.array_equal(iter32, iter64) and np.array_equal(bits32, bits64), name
    assert out64.shape == (n_, NWORDS) and np.all(iter64[fail64 == 1] == c["maxIter"] - 1)
    cfg = dict(name=name, table=TABLES[c["table"]], alg=c["alg"], maxIter=c["maxIter"], prec=c["prec"], snr_dB=c["snr"], seed=seed,
               n=int(n), m=int(m), n_=int(n_), want=c["want"], clip=bool(c.get("clip")), numpy=np.__version__)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"ldpc_{name}.npz")
    np.savez_compressed(path, indptr=H.indptr.astype(np.int32), indices=H.indices.astype(np.int32), shape=np.array(H.shape), n_=n_,
                        llrs=llrs, out64=out64, bits64=bits64, fail64=fail64, iter64=iter64, out32=out32, bits32=bits32,
                        fail32=fail32, iter32=iter32, self_err=self_err, amp=amp, cfg=json.dumps(cfg))
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size >> 10} KiB  seed {seed}  frameErrors {fail64.tolist()}  lastIter {iter64.tolist()}  "
          f"self_err {self_err.min():.1e} .. {self_err.max():.1e}  amp {amp.min():.2g} .. {amp.max():.2g}", flush=True)


def generate_graph(key):
    H = read_table(key)
    maps = reference_edge_maps(H)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"ldpc_graph_{key}.npz")
    np.savez_compressed(path, indptr=H.indptr.astype(np.int32), indices=H.indices.astype(np.int32), shape=np.array(H.shape),
                        table=TABLES[key], **maps)
    assert os.path.getsize(path) <= MAX_BYTES
    print(f"graph {key}: {H.shape}, {H.nnz} edges, max degrees {int(np.diff(maps['check_offsets']).max())} / "
          f"{int(np.diff(maps['var_offsets']).max())}", flush=True)
    if key == COMMITTED_ALIST:
        shutil.copyfile(os.path.join(ALIST, TABLES[key]), os.path.join(OUT, TABLES[key]))


def generate_llr(name):
    c = LLR_CASES[name]
    M = c["M"]
    rng = np.random.default_rng(c["seed"])
    const = ref_gray(M, "qam")
    bitMap = ref_demod(const, M, "qam").reshape(-1, int(np.log2(M)))
    px = np.exp(-c["shaping"] * np.abs(ref_pnorm(const)) ** 2)
    px = px / px.sum()
    const = const / np.sqrt(np.sum(np.abs(const) ** 2 * px))
    if np.dtype(c["dtype"]) == np.complex64:
        # (with rxSymb and constSymb both complex64 the reference's arithmetic is single precision: not what the device, which
        #  is double whatever it is given, can be held to 1e-9 against; a complex128 constellation makes the reference widen)
        const = const.astype(np.complex128)
    assert np.result_type(np.dtype(c["dtype"]), const.dtype) == np.complex128
    sigma2 = 10 ** (-c["snr"] / 10)
    tx = const[rng.choice(M, size=c["n"], p=px)]
    rx = (tx + np.sqrt(sigma2 / 2) * (rng.normal(size=c["n"]) + 1j * rng.normal(size=c["n"]))).astype(c["dtype"])
    keep = rx.copy()
    with np.errstate(divide="ignore"):
        llr = ref_metrics.calcLLR(rx, sigma2, const, bitMap, px)
    assert np.array_equal(rx, keep) and llr.dtype == np.float64 and llr.shape == (c["n"] * bitMap.shape[1],)
    if name.endswith("underflow"):
        assert np.any(np.isinf(llr)) and not np.any(np.isnan(llr)), name
    else:
        assert np.all(np.isfinite(llr)), name
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"llr_{name}.npz")
    np.savez_compressed(path, rxSymb=rx, sigma2=sigma2, constSymb=const, bitMap=bitMap, px=px, llr=llr,
                        cfg=json.dumps(dict(c, name=name, numpy=np.__version__)))
    assert os.path.getsize(path) <= MAX_BYTES
    print(f"llr {name}: {os.path.getsize(path) >> 10} KiB  |LLR| up to {np.max(np.abs(llr[np.isfinite(llr)])):.1f}, "
          f"{int(np.sum(np.isinf(llr)))} infinite", flush=True)


EDGE_CASES = {"edge_msa_deg1": "MSA", "edge_spa_deg1": "SPA"}
EDGE_M, EDGE_N, EDGE_MAXITER, EDGE_GRAPH_SEED, EDGE_SIGMA2 = 12, 24, 6, 5, 0.5


def edge_graph():
    """scipy CSR of the m = 12, n = 24 edge graph: check 0 has degree 1 (variable 3, which other checks hold too, so that its infinite
    posterior travels), variable 23 has degree 0, the other checks have 2 .. 6 distinct variables of 0 .. 22 and every one of those
    is in a check."""
    import scipy.sparse
    rng = np.random.default_rng(EDGE_GRAPH_SEED)
    rows = [np.array([3])]
    for d in rng.integers(2, 7, size=EDGE_M - 1):
        rows.append(np.sort(rng.choice(EDGE_N - 1, size=int(d), replace=False)))
    indptr = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    indices = np.concatenate(rows)
    H = scipy.sparse.csr_matrix((np.ones(len(indices), dtype=np.int8), indices, indptr), shape=(EDGE_M, EDGE_N))
    dv = np.bincount(indices, minlength=EDGE_N)
    assert np.diff(indptr).min() == 1 and np.sum(np.diff(indptr) == 1) == 1 and np.sum(dv == 0) == 1 and dv[EDGE_N - 1] == 0 and dv[3] >= 2
    return H


def generate_edge(name):
    """``<name>.npz`` (no ``ldpc_`` prefix: not one of the nine cases): the fields of a decoding fixture but ``amp``, on the
    edge graph.  Min-sum answers the check of degree 1 with an infinite message and gets ``inf - inf`` back, so out64 / out32 hold
    +-inf and may hold NaN; bits32 / bits64 are meaningful where the posterior is not NaN."""
    alg = EDGE_CASES[name]
    H = edge_graph()
    for seed in range(1, 200):
        rng = np.random.default_rng(seed)
        llrs = 2 * (1 + np.sqrt(EDGE_SIGMA2) * rng.normal(size=(EDGE_N, NWORDS))) / EDGE_SIGMA2
        with np.errstate(invalid="ignore"):
            out64, bits64, fail64, iter64 = reference_decode(H, llrs, alg, EDGE_MAXITER, "float64")
            out32, bits32, fail32, iter32 = reference_decode(H, llrs, alg, EDGE_MAXITER, "float32")
        same = np.array_equal(fail32, fail64) and np.array_equal(iter32, iter64) and \
            np.array_equal(bits32[~np.isnan(out64)], bits64[~np.isnan(out64)]) and np.array_equal(np.isnan(out32), np.isnan(out64))
        if same and 0 < fail64.sum() < NWORDS and np.any((fail64 == 0) & (iter64 > 0)):
            break
    else:
        raise SystemExit(f"{name}: no seed gives failed codewords next to one that converges after iteration 0")
    assert np.any(np.isinf(out64)) == (alg == "MSA") and np.any(np.isinf(out32)) == (alg == "MSA"), name
    if alg == "SPA":
        assert np.all(np.isfinite(out64)) and np.all(np.isfinite(out32))
        self_err = rel_cols(out32, out64)
    else:
        self_err = np.zeros(NWORDS)
    cfg = dict(name=name, alg=alg, maxIter=EDGE_MAXITER, prec="float64", sigma2=EDGE_SIGMA2, seed=seed, graph_seed=EDGE_GRAPH_SEED,
               n=EDGE_N, m=EDGE_M, n_=EDGE_N, numpy=np.__version__)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, indptr=H.indptr.astype(np.int32), indices=H.indices.astype(np.int32), shape=np.array(H.shape), n_=EDGE_N,
                        llrs=llrs, out64=out64, bits64=bits64, fail64=fail64, iter64=iter64, out32=out32, bits32=bits32,
                        fail32=fail32, iter32=iter32, self_err=self_err, cfg=json.dumps(cfg))
    assert os.path.getsize(path) <= MAX_BYTES
    print(f"{name}: {os.path.getsize(path)} bytes  seed {seed}  frameErrors {fail64.tolist()}  lastIter {iter64.tolist()}  "
          f"{int(np.sum(np.isinf(out64)))} infinite, {int(np.sum(np.isnan(out64)))} NaN posteriors", flush=True)


def check_set():
    fails, iters = [], []
    for name in CASES:
        z = np.load(os.path.join(OUT, f"ldpc_{name}.npz"))
        fails += z["fail64"].tolist()
        iters += z["iter64"].tolist()
    assert 0 in fails and 1 in fails and len(set(iters)) >= 2


if __name__ == "__main__":
    todo = sys.argv[1:] or [f"graph:{k}" for k in TABLES] + [f"llr:{k}" for k in LLR_CASES] + list(CASES) + list(EDGE_CASES)
    for case in todo:
        if case in EDGE_CASES:
            generate_edge(case)
        elif case.startswith("graph:"):
            generate_graph(case[6:])
        elif case.startswith("llr:"):
            generate_llr(case[4:])
        else:
            generate(case)
    if not sys.argv[1:]:
        check_set()
