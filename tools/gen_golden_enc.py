#!/usr/bin/env python3
"""Generate the encoder fixtures tests/golden/enc/*.npz by IMPORTING THE REFERENCE.

Runs only where the reference checkout is (OPTICOMMPY_REFERENCE, by default a directory `reference` next to this repository);
never on the GPU box.  It imports tools/gen_golden_fec.py first, which registers the throw-away ``numba`` stub (``njit`` =
identity, ``prange`` = ``range``): ``gaussElim``, ``triangularize``, ``inverseMatrixGF2`` and the three encoders are then the
plain Python loops (3 s to 40 s per table here).  The reference needs scipy; the package and its tests do not.

Encoder fixtures ``enc_<case>.npz``: five messages each (three random, the all-zero and the all-one message):
    indptr, indices, shape   H as handed to the reference, CSR
    bits                     (k, 5) uint8;   codewords  (n, 5) uint8, the reference's encodeLDPC(bits, param)
    hm_indptr, hm_indices    param.H after the call (CSR), where the reference writes it back
    G_packed, G_shape        param.G after the call, np.packbits along the rows  -- the generator-matrix branches
    colSwaps                 the column permutation par2gen returns              -- the generator-matrix branches
    P1_packed, P1_shape, P2_packed, P2_shape   param.P1, param.P2 after the call -- the triangular branch
    syndrome_weight          per codeword, the weight of Hm c for the (unpunctured) codeword c the reference computed
    cfg                      JSON: mode, n, R, branch ('G', 'P1P2' or 'DVBS2'), seed, table, numpy version
``mod_<case>.npz``: bits, M, constType and the reference's modulateGray symbols.

Conditions asserted here and re-asserted by tests/enc_cases.py:check_conditions: the branch the case is named for was taken;
the syndrome is zero; the parity part of every random codeword is neither all 0 nor all 1; a DVB-S2 graph has an empty row of A.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_enc.py [case ...]
"""
import json
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden_fec as gf  # noqa: E402  (the stubs, REFERENCE, ALIST, MAX_BYTES)

import numpy as np  # noqa: E402
import scipy.sparse  # noqa: E402

import optic.comm.fec as ref_fec  # noqa: E402
from optic.comm.modulation import modulateGray as ref_mod  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "enc")
MAX_BYTES = gf.MAX_BYTES
NRANDOM = 3

# name: mode, n, R, the branch the reference must take, seed;  DVB-S2: a seeded synthetic H = [A | dual diagonal] (m, k, row weight)
CASES = {
    "g_648_r12": dict(mode="IEEE_802.11nD2", n=648, R="1/2", branch="G", seed=1),
    "p_648_r34": dict(mode="IEEE_802.11nD2", n=648, R="3/4", branch="P1P2", seed=2),
    "g_ar4ja_1280": dict(mode="AR4JA", n=1280, R="4/5", branch="G", seed=3),
    "dvbs2_m40_k88": dict(mode="DVBS2", m=40, k=88, weight=5, branch="DVBS2", seed=4),
    "dvbs2_m65_k130": dict(mode="DVBS2", m=65, k=130, weight=7, branch="DVBS2", seed=5),
}
MOD_CASES = {
    "psk2": dict(M=2, constType="psk", n=200, seed=11),         # (the reference's qamConst has no M = 2: BPSK is its 2-point table)
    "qam4": dict(M=4, constType="qam", n=200, seed=12),
    "qam16": dict(M=16, constType="qam", n=300, seed=13),
    "qam64": dict(M=64, constType="qam", n=600, seed=14),
    "qam256": dict(M=256, constType="qam", n=2000, seed=15),
    "psk8": dict(M=8, constType="psk", n=200, seed=16),
    "pam4": dict(M=4, constType="pam", n=200, seed=17),
    "ook": dict(M=4, constType="ook", n=200, seed=18),          # M != 2: the reference takes M = 2
}


class Param:
    pass


def dvbs2_graph(c):
    """H = [A | D] with D the dual diagonal (ones at (i, i) and (i, i - 1)); rows 0, m // 2 and m - 1 of A are empty."""
    rng = np.random.default_rng(c["seed"] + 100)
    m, k = c["m"], c["k"]
    A = np.zeros((m, k), dtype=np.uint8)
    for i in range(m):
        if i not in (0, m // 2, m - 1):
            A[i, rng.choice(k, size=c["weight"], replace=False)] = 1
    D = np.eye(m, dtype=np.uint8)
    D[np.arange(1, m), np.arange(m - 1)] = 1
    return scipy.sparse.csr_matrix(np.hstack((A, D)))


def messages(k, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, size=(k, NRANDOM + 2)).astype(np.uint8)
    bits[:, NRANDOM] = 0
    bits[:, NRANDOM + 1] = 1
    return bits


def packed(M):
    M = np.asarray(M, dtype=np.uint8)
    return np.packbits(M, axis=1), np.array(M.shape)


def generate(name):
    c = CASES[name]
    p = Param()
    p.mode = c["mode"]
    if c["mode"] == "DVBS2":
        p.H = dvbs2_graph(c)
        p.n = p.H.shape[1]
        table = ""
    else:
        p.n, p.R, p.path = c["n"], c["R"], gf.ALIST + os.sep
        table = f"LDPC_{c['mode']}_{c['n']}b_R{c['R'][0]}{c['R'][2]}.txt"
        p.H = ref_fec.readAlist(os.path.join(gf.ALIST, table))
    H0 = p.H.copy()
    m, nH = H0.shape
    k = nH - m
    bits = messages(k, c["seed"])
    keep = bits.copy()
    caught = {}
    inner = ref_fec.par2gen

    def wrapped(H):
        r = inner(H)
        caught["colSwaps"] = np.asarray(r[1])
        return r

    ref_fec.par2gen = wrapped
    try:
        cw = np.asarray(ref_fec.encodeLDPC(bits, p))
    finally:
        ref_fec.par2gen = inner
    assert np.array_equal(bits, keep) and cw.dtype == np.uint8 and cw.shape == (p.n, bits.shape[1]), (name, cw.shape)
    assert np.array_equal(cw[:k], bits), name
    G, P1, P2 = getattr(p, "G", None), getattr(p, "P1", None), getattr(p, "P2", None)
    branch = "DVBS2" if c["mode"] == "DVBS2" else "P1P2" if P1 is not None else "G" if G is not None else "?"
    assert branch == c["branch"], (name, branch)
    Hm = scipy.sparse.csr_matrix(p.H)
    Hm.sort_indices()
    extra = {}
    if branch == "G":
        # the unpunctured codeword, for the syndrome (AR4JA is cropped to n rows)
        full = np.asarray(ref_fec.encoder(np.asarray(G, dtype=np.uint8), bits, True))
        assert np.array_equal(full[:p.n], cw)
        extra["G_packed"], extra["G_shape"] = packed(G)
        extra["colSwaps"] = caught["colSwaps"].astype(np.int32)
    else:
        full = cw
        if branch == "P1P2":
            extra["P1_packed"], extra["P1_shape"] = packed(P1)
            extra["P2_packed"], extra["P2_shape"] = packed(P2)
    syn = (Hm.astype(np.int64) @ full.astype(np.int64)) % 2
    weight = np.asarray(syn.sum(axis=0)).reshape(-1)
    assert np.all(weight == 0), (name, weight)
    par = cw[k:, :NRANDOM]
    assert np.all(par.any(axis=0)) and not np.any(par.all(axis=0)), name
    if branch == "DVBS2":
        assert np.any(np.diff(H0[:, :k].tocsr().indptr) == 0), name
    cfg = dict(name=name, mode=c["mode"], n=int(p.n), R=c.get("R", ""), branch=branch, seed=c["seed"], table=table, k=int(k), m=int(m),
               numpy=np.__version__)
    H0.sort_indices()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"enc_{name}.npz")
    np.savez_compressed(path, indptr=H0.indptr.astype(np.int32), indices=H0.indices.astype(np.int32), shape=np.array(H0.shape),
                        bits=bits, codewords=cw, hm_indptr=Hm.indptr.astype(np.int32), hm_indices=Hm.indices.astype(np.int32),
                        syndrome_weight=weight.astype(np.int64), cfg=json.dumps(cfg), **extra)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(f"{name}: {size >> 10} KiB  branch {branch}  k {k}  m {m}  codeword weights {cw.sum(axis=0).tolist()}", flush=True)


def generate_mod(name):
    c = MOD_CASES[name]
    M = 2 if c["constType"] == "ook" else c["M"]
    b = int(np.log2(M))
    bits = np.random.default_rng(c["seed"]).integers(0, 2, size=c["n"] * b)
    symb = np.asarray(ref_mod(bits, c["M"], c["constType"]))
    assert symb.shape == (c["n"],), (name, symb.shape)
    assert len(np.unique(symb)) == M, name                      # every point of the constellation is drawn
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"mod_{name}.npz")
    np.savez_compressed(path, bits=bits.astype(np.uint8), symbols=symb, cfg=json.dumps(dict(c, name=name, numpy=np.__version__)))
    assert os.path.getsize(path) <= MAX_BYTES
    print(f"mod {name}: {os.path.getsize(path)} bytes  {symb.dtype}", flush=True)


if __name__ == "__main__":
    todo = sys.argv[1:] or [f"mod:{k}" for k in MOD_CASES] + list(CASES)
    for case in todo:
        if case.startswith("mod:"):
            generate_mod(case[4:])
        else:
            generate(case)
