"""Shared by the encoder tests: the fixtures tests/golden/enc/*.npz (tools/gen_golden_enc.py), the conditions every fixture must
meet so that no test passes emptily, the parameter objects the tests hand to ``encodeLDPC``, and the files the emulator
(tests/emu/emu_enc.cpp) reads and writes.  Every comparison in the encoder tests is ``np.array_equal``: the arithmetic is GF(2)
and a table lookup."""
import glob
import json
import os
import subprocess

import numpy as np

from opticommpy_amd import _lib, fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "enc")
CASES = sorted(os.path.basename(p)[len("enc_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "enc_*.npz")))
# name -> the branch of encodeLDPC the reference took
EXPECTED_CASES = {"dvbs2_m40_k88": "DVBS2", "dvbs2_m65_k130": "DVBS2", "g_648_r12": "G", "g_ar4ja_1280": "G", "p_648_r34": "P1P2"}
MOD_CASES = ["ook", "pam4", "psk2", "psk8", "qam16", "qam256", "qam4", "qam64"]
NRANDOM = 3                # the first columns of `bits` are random, then the all-zero and the all-one message


class Param:
    """Stand-in for the reference's parameters object: attributes only."""

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class Csr:
    """What a scipy.sparse.csr_matrix shows of itself to encodeLDPC."""

    def __init__(self, indptr, indices, shape):
        self.indptr, self.indices, self.shape = indptr, indices, (int(shape[0]), int(shape[1]))

    def toarray(self):
        D = np.zeros(self.shape, dtype=np.uint8)
        D[np.repeat(np.arange(self.shape[0]), np.diff(self.indptr)), self.indices] = 1
        return D


_LOADED = {}


def load(name, prefix="enc"):
    """A fixture, read once and shared (nobody writes to it)."""
    key = (prefix, name)
    if key not in _LOADED:
        z = np.load(os.path.join(GOLDEN, f"{prefix}_{name}.npz"))
        g = {k: z[k] for k in z.files}
        g["cfg"] = json.loads(str(g["cfg"]))
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _LOADED[key] = g
    return _LOADED[key]


def load_mod(name):
    return load(name, "mod")


def unpacked(g, key):
    """A matrix stored as ``np.packbits`` along its rows."""
    return np.unpackbits(g[f"{key}_packed"], axis=1, count=int(g[f"{key}_shape"][1]))


def H_of(g):
    return Csr(g["indptr"], g["indices"], g["shape"])


def Hm_of(g):
    return Csr(g["hm_indptr"], g["hm_indices"], g["shape"])


def param(g, **kw):
    """The parameters the reference was given for the fixture (H handed over, as the generator did)."""
    c = g["cfg"]
    p = Param(mode=c["mode"], n=c["n"], H=H_of(g))
    if c["R"]:
        p.R = c["R"]
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check_conditions(g):
    """What the case's name promises, re-asserted on the stored arrays."""
    c = g["cfg"]
    assert c["branch"] == EXPECTED_CASES[c["name"]], c
    bits, cw = g["bits"], g["codewords"]
    m, nH = (int(v) for v in g["shape"])
    k = nH - m
    assert bits.shape == (k, NRANDOM + 2) and cw.shape == (c["n"], NRANDOM + 2) and cw.dtype == np.uint8
    assert not bits[:, NRANDOM].any() and bits[:, NRANDOM + 1].all()
    assert np.array_equal(cw[:k], bits)
    assert not cw[:, NRANDOM].any()                                     # the all-zero message gives the all-zero codeword
    assert np.all(g["syndrome_weight"] == 0)
    par = cw[k:, :NRANDOM]
    assert par.shape[0] >= 1 and np.all(par.any(axis=0)) and not np.any(par.all(axis=0))
    if c["n"] == nH:                                                    # not punctured: the syndrome against Hm, recomputed
        assert not ((Hm_of(g).toarray().astype(np.int64) @ cw.astype(np.int64)) % 2).any()
    else:
        assert c["mode"] == "AR4JA" and c["n"] < nH
    if c["branch"] == "G":
        G = unpacked(g, "G")
        assert G.shape[0] == k and np.array_equal(G[:, :k], np.eye(k, dtype=np.uint8))
        assert sorted(g["colSwaps"].tolist()) == list(range(nH))
    elif c["branch"] == "P1P2":
        assert unpacked(g, "P1").shape[1] == k and unpacked(g, "P2").shape[1] == k
        assert unpacked(g, "P1").shape[0] + unpacked(g, "P2").shape[0] == m
    else:
        A = H_of(g).toarray()[:, :k]
        empty = np.flatnonzero(A.sum(axis=1) == 0)
        assert 0 in empty and m - 1 in empty and len(empty) >= 3       # empty rows of A, the first and the last among them
        D = H_of(g).toarray()[:, k:]
        assert np.array_equal(D, np.eye(m, dtype=np.uint8) + np.eye(m, k=-1, dtype=np.uint8))


def check_mod_conditions(g):
    c = g["cfg"]
    M = 2 if c["constType"] == "ook" else c["M"]
    b = int(np.log2(M))
    assert g["bits"].shape == (c["n"] * b,) and g["symbols"].shape == (c["n"],)
    assert len(np.unique(g["symbols"])) == M                            # every point of the constellation is drawn


# ---- the emulator's files (tests/emu/emu_enc.cpp)
def build_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("emu_enc") / "emu_enc"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "opticommpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "emu_enc.cpp"), "-o", str(exe)])
    return str(exe)


def run_emu_encode(exe, tmp, bits, prm, transposed=False):
    """``encodeLDPC`` with the kernels walked on the CPU: the host side is the package's own (``fec._prepare_encode``)."""
    x = np.ascontiguousarray(bits.T if transposed else bits)
    q = fec._prepare_encode(x, prm, transposed)
    plan = q["plan"]
    rows = plan["m1"] + plan["m2"]
    head = np.array([plan["form"], plan["k"], rows, plan["systematic"], plan["nnz"], q["N"], q["n_out"], int(transposed)], dtype=np.int32)
    with open(tmp / "in.bin", "wb") as f:
        f.write(head.tobytes())
        if plan["form"] == _lib.ENC_DENSE:
            for blk in plan["blocks"]:
                f.write(np.ascontiguousarray(blk).tobytes())
        else:
            f.write(plan["indptr"].tobytes())
            f.write(plan["indices"].tobytes())
        f.write(q["bits"].tobytes())
    subprocess.check_call([exe, "enc", str(tmp / "in.bin"), str(tmp / "out.bin")])
    out = np.fromfile(tmp / "out.bin", dtype=np.uint8)
    out = out.reshape((q["N"], q["n_out"]) if transposed else (q["n_out"], q["N"]))
    return out.T if transposed else out


def run_emu_modulate(exe, tmp, bits, M, constType):
    q = fec._prepare_mod(bits, M, constType)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([q["M"], q["b"]], dtype=np.int32).tobytes())
        f.write(np.array([q["nsymb"]], dtype=np.int64).tobytes())
        f.write(q["table"].tobytes())
        f.write(q["bits"].tobytes())
    subprocess.check_call([exe, "mod", str(tmp / "in.bin"), str(tmp / "out.bin")])
    return np.fromfile(tmp / "out.bin", dtype=np.complex128)
