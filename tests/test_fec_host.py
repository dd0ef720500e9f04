"""The host side of the soft-decision FEC functions, no GPU compute: argument checking (every ValueError comes before the library
is loaded), readAlist, the forms param.H is accepted in, the edge maps against those the reference builds (recorded in
tests/golden/fec/ldpc_graph_*.npz), the graph cache, the orientation flag, and the ABI structs against include/ssf.h."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fec_cases as fc
import opticommpy_amd as oa
from opticommpy_amd import _lib, fec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def small_H():
    return np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1]], dtype=np.uint8)


def test_exports():
    assert oa.decodeLDPC is fec.decodeLDPC and oa.calcLLR is fec.calcLLR and oa.readAlist is fec.readAlist
    for name in ("calcLLR", "decodeLDPC", "readAlist"):
        assert name in oa.__all__


def test_decode_arguments_are_checked_before_the_library_loads(no_library):
    H, x = small_H(), np.ones((6, 2))
    wide = np.ones((2, 70), dtype=np.uint8)                              # a check of degree 70
    tall = np.zeros((70, 3), dtype=np.uint8)
    tall[:, 0] = 1                                                       # a variable of degree 70
    tall[:, 1] = 1
    empty_row = small_H()
    empty_row[1] = 0
    bad = [
        (x, fc.Param(H=None), "H is None"),
        (x, fc.Param(), "H is None"),
        (x, fc.Param(H=H, alg="LAYERED"), "Unsupported algorithm"),
        (x, fc.Param(H=H, prec=np.float16), "prec"),
        (x, fc.Param(H=H, prec=np.complex64), "prec"),
        (x, fc.Param(H=H, maxIter=0), "maxIter"),
        (x, fc.Param(H=H, maxIter=2.5), "maxIter"),
        (np.ones((7, 2)), fc.Param(H=H), "n = 6"),
        (np.ones((70, 1)), fc.Param(H=wide), "check has degree 70"),
        (np.ones((3, 1)), fc.Param(H=tall), "variable has degree 70"),
        (x, fc.Param(H=empty_row), "degree 0"),
        (x, fc.Param(H=H, engine="hbm"), "engine"),
        (x, fc.Param(H=H * 2), "0 and 1"),
        (np.ones(6), fc.Param(H=H), "two dimensions"),
        (np.ones((6, 0)), fc.Param(H=H), "codewords"),
    ]
    for llrs, prm, text in bad:
        with pytest.raises(ValueError, match=text):
            oa.decodeLDPC(llrs, prm)
    with pytest.raises(ValueError, match="n = 6"):
        oa.decodeLDPC(np.ones((2, 7)), fc.Param(H=H), transposed=True)
    # a graph that cannot fit in a workgroup's LDS is refused for engine='lds' only
    big = fc.Csr(np.arange(0, 6 * 20001, 6), np.tile(np.arange(6), 20000) + np.repeat(np.arange(20000) * 2, 6) % 39995, (20000, 40000))
    with pytest.raises(ValueError, match="LDS"):
        oa.decodeLDPC(np.ones((40000, 1)), fc.Param(H=big, engine="lds", prec=np.float64))
    assert fec._prepare(np.ones((40000, 1)), fc.Param(H=big, engine="global"))["E"] == 120000


def test_llr_arguments_are_checked_before_the_library_loads(no_library):
    g = fc.load_llr("qam16")
    rx, s2, c, bm, px = g["rxSymb"], g["sigma2"], g["constSymb"], g["bitMap"], g["px"]
    for args, text in [((rx, s2, c[:12], bm[:12], px[:12]), "power of two"), ((rx, s2, c[:1], bm[:1, :0], px[:1]), "power of two"),
                       ((rx, s2, np.ones(2048), np.zeros((2048, 11)), np.ones(2048)), "power of two"),
                       ((rx, s2, c, bm[:, :3], px), "bitMap has shape"), ((rx, s2, c, bm + 1, px), "0 and 1"),
                       ((rx, s2, c, bm, px[:8]), "px has 8"), ((rx, 0.0, c, bm, px), "variance"), ((rx, -1.0, c, bm, px), "variance"),
                       ((rx.reshape(-1, 2), s2, c, bm, px), "one dimension")]:
        with pytest.raises(ValueError, match=text):
            oa.calcLLR(*args)
    q = fec._prepare_llr(rx.astype(np.complex64), s2, c.reshape(-1, 1), bm, px.reshape(-1, 1))      # the (M, 1) arrays of the docstring
    assert q["M"] == 16 and q["b"] == 4 and q["x"].dtype == np.complex64 and q["table"].shape == (32,)


def test_device_arrays_of_another_type_are_refused(no_library):
    d = object.__new__(oa.DeviceArray)                                  # (no GPU needed: the check is on the type)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (6, 2), np.dtype(np.int32), 0, None, d
    with pytest.raises(TypeError, match="float64 or float32"):
        oa.decodeLDPC(d, fc.Param(H=small_H()))
    g = fc.load_llr("qam16")
    d.shape, d.dtype = (8,), np.dtype(np.float64)
    with pytest.raises(TypeError, match="complex128 or complex64"):
        oa.calcLLR(d, g["sigma2"], g["constSymb"], g["bitMap"], g["px"])


def test_read_alist_gives_the_fixtures_matrix():
    H = oa.readAlist(fc.ALIST_648)
    z = fc.load_graph("648")
    assert H.shape == (324, 648) == tuple(z["shape"]) and H.nnz == 2376
    assert np.array_equal(H.indptr, z["indptr"]) and np.array_equal(H.indices, z["indices"])
    assert H.indptr.dtype == np.int32 and H.indices.dtype == np.int32
    g = fc.load("msa_648_mixed")
    assert np.array_equal(H.indptr, g["indptr"]) and np.array_equal(H.indices, g["indices"])
    assert H.toarray().sum() == 2376


def test_read_alist_reads_as_the_reference_does(tmp_path):
    """n m / max degrees / variable degrees / check degrees / one line per variable, 1-based and zero-padded; blank lines are
    dropped before the lines are counted; the check lines are not read."""
    p = tmp_path / "h.alist"
    p.write_text("6 3\n2 3\n\n2 2 2 1 1 1\n3 3 3\n1 3\n2 1\n3 2\n1 0\n2 0\n0 3\n9 9 9\n9 9 9\n9 9 9\n")
    H = oa.readAlist(str(p))
    assert H.shape == (3, 6) and np.array_equal(H.toarray(), small_H())


def test_every_form_of_H_gives_the_same_graph():
    z = fc.load_graph("648")
    want = fec._prepare(np.ones((648, 1)), fc.Param(H=fc.Csr(z["indptr"], z["indices"], z["shape"])))
    dense = np.zeros((324, 648), dtype=np.uint8)
    dense[np.repeat(np.arange(324), np.diff(z["indptr"])), z["indices"]] = 1
    # rows stored in descending column order, as an unsorted scipy matrix may hold them: the edges are still taken ascending
    rev = np.concatenate([z["indices"][a:b][::-1] for a, b in zip(z["indptr"][:-1], z["indptr"][1:])])
    for H in (oa.readAlist(fc.ALIST_648), dense, dense.astype(np.float64), fc.Csr(z["indptr"], rev, z["shape"])):
        q = fec._prepare(np.ones((648, 1)), fc.Param(H=H))
        assert q["digest"] == want["digest"] and (q["m"], q["n"], q["E"]) == (324, 648, 2376)
        for k, a in want["graph"].items():
            assert np.array_equal(q["graph"][k], a) and q["graph"][k].dtype == np.int32, k


@pytest.mark.parametrize("key", fc.GRAPHS)
def test_edge_maps_are_the_references(key):
    z = fc.load_graph(key)
    g = fec.build_graph(z["indptr"], z["indices"], int(z["shape"][1]))
    assert np.array_equal(g["check_offsets"], z["check_offsets"]) and np.array_equal(g["edge_var"], z["indices"])
    assert np.array_equal(g["var_offsets"], z["var_offsets"]) and np.array_equal(g["var_edge_indices"], z["var_edge_indices"])


def test_defaults_and_orientation():
    g = fc.load("spa_ar4ja_punct")
    q = fec._prepare(g["llrs"], fc.Param(H=fc.H_of(g)))
    p = q["params"]
    assert (p.n_, p.numCodewords, p.maxIter, p.alg, p.prec, p.in_dtype, p.transposed, p.engine, p.sync_every) == (1280, 4, 25, 0, 1, 0, 0, 0, 0)
    assert q["prec"] == np.float32 and q["n"] == 1408
    t = fec._prepare(np.ascontiguousarray(g["llrs"].T, dtype=np.float32), fc.Param(H=fc.H_of(g), alg="MSA", prec=np.float64, engine="global"), True)
    p = t["params"]
    assert (p.n_, p.numCodewords, p.alg, p.prec, p.in_dtype, p.transposed, p.engine) == (1280, 4, 1, 0, 1, 1, 2)
    assert fec._prepare(g["llrs"].astype(np.int64), fc.Param(H=fc.H_of(g)))["llrs"].dtype == np.float64
    assert _lib.fec_lds_bytes(2376, 648, "float64") == (2376 + 74 + 1 + 1296) * 8 + 16 + 656
    assert _lib.fec_lds_bytes(4992, 1408, "float32") <= _lib.FEC_LDS_BUDGET


def test_a_matrix_seen_before_is_not_prepared_again(monkeypatch):
    """The edge maps and the digest of a matrix are found again by comparing its CSR arrays, not by identity: an array changed in
    place is another matrix, and stored zeros are never taken for edges."""
    monkeypatch.setattr(fec, "_SEEN", [])
    z = fc.load_graph("648")
    H = fc.Csr(z["indptr"].copy(), z["indices"].copy(), z["shape"])
    a = fec._code_of(H)
    assert fec._code_of(H) is a and fec._code_of(fc.Csr(z["indptr"].copy(), z["indices"].copy(), z["shape"])) is a
    H.indices[0], H.indices[1] = H.indices[1], H.indices[0]            # the same row, stored unsorted: the same code, prepared anew
    b = fec._code_of(H)
    assert b is not a and b["digest"] == a["digest"]
    H.indices[0] = 5                                                     # another edge
    c = fec._code_of(H)
    assert c["digest"] != a["digest"] and c["graph"]["edge_var"][:2].tolist() == [0, 5]
    H.data = np.ones(H.indices.size)
    H.data[0] = 0                                                        # a stored zero: 2375 edges
    assert fec._code_of(H)["E"] == 2375 and len(fec._SEEN) == 3
    for k in range(20):
        fec._code_of(fc.Csr(np.array([0, 2, 4]), np.array([0, 1 + k, 1 + k, 30]), (2, 40)))
    assert len(fec._SEEN) == fec._SEEN_CAP


def test_graph_cache(monkeypatch):
    """One upload per matrix and device; the least recently used graph goes when the cache is full."""
    made, gone = [], []

    class Lib:
        @staticmethod
        def ssf_ldpc_graph_destroy(h):
            gone.append(h)
            return 0

    monkeypatch.setattr(fec, "_GRAPHS", {})
    monkeypatch.setattr(fec, "_GRAPH_CAP", 2)
    monkeypatch.setattr(fec, "_create_graph", lambda lib, dev, q: made.append((dev, q["digest"])) or len(made))
    qs = [fec._prepare(np.ones((6, 1)), fc.Param(H=np.roll(small_H(), k, axis=1) if k < 2 else np.ones((1, 6)))) for k in range(3)]
    assert len({q["digest"] for q in qs}) == 3
    a = fec._graph_handle(Lib, 0, qs[0])
    assert fec._graph_handle(Lib, 0, qs[0]) == a and len(made) == 1
    assert fec._graph_handle(Lib, 0, fec._prepare(np.ones((6, 3)), fc.Param(H=fec.CSR(*fec._as_csr(small_H())[:2], (3, 6)), alg="MSA"))) == a
    b = fec._graph_handle(Lib, 0, qs[1])
    assert b != a and len(made) == 2 and not gone
    assert fec._graph_handle(Lib, 0, qs[0]) == a                        # a is now the most recent
    c = fec._graph_handle(Lib, 0, qs[2])
    assert gone == [b] and len(made) == 3 and fec.graph_cache_info() == [(0, qs[0]["digest"]), (0, qs[2]["digest"])]
    assert fec._graph_handle(Lib, 1, qs[0]) not in (a, b, c) and gone == [b, a]      # another device: another upload
    fec_release = fec.release_graphs
    monkeypatch.setattr(_lib, "load", lambda: Lib)
    fec_release()
    assert fec.graph_cache_info() == [] and len(gone) == 4


def test_struct_layout_matches_header(tmp_path):
    cls, cname = _lib.LdpcParams, "ssf_ldpc_params"
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));'] + [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'printf("{n} %d\\n", (int){n});' for n in ("SSF_FEC_SPA", "SSF_FEC_MSA", "SSF_FEC_F64", "SSF_FEC_F32", "SSF_FEC_AUTO",
                                                          "SSF_FEC_LDS", "SSF_FEC_GLOBAL")]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"ssf.h\"\nint main(void){" + "".join(lines) + "return 0;}"
    (tmp_path / "layout.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")]).decode().splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert [int(got[k]) for k in ("SSF_FEC_SPA", "SSF_FEC_MSA")] == [_lib.FEC_ALGS["SPA"], _lib.FEC_ALGS["MSA"]]
    assert [int(got[k]) for k in ("SSF_FEC_F64", "SSF_FEC_F32")] == [_lib.FEC_PRECS["float64"], _lib.FEC_PRECS["float32"]]
    assert [int(got[k]) for k in ("SSF_FEC_AUTO", "SSF_FEC_LDS", "SSF_FEC_GLOBAL")] == [_lib.FEC_ENGINES[k] for k in ("auto", "lds", "global")]


def test_kernel_constants_match_the_binding():
    text = open(os.path.join(ROOT, "opticommpy_amd", "csrc", "fec_kernels.h")).read()
    assert f"kMaxDeg = {_lib.FEC_MAX_DEGREE};" in text and "kLdsBudget = 160 * 1024;" in text and _lib.FEC_LDS_BUDGET == 160 * 1024


def test_library_rejects_bad_graphs_and_arguments_without_a_device():
    """The kernels index with the graph arrays unchecked: the library refuses, before it looks for a device, whatever could send
    them out of bounds or two threads to one edge."""
    lib = _lib.load()
    g = fec.build_graph(*fec._as_csr(small_H())[:2], 6)
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731

    def create(m=3, n=6, E=9, **change):
        a = {k: np.array(v) for k, v in g.items()}
        for k, (i, v) in change.items():
            a[k][i] = v
        keep = [np.ascontiguousarray(a[k], dtype=np.int32) for k in ("check_offsets", "edge_var", "var_offsets", "var_edge_indices")]
        h = C.c_void_p()
        rc = lib.ssf_ldpc_graph_create(0, m, n, E, *[ip(k) for k in keep], C.byref(h))
        assert rc != 0 and not h.value
        return rc, lib.ssf_last_error(None).decode()

    for kw, text in [(dict(edge_var=(4, 6)), "edge_var"), (dict(edge_var=(0, -1)), "edge_var"), (dict(check_offsets=(3, 10)), "check_offsets"),
                     (dict(check_offsets=(1, 0)), "check"), (dict(var_offsets=(6, 8)), "var_offsets"), (dict(var_offsets=(2, 1)), "var_"),
                     (dict(var_edge_indices=(0, 9)), "var_edge_indices"), (dict(var_edge_indices=(0, 1)), "var_edge_indices"),
                     (dict(m=0), "positive"), (dict(E=0), "positive")]:
        rc, msg = create(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    assert lib.ssf_ldpc_graph_create(0, 3, 6, 9, None, None, None, None, None) == -1
    assert lib.ssf_ldpc_graph_destroy(None) == 0
    assert lib.ssf_ldpc_decode(0, None, None, None, None, None, None, None) == -1
    one = np.ones(4)
    dp = one.ctypes.data_as(C.POINTER(C.c_double))
    bm = np.zeros(4, dtype=np.int32)
    assert lib.ssf_calc_llr(0, 1, 0, 3, 1.0, dp, ip(bm), dp, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == -1
    assert b"power of two" in lib.ssf_last_error(None)
    assert lib.ssf_calc_llr(0, 1, 0, 2, 0.0, dp, ip(bm), dp, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == -1
    assert lib.ssf_calc_llr(0, 1, 2, 2, 1.0, dp, ip(bm), dp, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == -1
    bm[1] = 2
    assert lib.ssf_calc_llr(0, 1, 0, 2, 1.0, dp, ip(bm), dp, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p)) == -1
    assert b"bitmap" in lib.ssf_last_error(None)
