"""The host side of encodeLDPC and modulateGray without a GPU: the names, every refusal (reached before the library is loaded), the
write-backs of every branch of the reference's encodeLDPC (fec.py:153-251), and the GF(2) helpers par2gen, triangP1P2 and
writeAlist against what the reference made of the same tables (tests/golden/enc, tools/gen_golden_enc.py)."""
import numpy as np
import pytest

import enc_cases as ec
import fec_cases as fc
import opticommpy_amd as oa
from opticommpy_amd import _lib, fec

NEW_NAMES = ["encodeLDPC", "modulateGray", "par2gen", "triangP1P2", "writeAlist"]


@pytest.fixture
def no_library(monkeypatch):
    """Whatever the test does, it does without the library."""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def same_csr(a, indptr, indices, shape):
    return isinstance(a, fec.CSR) and a.shape == tuple(int(s) for s in shape) and np.array_equal(a.indptr, indptr) and \
        np.array_equal(a.indices, indices)


def test_the_new_names_are_exported():
    for name in NEW_NAMES:
        assert callable(getattr(oa, name)) and name in oa.__all__ and name in fec.__all__
        assert getattr(oa, name) is getattr(fec, name)
    for sym in ("ssf_ldpc_encoder_create", "ssf_ldpc_encoder_destroy", "ssf_ldpc_encode", "ssf_modulate"):
        assert sym in _lib.SYMBOLS
    assert _lib.ENC_SPAN == _lib.ENC_BLOCK and _lib.ENC_ROWS == _lib.ENC_BLOCK and _lib.ENC_SPAN % _lib.ENC_WAVE_SPAN == 0


def test_the_fixture_set_is_complete():
    assert ec.CASES == sorted(ec.EXPECTED_CASES)
    for name in ec.CASES:
        ec.check_conditions(ec.load(name))
    for name in ec.MOD_CASES:
        ec.check_mod_conditions(ec.load_mod(name))


def test_encode_refusals(no_library, tmp_path):
    G = np.hstack((np.eye(3, dtype=np.uint8), np.ones((3, 2), dtype=np.uint8)))
    ok = np.zeros((3, 4), dtype=np.uint8)

    def prm(**kw):
        return ec.Param(**dict(dict(mode="AR4JA", n=5, G=G), **kw))

    assert fec._prepare_encode(ok, prm())["n_out"] == 5
    with pytest.raises(ValueError, match="Unsupported mode"):
        oa.encodeLDPC(ok, prm(mode="LDPC"))
    with pytest.raises(ValueError, match="0 and 1"):
        oa.encodeLDPC(ok + 2, prm())
    with pytest.raises(ValueError, match="0 and 1"):
        oa.encodeLDPC(ok.astype(np.int8) - 1, prm())
    with pytest.raises(ValueError, match="integer or bool"):
        oa.encodeLDPC(ok.astype(np.float64), prm())
    with pytest.raises(ValueError, match="two dimensions"):
        oa.encodeLDPC(ok[:, 0], prm())
    with pytest.raises(ValueError, match="k = 3"):
        oa.encodeLDPC(np.zeros((4, 3), dtype=np.uint8), prm())
    with pytest.raises(ValueError, match="k = 3"):
        oa.encodeLDPC(ok, prm(), transposed=True)                       # (N, k) asked for, (k, N) given
    assert fec._prepare_encode(np.ascontiguousarray(ok.T), prm(), True)["N"] == 4
    with pytest.raises(ValueError, match="65535"):
        oa.encodeLDPC(np.zeros((3, 65536), dtype=np.uint8), prm())
    with pytest.raises(ValueError, match="param.H is None"):
        oa.encodeLDPC(ok, prm(G=None))                                  # neither H nor a path
    with pytest.raises(ValueError, match="param.H is None"):
        oa.encodeLDPC(ok, ec.Param(mode="DVBS2", n=5))
    with pytest.raises(FileNotFoundError):
        oa.encodeLDPC(ok, ec.Param(mode="DVBS2", n=5, R="1/2", path=str(tmp_path)))
    with pytest.raises(ValueError, match="0 and 1"):
        oa.encodeLDPC(ok, prm(G=G * 2))
    with pytest.raises(ValueError, match="more columns than rows"):
        oa.encodeLDPC(ok, prm(G=np.eye(3, dtype=np.uint8)))
    with pytest.raises(ValueError, match="message bits"):
        oa.encodeLDPC(ok, ec.Param(mode="DVBS2", n=2, H=np.ones((2, 5), dtype=np.uint8)))          # k = n - m = 0
    big = np.zeros((1, fec.MAX_K_DENSE + 1), dtype=np.uint8)
    with pytest.raises(ValueError, match="at most"):
        oa.encodeLDPC(big, ec.Param(mode="IEEE_802.11nD2", n=9, P1=big, P2=big), transposed=True)
    d = object.__new__(oa.DeviceArray)                                  # (no GPU needed: the check is on the type)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (3, 4), np.dtype(np.int32), 0, None, d
    with pytest.raises(TypeError, match="uint8 or int8"):
        oa.encodeLDPC(d, prm())


def test_modulate_refusals(no_library):
    bits = np.zeros(12, dtype=np.uint8)
    assert fec._prepare_mod(bits, 16, "qam")["nsymb"] == 3
    assert fec._prepare_mod(bits, 64, "ook")["M"] == 2                  # 'ook' with M != 2 becomes M = 2
    for M in (3, 1, 2048, 0):
        with pytest.raises(ValueError, match="power of two"):
            oa.modulateGray(bits, M, "qam")
    with pytest.raises(ValueError, match="constType"):
        oa.modulateGray(bits, 4, "apsk")
    with pytest.raises(ValueError):
        oa.modulateGray(bits, 8, "qam")                                 # no square 8-QAM
    with pytest.raises(ValueError, match="whole number"):
        oa.modulateGray(bits[:11], 16, "qam")
    with pytest.raises(ValueError, match="whole number"):
        oa.modulateGray(bits[:0], 16, "qam")
    with pytest.raises(ValueError, match="one dimension"):
        oa.modulateGray(bits.reshape(3, 4), 16, "qam")
    with pytest.raises(ValueError, match="0 and 1"):
        oa.modulateGray(bits + 3, 16, "qam")
    d = object.__new__(oa.DeviceArray)
    d.shape, d.dtype, d.device, d._ptr, d._owner = (12,), np.dtype(np.int64), 0, None, d
    with pytest.raises(TypeError, match="uint8 or int8"):
        oa.modulateGray(d, 16, "qam")


def test_tables_of_modulate_are_the_mapping_of_the_package(no_library):
    for M, ct in ((4, "qam"), (8, "psk"), (4, "pam"), (1024, "qam")):
        q = fec._prepare_mod(np.zeros(10 * int(np.log2(M)), dtype=np.uint8), M, ct)
        assert np.array_equal(q["table"].view(np.complex128), oa.grayMapping(M, ct).astype(np.complex128))
    assert np.array_equal(fec._prepare_mod(np.zeros(4, dtype=bool), 2, "ook")["table"], [0, 0, 1, 0])


@pytest.mark.parametrize("name", ["g_648_r12", "g_ar4ja_1280"])
def test_generator_branch_writes_G_and_Hm_back(no_library, name):
    g = ec.load(name)
    p = ec.param(g)
    q = fec._prepare_encode(g["bits"], p)
    assert isinstance(p.G, np.ndarray) and p.G.dtype == np.uint8 and np.array_equal(p.G, ec.unpacked(g, "G"))
    assert same_csr(p.H, g["hm_indptr"], g["hm_indices"], g["shape"])
    assert getattr(p, "P1", None) is None and getattr(p, "P2", None) is None
    k = p.G.shape[0]
    assert q["plan"]["form"] == _lib.ENC_DENSE and q["plan"]["k"] == k and q["plan"]["m1"] == p.G.shape[1] - k and q["plan"]["m2"] == 0
    assert q["n_out"] == g["cfg"]["n"] and q["params"].n == g["cfg"]["n"]                          # AR4JA: cropped to n rows
    # a second call with the same object: H is now Hm, G is given
    digest = q["plan"]["digest"]
    q2 = fec._prepare_encode(g["bits"], p)
    assert q2["plan"]["digest"] == digest and same_csr(p.H, g["hm_indptr"], g["hm_indices"], g["shape"])


def test_triangular_branch_writes_P1_P2_and_Hm_back(no_library):
    g = ec.load("p_648_r34")
    p = ec.param(g)
    q = fec._prepare_encode(g["bits"], p)
    assert np.array_equal(p.P1, ec.unpacked(g, "P1")) and np.array_equal(p.P2, ec.unpacked(g, "P2"))
    assert p.P1.dtype == np.uint8 and p.P1.shape == (27, 486) and p.P2.shape == (135, 486)
    assert same_csr(p.H, g["hm_indptr"], g["hm_indices"], g["shape"]) and getattr(p, "G", None) is None
    assert (q["plan"]["m1"], q["plan"]["m2"], q["plan"]["k"], q["n_out"]) == (27, 135, 486, 648)
    # P1 and P2 given (the reference returns None here): they encode, nothing is written, H is not needed
    given = ec.Param(mode="IEEE_802.11nD2", n=648, P1=p.P1, P2=p.P2)
    q2 = fec._prepare_encode(g["bits"], given)
    assert q2["plan"]["digest"] == q["plan"]["digest"] and getattr(given, "H", None) is None and getattr(given, "G", None) is None


def test_dvbs2_branch_leaves_the_parameters_alone(no_library):
    g = ec.load("dvbs2_m40_k88")
    p = ec.param(g)
    H = p.H
    q = fec._prepare_encode(g["bits"], p)
    assert p.H is H and getattr(p, "G", None) is None and getattr(p, "P1", None) is None
    plan = q["plan"]
    assert plan["form"] == _lib.ENC_SPARSE and (plan["k"], plan["m1"]) == (88, 40) and q["n_out"] == 128
    A = H.toarray()[:, :88]
    assert np.array_equal(np.diff(plan["indptr"]), A.sum(axis=1)) and np.array_equal(plan["indices"], np.nonzero(A)[1])


def test_a_missing_H_is_read_from_path_and_written_back(no_library, tmp_path):
    import os
    g = ec.load("g_648_r12")
    p = ec.Param(mode="IEEE_802.11nD2", n=648, R="1/2", path=os.path.dirname(fc.ALIST_648))
    fec._prepare_encode(g["bits"], p)
    assert np.array_equal(p.G, ec.unpacked(g, "G")) and same_csr(p.H, g["hm_indptr"], g["hm_indices"], g["shape"])
    # DVB-S2 keeps the matrix it read
    d = ec.load("dvbs2_m65_k130")
    fec.writeAlist(ec.H_of(d), tmp_path / "LDPC_DVBS2_195b_R23.txt")
    p = ec.Param(mode="DVBS2", n=195, R="2/3", path=str(tmp_path) + os.sep)
    fec._prepare_encode(d["bits"], p)
    assert same_csr(p.H, d["indptr"], d["indices"], d["shape"])


def test_eliminations_run_once_per_matrix(no_library, monkeypatch):
    g = ec.load("p_648_r34")
    calls = []
    inner = fec.triangP1P2
    monkeypatch.setattr(fec, "triangP1P2", lambda H: calls.append(1) or inner(H))
    monkeypatch.setattr(fec, "_ENC_SEEN", [])
    for _ in range(3):
        fec._prepare_encode(g["bits"], ec.param(g))
    assert len(calls) == 1


def test_par2gen_matches_the_reference():
    for name in ("g_648_r12", "g_ar4ja_1280"):
        g = ec.load(name)
        G, colSwaps, Hm = oa.par2gen(ec.H_of(g))
        assert G.dtype == np.uint8 and np.array_equal(G, ec.unpacked(g, "G")) and np.array_equal(colSwaps, g["colSwaps"])
        assert np.array_equal(Hm, ec.Hm_of(g).toarray())
        assert np.array_equal(oa.par2gen(ec.H_of(g).toarray())[0], G)   # a dense matrix in


def test_triangP1P2_matches_the_reference():
    assert oa.triangP1P2(ec.H_of(ec.load("g_648_r12"))) == (None, None, None)       # T is singular: the reference falls back to G
    g = ec.load("p_648_r34")
    P1, P2, Hm = oa.triangP1P2(ec.H_of(g))
    assert np.array_equal(P1, ec.unpacked(g, "P1")) and np.array_equal(P2, ec.unpacked(g, "P2"))
    assert np.array_equal(Hm, ec.Hm_of(g).toarray())


def test_small_eliminations_against_plain_loops():
    """gaussElim, inverseMatrixGF2 and triangularize on small random matrices against the reference's loops restated on plain
    arrays; singular and wide cases among them."""
    rng = np.random.default_rng(3)
    singular = 0
    for m, n in ((5, 9), (8, 8), (12, 20), (9, 4), (17, 33)):
        for _ in range(6):
            M = rng.integers(0, 2, size=(m, n)).astype(np.uint8)
            want = M.copy()
            lead = 0
            for r in range(m):                                          # fec.py:117-150
                while lead < n and not want[r:, lead].any():
                    lead += 1
                if lead == n:
                    break
                i = r + int(np.argmax(want[r:, lead]))
                want[[r, i]] = want[[i, r]]
                for j in range(m):
                    if j != r and want[j, lead]:
                        want[j] ^= want[r]
                lead += 1
            assert np.array_equal(fec.gaussElim(M), want)
            T, rowPerm, colPerm = fec.triangularize(M)
            tw, rp, cp = M.copy(), np.arange(m), np.arange(n)
            for i in range(m):                                          # fec.py:921-950
                hit = [(r, c) for r in range(i, m) for c in range(i, n) if tw[r, c]][:1]
                if not hit:
                    continue
                r, c = hit[0]
                tw[[i, r]], rp[[i, r]] = tw[[r, i]], rp[[r, i]]
                tw[:, [i, c]], cp[[i, c]] = tw[:, [c, i]], cp[[c, i]]
                for r in range(i + 1, m):
                    if tw[r, i]:
                        tw[r] ^= tw[i]
            assert np.array_equal(T, tw) and np.array_equal(rowPerm, rp) and np.array_equal(colPerm, cp)
            if m == n:
                inv, found = fec.inverseMatrixGF2(M)
                singular += not found
                if found:
                    assert np.array_equal((M.astype(int) @ inv.astype(int)) % 2, np.eye(m, dtype=int))
    assert singular >= 1
    inv, found = fec.inverseMatrixGF2(np.array([[0, 1, 0], [1, 1, 0], [1, 0, 1]]))
    assert found and np.array_equal(inv, [[1, 1, 0], [1, 0, 0], [1, 1, 1]])


def test_write_alist_round_trip(tmp_path):
    for name in ("dvbs2_m40_k88", "p_648_r34"):
        g = ec.load(name)
        oa.writeAlist(ec.H_of(g), tmp_path / "h.txt")
        H = oa.readAlist(tmp_path / "h.txt")
        assert same_csr(H, g["indptr"], g["indices"], g["shape"])
    # the committed table, written again, is the reference's text number for number
    H = oa.readAlist(fc.ALIST_648)
    oa.writeAlist(H.toarray(), tmp_path / "again.txt")
    tokens = [line.split() for line in open(fc.ALIST_648) if line.strip()]
    again = [line.split() for line in open(tmp_path / "again.txt") if line.strip()]
    assert again[:4 + 648] == tokens[:4 + 648]
