"""encodeLDPC and modulateGray on the GPU against the reference's recorded codewords and symbols (tests/golden/enc,
tools/gen_golden_enc.py), and the loop they close: encode -> map -> LLR -> decode -> the codewords again, on DeviceArrays (run with
-m gpu).  The arithmetic is GF(2) and a table lookup: every comparison is ``np.array_equal``, and every way of making one call --
numpy or DeviceArray, either orientation, a second time -- must give the same bytes."""
import numpy as np
import pytest

import enc_cases as ec
import opticommpy_amd as oa
from opticommpy_amd import device, fec

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def encode(bits, prm, transposed=False, on_device=False, dtype=np.uint8):
    """One call, made twice; the codewords as an (n, N) numpy array whatever the orientation asked for."""
    x0 = np.ascontiguousarray((bits.T if transposed else bits).astype(dtype))
    x = oa.to_device(x0) if on_device else x0.copy()
    before = device.transfer_counts()
    cw = oa.encodeLDPC(x, prm, transposed=transposed)
    again = oa.encodeLDPC(x, prm, transposed=transposed)
    after = device.transfer_counts()
    assert type(cw) is (oa.DeviceArray if on_device else np.ndarray) and cw.dtype == np.uint8
    if on_device:
        assert after == before, (before, after)                         # no DeviceArray.get / .set inside the calls
    assert np.array_equal(host(x), x0)                                  # the input is never written
    cw, again = host(cw), host(again)
    assert cw.tobytes() == again.tobytes()
    return cw.T if transposed else cw


@pytest.mark.parametrize("name", sorted(ec.EXPECTED_CASES))
def test_encoder_matches_the_reference(name):
    g = ec.load(name)
    ec.check_conditions(g)
    for transposed in (False, True):
        for on_device in (False, True):
            p = ec.param(g)                                             # a fresh object: the branch is taken from H every time
            got = encode(g["bits"], p, transposed, on_device)
            assert got.shape == g["codewords"].shape and np.array_equal(got, g["codewords"]), (name, transposed, on_device)
            branch = g["cfg"]["branch"]
            assert (getattr(p, "G", None) is not None) == (branch == "G") and (getattr(p, "P1", None) is not None) == (branch == "P1P2")
    # the object of the last call again (G or P1 / P2 set, H = Hm), int8 on the device, more codewords than a tile
    cols = np.arange(37) % g["bits"].shape[1]
    got = encode(np.ascontiguousarray(g["bits"][:, cols]), p, True, True, np.int8)
    assert np.array_equal(got, g["codewords"][:, cols])
    assert len(fec.encoder_cache_info()) >= 1


def test_an_encoder_is_uploaded_once_per_code():
    fec.release_encoders()
    assert fec.encoder_cache_info() == []
    a, b = ec.load("dvbs2_m40_k88"), ec.load("p_648_r34")
    for _ in range(2):
        for g in (a, b):
            assert np.array_equal(oa.encodeLDPC(g["bits"], ec.param(g)), g["codewords"])
    info = fec.encoder_cache_info()
    assert len(info) == 2 and len(set(info)) == 2 and all(dev == 0 for dev, _ in info)
    for k in range(fec._GRAPH_CAP + 3):                                 # more codes than are kept: the oldest are destroyed
        G = np.hstack((np.eye(4, dtype=np.uint8), np.array([[(k >> j) & 1 for j in range(5)]] * 4, dtype=np.uint8)))
        G[0, 4:] = 1
        cw = oa.encodeLDPC(np.eye(4, dtype=np.uint8), ec.Param(mode="AR4JA", n=9, G=G))
        assert np.array_equal(cw, G.T)
    assert len(fec.encoder_cache_info()) == fec._GRAPH_CAP and info[0] not in fec.encoder_cache_info()
    assert np.array_equal(oa.encodeLDPC(a["bits"], ec.param(a)), a["codewords"])                   # uploaded again
    fec.release_encoders()
    assert fec.encoder_cache_info() == []


def test_P1_and_P2_given_encode():
    g = ec.load("p_648_r34")
    p = ec.Param(mode="IEEE_802.11nD2", n=648, P1=ec.unpacked(g, "P1"), P2=ec.unpacked(g, "P2"))
    assert np.array_equal(encode(g["bits"], p, True, True), g["codewords"])
    assert getattr(p, "H", None) is None


def test_a_device_array_counts_as_b_and_1():
    g = ec.load("dvbs2_m40_k88")
    noisy = (g["bits"] + 2 * np.random.default_rng(1).integers(0, 64, size=g["bits"].shape)).astype(np.uint8)
    assert noisy.max() > 1 and np.array_equal(noisy & 1, g["bits"])
    got = oa.encodeLDPC(oa.to_device(noisy), ec.param(g)).get()
    assert np.array_equal(got, g["codewords"])


@pytest.mark.parametrize("name", ec.MOD_CASES)
def test_mapper_matches_the_reference(name):
    g = ec.load_mod(name)
    ec.check_mod_conditions(g)
    c = g["cfg"]
    want = g["symbols"].astype(np.complex128)
    got = oa.modulateGray(g["bits"], c["M"], c["constType"])
    assert type(got) is np.ndarray and got.dtype == np.complex128 and np.array_equal(got, want)
    for dtype in (np.uint8, np.int8):
        d = oa.to_device(g["bits"].astype(dtype))
        before = device.transfer_counts()
        got_d = oa.modulateGray(d, c["M"], c["constType"])
        again = oa.modulateGray(d, c["M"], c["constType"])
        assert device.transfer_counts() == before and type(got_d) is oa.DeviceArray and got_d.dtype == np.complex128
        assert got_d.get().tobytes() == want.tobytes() and again.get().tobytes() == want.tobytes()


def test_closed_loop_on_device_arrays():
    """encodeLDPC -> modulateGray(16-QAM) -> pnorm -> calcLLR -> decodeLDPC with param.H as encodeLDPC wrote it back (the codewords
    of the 648 R1/2 table satisfy Hm, not the table's own H): the decoder returns the codewords at iteration 0, and no array
    crosses the bus between the first call and the last."""
    g = ec.load("g_648_r12")
    M, N = 16, 8
    rng = np.random.default_rng(7)
    msgs = rng.integers(0, 2, size=(N, g["bits"].shape[0])).astype(np.uint8)
    const = oa.grayMapping(M, "qam").astype(np.complex128)
    const = const / np.sqrt(np.mean(np.abs(const) ** 2))
    b = 4
    bitMap = (np.arange(M)[:, None] >> np.arange(b - 1, -1, -1)) & 1     # point i carries the label i
    px = np.full(M, 1 / M)
    p = ec.param(g)
    msgs_d = oa.to_device(msgs)
    before = device.transfer_counts()
    cw = oa.encodeLDPC(msgs_d, p, transposed=True)                      # (N, 648)
    symb = oa.modulateGray(cw.reshape(-1), M, "qam")
    symb = oa.pnorm(symb)
    llr = oa.calcLLR(symb, 0.02, const, bitMap, px)
    dec = ec.Param(H=p.H, alg="MSA", maxIter=5, prec=np.float64)
    bits, post, fail, last = oa.decodeLDPC(llr.reshape(N, -1), dec, transposed=True, returnIter=True)
    assert device.transfer_counts() == before
    assert all(type(a) is oa.DeviceArray for a in (cw, symb, llr, bits, post))
    cw_h = cw.get()
    assert cw_h.shape == (N, 648) and np.array_equal(cw_h[:, :324], msgs) and cw_h[:, 324:].any()
    assert np.array_equal(bits.get(), cw_h.astype(np.int8))
    assert np.array_equal(fail, np.zeros(N, dtype=np.int8)) and np.array_equal(last, np.zeros(N, dtype=np.uint32))
    assert np.isclose(np.mean(np.abs(symb.get()) ** 2), 1.0)
    # the table's own H does not hold for these codewords: the write-back matters
    H0 = ec.H_of(g).toarray().astype(np.int64)
    assert ((H0 @ cw_h.T.astype(np.int64)) % 2).any()
    assert not ((p.H.toarray().astype(np.int64) @ cw_h.T.astype(np.int64)) % 2).any()
