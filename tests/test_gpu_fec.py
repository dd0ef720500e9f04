"""Soft-decision FEC on the GPU (calcLLR, decodeLDPC) against the reference's recorded results (tests/golden/fec,
tools/gen_golden_fec.py) and, for graphs too large to store, against tests/fec_restatement.py, which a non-GPU test pins to the
same fixtures (run with -m gpu).

Bounds (tests/fec_cases.py): min-sum bit-equal to the reference in the same precision; sum-product in float64 within 1e-9 rel-L2
per codeword and 1e-9 of the column's max |ref| per element; in float32 within 4 x the reference's own distance between its
float32 and float64 runs, per codeword; decisions, frameErrors and lastIter equal in every case; calcLLR within 1e-9 relative
(floor 1e-12).  Every way of making one call -- numpy or DeviceArray, either engine, either orientation, a second time -- must
give the same bits."""
import numpy as np
import pytest

import fec_cases as fc
import fec_restatement as fr
import opticommpy_amd as oa
from fec_shape_cases import regular_code
from opticommpy_amd import _lib, device

pytestmark = pytest.mark.gpu


def host(a):
    return a.get() if isinstance(a, oa.DeviceArray) else a


def decode(llrs, prm, transposed=False, on_device=False):
    """One call; the results as (n_, numCodewords) numpy arrays whatever the orientation asked for."""
    x0 = np.ascontiguousarray(llrs.T if transposed else llrs)
    x = oa.to_device(x0) if on_device else x0.copy()
    before = device.transfer_counts()
    bits, out, fail, last = oa.decodeLDPC(x, prm, transposed=transposed, returnIter=True)
    three = oa.decodeLDPC(x, prm, transposed=transposed)
    after = device.transfer_counts()
    kind = oa.DeviceArray if on_device else np.ndarray
    assert type(bits) is kind and type(out) is kind and type(fail) is np.ndarray and type(last) is np.ndarray
    assert bits.shape == x0.shape and out.shape == x0.shape and len(three) == 3
    if on_device:
        assert after == before, (before, after)                         # no DeviceArray.get / .set inside the calls
    assert np.array_equal(host(x), x0)                                   # the input is never written
    bits, out = host(bits), host(out)
    assert np.array_equal(host(three[0]), bits) and host(three[1]).tobytes() == out.tobytes() and np.array_equal(three[2], fail)
    return (bits.T, out.T, fail, last) if transposed else (bits, out, fail, last)


def same_bits(a, b, label):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), label


@pytest.mark.parametrize("name", fc.EXPECTED_CASES)
def test_decoder_matches_the_reference(name):
    g = fc.load(name)
    fc.check_conditions(g)
    prec = g["cfg"]["prec"]
    first = None
    for engine in ("lds", "global"):
        for transposed in (False, True):
            for on_device in (False, True):
                label = f"{name} [{prec}, {engine}, transposed={transposed}, device={on_device}]"
                got = decode(g["llrs"], fc.param(g, engine=engine), transposed, on_device)
                if first is None:
                    first = got
                    fc.compare_decode(got, g, prec, label)
                same_bits(got, first, label)
    other = "float32" if prec == "float64" else "float64"
    got = decode(g["llrs"], fc.param(g, other))                          # engine left at 'auto'
    fc.compare_decode(got, g, other, f"{name} [{other}, auto]")
    same_bits(decode(g["llrs"], fc.param(g, other, engine="global"), True, True), got, name)
    x32 = g["llrs"].astype(np.float32)                                   # a single-precision input: clipped, then widened
    same_bits(decode(x32, fc.param(g, "float64", engine="lds")), decode(x32.astype(np.float64), fc.param(g, "float64", engine="global")), name)


@pytest.mark.parametrize("name", ["msa_648_mixed", "spa_648_mixed", "msa_ar4ja_punct"])
@pytest.mark.parametrize("ncw", [1, 65, 300])
def test_one_codeword_and_one_more_than_a_wavefront(name, ncw):
    """The fixture's columns repeated: every codeword of the batch must come out as the fixture's.  (300: more codewords than a
    workgroup of the global engine has threads, where its parity flags are kept per thread and not per codeword.)"""
    g = fc.load(name)
    cols = np.arange(ncw) % 4 if ncw > 1 else np.array([2])
    x = np.ascontiguousarray(g["llrs"][:, cols])
    for prec in fc.PRECS:
        got = {e: decode(x, fc.param(g, prec, engine=e), transposed=(e == "global"), on_device=True) for e in ("lds", "global")}
        fc.compare_decode(got["lds"], g, prec, f"{name} x {ncw} [{prec}]", columns=cols)
        same_bits(got["global"], got["lds"], name)


def test_reading_the_flags_early_changes_nothing():
    """syncEvery: the host looks at the convergence flags every few iterations and stops launching once every codeword is done."""
    for name in ("msa_648_iter25", "spa_648_iter25", "spa_648_mixed"):
        g = fc.load(name)
        want = decode(g["llrs"], fc.param(g, engine="global"))
        fc.compare_decode(want, g, g["cfg"]["prec"], name)
        for every in (1, 2, 7):
            same_bits(decode(g["llrs"], fc.param(g, engine="global", syncEvery=every)), want, (name, every))


def noisy_zero_codewords(n, snrs_dB, seed):
    rng = np.random.default_rng(seed)
    s2 = 10 ** (-np.asarray(snrs_dB) / 10)
    return 2 * (1 + np.sqrt(s2) * rng.normal(size=(n, len(snrs_dB)))) / s2


def test_a_graph_that_cannot_fit_in_lds():
    """n = 2^16, 196 608 edges: 1.5 MiB of float64 messages per codeword.  Two codewords, one clean enough to converge inside
    maxIter = 6 and one that cannot; against the restatement at the fixtures' bounds."""
    n = 1 << 16
    H = regular_code(n, 3)
    x = noisy_zero_codewords(n, [6.0, 1.0], 4)
    assert _lib.fec_lds_bytes(3 * n, n, "float32") > _lib.FEC_LDS_BUDGET
    with pytest.raises(ValueError, match="LDS"):
        oa.decodeLDPC(x, fc.Param(H=H, engine="lds", maxIter=6))
    for alg, prec in (("MSA", "float64"), ("MSA", "float32"), ("SPA", "float64")):
        want = fr.decode(H.indptr, H.indices, H.shape, x, alg, 6, prec)
        assert want[2].tolist() == [0, 1] and want[3][0] < 5 and want[3][1] == 5, (alg, prec, want[2], want[3])
        prm = fc.Param(H=H, alg=alg, maxIter=6, prec=np.dtype(prec).type)
        got = decode(x, prm, transposed=True, on_device=True)            # engine 'auto': the global one
        same_bits(decode(x, fc.Param(H=H, alg=alg, maxIter=6, prec=np.dtype(prec).type, engine="global")), got, alg)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (alg, prec)
        if alg == "MSA":
            assert np.array_equal(got[1], want[1]), (alg, prec)
        else:
            e2 = fc.rel_cols(got[1], want[1])
            emax = np.max(np.abs(got[1] - want[1]), axis=0) / np.max(np.abs(want[1]), axis=0)
            print(f"(3, 6)-regular, n = {n}, SPA float64: rel-L2 {e2}, element error / max |ref| {emax}")
            assert np.all(e2 <= fc.REL) and np.all(emax <= fc.REL)


def test_a_graph_that_needs_more_than_64_kib_of_lds():
    """n = 4096 in float32: 86 KiB of LDS, beyond what a workgroup gets without asking; in float64 the same graph does not fit and
    'auto' goes to the global engine."""
    n = 4096
    H = regular_code(n, 5)
    x = noisy_zero_codewords(n, [5.0, 1.0, 2.5], 6)
    need32, need64 = _lib.fec_lds_bytes(3 * n, n, "float32"), _lib.fec_lds_bytes(3 * n, n, "float64")
    assert 64 * 1024 < need32 <= _lib.FEC_LDS_BUDGET < need64
    for alg in ("MSA", "SPA"):
        prm = dict(H=H, alg=alg, maxIter=10, prec=np.float32)
        lds = decode(x, fc.Param(engine="lds", **prm), on_device=True)
        same_bits(decode(x, fc.Param(engine="global", **prm), transposed=True), lds, alg)
        same_bits(decode(x, fc.Param(**prm)), lds, alg)
        want = fr.decode(H.indptr, H.indices, H.shape, x, alg, 10, np.float32)
        assert np.array_equal(lds[0], want[0]) and np.array_equal(lds[2], want[2]) and np.array_equal(lds[3], want[3]), alg
        assert len(set(want[2].tolist())) == 2
        if alg == "MSA":
            assert np.array_equal(lds[1], want[1])
    with pytest.raises(ValueError, match="LDS"):
        oa.decodeLDPC(x, fc.Param(H=H, engine="lds", prec=np.float64))
    got = decode(x, fc.Param(H=H, alg="MSA", maxIter=10, prec=np.float64))
    assert np.array_equal(got[1], fr.decode(H.indptr, H.indices, H.shape, x, "MSA", 10, np.float64)[1])


@pytest.mark.parametrize("name", fc.LLR_CASES)
def test_llr_matches_the_reference(name):
    g = fc.load_llr(name)
    args = (g["sigma2"], g["constSymb"], g["bitMap"], g["px"])
    x0 = g["rxSymb"].copy()
    got = oa.calcLLR(x0, *args)
    assert type(got) is np.ndarray and np.array_equal(x0, g["rxSymb"])
    fc.compare_llr(got, g, name)
    xd = oa.to_device(x0)
    before = device.transfer_counts()
    gd = oa.calcLLR(xd, *args)
    gd2 = oa.calcLLR(xd, *args)
    assert device.transfer_counts() == before and type(gd) is oa.DeviceArray and gd.shape == got.shape and gd.dtype == np.float64
    assert gd.get().tobytes() == got.tobytes() == gd2.get().tobytes() and np.array_equal(xd.get(), x0)
    other = np.complex64 if x0.dtype == np.complex128 else np.complex128                 # the other input type: widened on load
    assert oa.calcLLR(x0.astype(other).astype(np.complex128), *args).tobytes() == oa.calcLLR(x0.astype(other), *args).tobytes()


def test_llr_sizes_around_a_workgroup():
    g = fc.load_llr("qam64_shaped")
    args = (g["sigma2"], g["constSymb"], g["bitMap"], g["px"])
    whole = oa.calcLLR(g["rxSymb"], *args)
    for n in (1, 255, 257, 1025):
        assert oa.calcLLR(g["rxSymb"][:n], *args).tobytes() == whole[:6 * n].tobytes(), n
    assert oa.calcLLR(g["rxSymb"][:0], *args).shape == (0,)


def test_the_end_of_the_chain_stays_on_the_device():
    """to_device(symbols) -> calcLLR -> reshape -> decodeLDPC(transposed=True): no host copy, the same bits as the host path with
    the reference's .T."""
    g = fc.load("msa_648_mixed")
    rng = np.random.default_rng(8)
    M, nwords, n = 16, 6, 648
    raw = oa.grayMapping(M, "qam")
    bitMap = oa.demodulateGray(raw, M, "qam").reshape(-1, 4)
    const = (raw / np.sqrt(np.mean(np.abs(raw) ** 2))).astype(np.complex128)
    px = np.ones(M) / M
    zero = const[np.flatnonzero(~bitMap.any(axis=1))[0]]                 # the symbol that carries 0000: the all-zero codeword
    snr_dB = 7.0
    s2 = 10 ** (-snr_dB / 10)
    nsym = nwords * n // 4
    rx = zero + np.sqrt(s2 / 2) * (rng.normal(size=nsym) + 1j * rng.normal(size=nsym))
    prm = fc.Param(H=fc.H_of(g), alg="SPA", maxIter=20, prec=np.float32)

    llr_h = oa.calcLLR(rx, s2, const, bitMap, px)
    bits_h, post_h, fail_h = oa.decodeLDPC(llr_h.reshape(nwords, -1).T, prm)

    rxd = oa.to_device(rx)
    before = device.transfer_counts()
    llr_d = oa.calcLLR(rxd, s2, const, bitMap, px)
    bits_d, post_d, fail_d, last = oa.decodeLDPC(llr_d.reshape(nwords, -1), prm, transposed=True, returnIter=True)
    assert device.transfer_counts() == before and isinstance(bits_d, oa.DeviceArray) and isinstance(post_d, oa.DeviceArray)
    assert bits_d.shape == (nwords, n) and post_d.dtype == np.float32
    assert np.array_equal(bits_d.get().T, bits_h) and post_d.get().T.tobytes() == np.ascontiguousarray(post_h).tobytes()
    assert np.array_equal(fail_d, fail_h)
    print(f"frameErrors {fail_d.tolist()}, lastIter {last.tolist()}, pre-FEC bit errors {int(np.sum(llr_h < 0))} of {llr_h.size}")
    assert np.sum(llr_h < 0) > 0 and fail_d.sum() < nwords and not bits_d.get()[fail_d == 0].any()
