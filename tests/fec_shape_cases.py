"""The case table of tests/test_gpu_fec_shapes.py, shared with tests/test_fec_emu.py (which runs the rows marked for it through the
g++ emulator): synthetic graphs and inputs with literal seeds at the sizes at which opticommpy_amd/csrc/engine_fec.hip and
fec_kernels.h take another path, judged against tests/fec_restatement.py at the bounds of tests/fec_cases.py, unchanged.

The engine's geometry: every kernel has 256 lanes.  The LDS engine gives a codeword to a workgroup, which strides over the m
checks, the n variables and the E edges (padded by one slot after every 32: fec::Padded); the global engine gives thread t node
t / ncw of codeword t % ncw and keeps its parity flags per codeword below 256 codewords, per thread from 256 on.  The sum-product
check body is unrolled to 8 entries for a largest check degree <= 8, to 32 for <= 32, and is a loop over up to 64 beyond.
calcLLR gives a thread a symbol and strides with at most 8192 workgroups, so one grid round is 8192 x 256 symbols.

Inputs of a decoding row: the all-zero codeword over BPSK, ``2 (1 + sigma randn) / sigma^2``, with sigma^2 per row such that the
outcome the row or its group is there for occurs (check_conditions).  The expectation is ``fr.decode`` in the row's ``prec``;
sum-product rows in float32 also get the float64 run, against which they are judged.

Groups (every one holds converged and failed codewords and two values of lastIter):
  degree   m = 40, n = 160, check degrees 2 .. dc with the first check of degree dc, dc = 8, 9, 32, 33, 64; a variable of degree 64
  tiny     one check of degree 2; Hamming (7, 4), E = 12; E = 31, 32, 33; the graph of the edge fixtures (a check of degree 1, a
           variable of degree 0), where min-sum posteriors are infinite
  group    n = 255, 256, 257 with m = n // 2; m = 255, 256, 257 with n = 2 m; n = 1023
  ncw      1 .. 513 codewords on m = 20, n = 40; 256 and 257 on m = 13
  iter     maxIter = 1, 2, 3 with a codeword that converges at iteration 0, one at the last iteration and one that fails
  input    n_ < n; a float32 input; inputs that hold +-inf, 0, -0.0 and values beyond the clip at 200
calcLLR rows (LLR_ROWS, expectation ``fr.calc_llr``): M = 2 .. 1024 in both complex widths on Gray-labelled rectangular QAM, shaped
``px`` and a zero in it, n around a workgroup and one past a grid round, at 12 dB where every LLR is finite; one M = 1024 row at
47 dB keeps +-inf and is judged as the underflow fixture is.

``regular_code`` (tests/test_gpu_fec.py builds its large graphs with it) lives here with the other graph builders.
"""
import collections
import functools

import numpy as np

import fec_cases as fc
import fec_restatement as fr

Row = collections.namedtuple("Row", "id group graph claim alg prec ncw maxIter sigma2 seed n_ in_dtype special inf emu")
# graph: the arguments of `graph`; claim: what the id says of the graph, as (name, value) pairs; n_ = 0: n; special: a dozen
# inputs replaced by +-inf, 0, -0.0, +-250; inf: the expectation holds infinite posteriors (and may hold NaN)
LlrRow = collections.namedtuple("LlrRow", "id M dtype n snr_dB shaping zero_px seed emu")

BLOCK = 256
PRECS = ("float32", "float64")
LLR_GRID = 8192 * BLOCK
SMALL = ("sampled", 20, 40, (), 2, 6, 40)       # the m = 20, n = 40 graph of the ncw, iter and input groups
# sigma^2 of the degree rows: the more variables a check holds, the cleaner they must be for some codeword to converge
DEGREE_SIGMA2 = {8: 0.4, 9: 0.3, 32: 0.3, 33: 0.3, 64: 0.25}


def sampled_graph(rng, m, n, first, lo, hi):
    """CSR (indptr, indices) of m checks over n variables: check i < len(first) has degree first[i], the others a degree drawn
    from lo .. hi; the columns of a check are distinct, drawn at random, ascending."""
    degrees = np.r_[np.asarray(first, dtype=np.int64), rng.integers(lo, hi + 1, size=m - len(first))]
    rows = [np.sort(rng.choice(n, size=int(d), replace=False)) for d in degrees]
    return np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32), np.concatenate(rows).astype(np.int32)


def regular_code(n, seed):
    """CSR of a seeded random (3, 6)-regular parity-check matrix with n variables: three layers, each a permutation of the
    variables dealt two to a check; a variable that meets itself in a check is swapped away until none does."""
    rng = np.random.default_rng(seed)
    m = n // 2
    layers = np.stack([rng.permutation(n) for _ in range(3)])           # check c gets layers[:, 2 c] and layers[:, 2 c + 1]
    for _ in range(100):
        cols = layers.reshape(3, m, 2).transpose(1, 0, 2).reshape(m, 6)
        s = np.sort(cols, axis=1)
        bad = np.flatnonzero(np.any(s[:, 1:] == s[:, :-1], axis=1))
        if not len(bad):
            break
        for c in bad:                                                    # move the check's entries of two layers elsewhere
            for layer in (1, 2):
                for k in (2 * c, 2 * c + 1):
                    o = int(rng.integers(0, n))
                    layers[layer, k], layers[layer, o] = layers[layer, o], layers[layer, k]
    else:
        raise AssertionError("no simple graph found")
    cols = np.sort(cols, axis=1)
    assert np.all(np.bincount(cols.reshape(-1), minlength=n) == 3)
    return fc.Csr(np.arange(0, 6 * m + 1, 6, dtype=np.int32), cols.reshape(-1).astype(np.int32), (m, n))


@functools.lru_cache(maxsize=None)
def graph(spec):
    """The parity-check matrix of a row (fc.Csr, read-only, built once per process)."""
    kind = spec[0]
    if kind == "sampled":
        _, m, n, first, lo, hi, seed = spec
        indptr, indices = sampled_graph(np.random.default_rng(seed), m, n, first, lo, hi)
    elif kind == "hub":                                                  # variable 0 in every one of 64 checks
        _, m, n, seed = spec
        ip, ix = sampled_graph(np.random.default_rng(seed), m, n - 1, (), 1, 5)
        rows = [np.r_[0, ix[ip[c]:ip[c + 1]] + 1] for c in range(m)]
        indptr, indices = np.concatenate(([0], np.cumsum([len(r) for r in rows]))), np.concatenate(rows)
    elif kind == "single":
        indptr, indices, m, n = [0, 2], [0, 1], 1, 2
    elif kind == "hamming":
        indptr, indices, m, n = [0, 4, 8, 12], [0, 2, 4, 6, 1, 2, 5, 6, 3, 4, 5, 6], 3, 7
    elif kind == "edge":
        g = fc.load("edge_msa_deg1")
        indptr, indices, (m, n) = g["indptr"], g["indices"], g["shape"]
    else:
        raise ValueError(spec)
    indptr, indices = np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32)
    indptr.setflags(write=False)
    indices.setflags(write=False)
    return fc.Csr(indptr, indices, (int(m), int(n)))


def _row(group, tag, spec, claim, alg, prec, sigma2, seed, ncw=3, maxIter=5, n_=0, in_dtype="float64", special=False, inf=False, emu=True):
    parts = [group, tag, alg.lower(), prec[-2:]] + ([f"n_{n_}"] if n_ else []) + (["in32"] if in_dtype == "float32" else []) + \
        (["special"] if special else []) + (["inf"] if inf else [])
    return Row("-".join(parts), group, spec, tuple(claim), alg, prec, ncw, maxIter, sigma2, seed, n_, in_dtype, special, inf, emu)


def _rows():
    rows = []
    both = (("SPA", "float64"), ("SPA", "float32"), ("MSA", "float64"), ("MSA", "float32"))

    def pair(i):                                                         # one sum-product and one min-sum row, the precisions swapped
        return (("SPA", "float64"), ("MSA", "float32")) if i % 2 == 0 else (("SPA", "float32"), ("MSA", "float64"))

    # the three forms of the sum-product check body, at and one beyond their limits; a variable of the largest degree
    for i, dc in enumerate((8, 9, 32, 33, 64)):
        spec = ("sampled", 40, 160, (dc,), 2, dc, 300 + dc)
        for alg, prec in both:
            rows.append(_row("degree", f"dc{dc}", spec, [("dc", dc), ("m", 40), ("n", 160)], alg, prec, DEGREE_SIGMA2[dc], 310 + i))
    for alg, prec in both:
        rows.append(_row("degree", "dv64", ("hub", 64, 80, 364), [("dv", 64), ("m", 64), ("n", 80)], alg, prec, 0.5, 320))
    # graphs below one workgroup, one wave, one padding step of the LDS message array
    for alg, prec in (("SPA", "float64"), ("MSA", "float64"), ("MSA", "float32")):
        # (no sum-product row in float32: the posterior of a lone check of degree 2 is llr + 2 atanh(tanh(llr' / 2)), which float32
        #  gives to within 1e-8 for some codeword, below what the float32 bound can be measured against)
        rows.append(_row("tiny", "single", ("single",), [("E", 2), ("m", 1), ("n", 2)], alg, prec, 1.0, 330, ncw=8))
    for alg, prec in both:
        rows.append(_row("tiny", "hamming", ("hamming",), [("E", 12), ("m", 3), ("n", 7)], alg, prec, 0.7, 331, ncw=8))
        rows.append(_row("tiny", "deg1", ("edge",), [("dc1", 1), ("dv0", 1), ("m", 12), ("n", 24)], alg, prec, 0.5, 332, ncw=6, maxIter=6,
                         inf=alg == "MSA"))
    for i, (E, first) in enumerate(((31, (3,) + (4,) * 7), (32, (4,) * 8), (33, (5,) + (4,) * 7))):
        for alg, prec in pair(i):
            rows.append(_row("tiny", f"E{E}", ("sampled", 8, 16, first, 0, 0, 340 + i), [("E", E), ("m", 8), ("n", 16)], alg, prec, 0.6, 345 + i, ncw=6))
    # n and m around a workgroup; four rounds of the LDS stride loops with a ragged tail
    for i, n in enumerate((255, 256, 257)):
        for alg, prec in pair(i):
            rows.append(_row("group", f"n{n}", ("sampled", n // 2, n, (), 2, 8, 350 + i), [("n", n), ("m", n // 2)], alg, prec, 0.45, 355 + i))
    for i, m in enumerate((255, 256, 257)):
        for alg, prec in pair(i + 1):
            rows.append(_row("group", f"m{m}", ("sampled", m, 2 * m, (), 2, 8, 360 + i), [("m", m), ("n", 2 * m)], alg, prec, 0.45, 365 + i))
    for alg, prec in pair(0):
        rows.append(_row("group", "n1023", ("sampled", 511, 1023, (), 2, 8, 370), [("n", 1023), ("m", 511)], alg, prec, 0.45, 371))
    # codeword counts around a wave and around the change of layout of the global engine's parity flags
    # (sum-product in float32 only with one or two codewords: its bound, a multiple of the restatement's own float32 error per
    #  codeword, compares two roundings of a recursion in which one message next to the product clip can carry the whole error;
    #  the g++ emulation exceeds 4 for about one codeword in 1500 -- 4.07 for one of 64 here -- which says nothing of the flags
    #  and the launch geometry that these rows are for.  Min-sum is bit-equal and float64 has two decades to spare.)
    for i, ncw in enumerate((1, 2, 63, 64, 65, 255, 256, 257, 513)):
        for alg, prec in (("SPA", "float64"), ("MSA", PRECS[i % 2])) + ((("SPA", "float32"),) if ncw <= 2 else ()):
            rows.append(_row("ncw", f"x{ncw}", SMALL, [("ncw", ncw), ("m", 20), ("n", 40)], alg, prec, 0.64, 380 + i, ncw=ncw, maxIter=6))
    for i, ncw in enumerate((256, 257)):
        for alg, prec in (("SPA", "float64"), ("MSA", PRECS[i % 2])):
            rows.append(_row("ncw", f"m13x{ncw}", ("sampled", 13, 26, (), 2, 6, 390), [("ncw", ncw), ("m", 13), ("n", 26)], alg, prec, 0.64,
                             391 + i, ncw=ncw, maxIter=6))
    # the first rows of the unsat flags and the edge of the early exit
    for i, maxIter in enumerate((1, 2, 3)):
        for alg, prec in (("SPA", "float32"), ("MSA", "float64")):
            rows.append(_row("iter", f"max{maxIter}", SMALL, [("m", 20), ("n", 40)], alg, prec, 0.5, 430, ncw=8, maxIter=maxIter))
    # punctured tails, the input's type, values the clip and the sign rules meet
    for i, n_ in enumerate((39, 33, 1)):
        for alg, prec in (("SPA", "float64"), ("MSA", "float32")):
            rows.append(_row("input", "punct", SMALL, [("m", 20), ("n", 40)], alg, prec, 0.5, 400 + i, ncw=6, maxIter=6, n_=n_))
    for alg, prec in both:
        rows.append(_row("input", "type", SMALL, [("m", 20), ("n", 40)], alg, prec, 0.6, 410, ncw=6, maxIter=6, in_dtype="float32"))
    for alg, prec, in_dtype in (("SPA", "float64", "float64"), ("SPA", "float32", "float64"), ("MSA", "float32", "float64"),
                                ("MSA", "float64", "float32"), ("SPA", "float64", "float32")):
        rows.append(_row("input", "values", SMALL, [("m", 20), ("n", 40)], alg, prec, 0.6, 420, ncw=6, maxIter=6, in_dtype=in_dtype, special=True))
    return rows


ROWS = _rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
EMU_ROWS = [r for r in ROWS if r.emu]
GROUPS = sorted({r.group for r in ROWS})


@functools.lru_cache(maxsize=None)
def signals(row):
    """The (n_, ncw) input LLRs of a row in its input type; read-only, built once per process."""
    n = graph(row.graph).shape[1]
    rng = np.random.default_rng(row.seed)
    x = 2 * (1 + np.sqrt(row.sigma2) * rng.normal(size=(n, row.ncw))) / row.sigma2
    x = x[:row.n_ or n]
    if row.special:
        flat = x.reshape(-1)
        at = rng.permutation(flat.size)[:12]
        flat[at] = [np.inf, -np.inf, 0.0, -0.0, 250.0, -250.0, np.inf, -np.inf, 0.0, -0.0, 1e30, -201.0]
    x = np.ascontiguousarray(x, dtype=row.in_dtype)
    x.setflags(write=False)
    return x


def _decode(row, prec):
    H = graph(row.graph)
    with np.errstate(invalid="ignore"):                                  # (inf - inf below a check of degree 1)
        return fr.decode(H.indptr, H.indices, H.shape, signals(row), row.alg, row.maxIter, prec)


@functools.lru_cache(maxsize=None)
def expected(row):
    """The restatement's results for a row in the form of a fixture of tests/fec_cases.py (what fc.compare_decode reads): out32 or
    out64 in the row's ``prec`` with bits64, fail64, iter64 from the same run; for sum-product in float32 also out64, with bits,
    fail and iter of that run under '_64', and self_err.  Read-only, computed once per process."""
    bits, out, fail, last = _decode(row, row.prec)
    g = dict(cfg=dict(alg=row.alg), llrs=signals(row), bits64=bits, fail64=fail, iter64=last)
    g["out64" if row.prec == "float64" else "out32"] = out
    if row.alg == "SPA" and row.prec == "float32":
        g["bits_64"], g["out64"], g["fail_64"], g["iter_64"] = _decode(row, "float64")
        g["self_err"] = fc.rel_cols(out, g["out64"])
    for a in g.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return g


def param(row, **extra):
    return fc.Param(H=graph(row.graph), alg=row.alg, maxIter=row.maxIter, prec=np.dtype(row.prec).type, **extra)


@functools.lru_cache(maxsize=None)
def _check_group(group):
    """Over a group: converged and failed codewords, and two values of lastIter."""
    rows = [r for r in ROWS if r.group == group]
    fails = np.concatenate([expected(r)["fail64"] for r in rows])
    iters = np.concatenate([expected(r)["iter64"] for r in rows if r.maxIter > 1])
    assert 0 in fails and 1 in fails and len(set(iters.tolist())) >= 2, (group, fails, iters)
    return True


def check_conditions(row):
    """The row cannot pass by luck, and it holds what its id says."""
    H, g, x = graph(row.graph), expected(row), signals(row)
    m, n = H.shape
    dc, dv = np.diff(H.indptr), np.bincount(H.indices, minlength=n)
    assert H.indptr.shape == (m + 1,) and dc.min() >= 1 and dc.max() <= 64 and dv.max() <= 64
    for c in range(m):                                                   # distinct ascending columns: a simple graph
        assert np.all(np.diff(H.indices[H.indptr[c]:H.indptr[c + 1]]) > 0), row.id
    have = dict(m=m, n=n, E=len(H.indices), ncw=row.ncw, dv=int(dv.max()), dc=int(dc.max()), dc1=int(np.sum(dc == 1)), dv0=int(np.sum(dv == 0)))
    for name, value in row.claim:
        assert have[name] == value, (row.id, name, have[name])
    if ("dc", have["dc"]) in row.claim:
        assert dc[0] == have["dc"] and dc.min() >= 2
    if "dc1" not in dict(row.claim):
        assert have["dc1"] == 0, row.id
    assert x.shape == (row.n_ or n, row.ncw) and x.dtype == np.dtype(row.in_dtype)
    tag = "out64" if row.prec == "float64" else "out32"
    out, fail, last = g[tag], g["fail64"], g["iter64"]
    assert out.dtype == np.dtype(row.prec) and out.shape == x.shape
    if row.inf:
        assert np.any(np.isinf(out)) and "inf" in row.id.split("-")
    else:
        assert np.all(np.isfinite(out)) and "inf" not in row.id.split("-"), row.id
    assert np.all(last[fail == 1] == row.maxIter - 1) and np.all(last < row.maxIter)
    if row.special:
        assert np.sum(np.isinf(x)) >= 4 and np.sum(x == 0) >= 4 and np.sum(np.signbit(x) & (x == 0)) >= 2 and np.sum(np.abs(x) > 200) >= 8
    if row.alg == "SPA" and row.prec == "float32":
        assert np.array_equal(g["bits_64"], g["bits64"]) and np.array_equal(g["fail_64"], fail) and np.array_equal(g["iter_64"], last), row.id
        assert np.all((g["self_err"] > 1e-8) & (g["self_err"] < 1e-3)), (row.id, g["self_err"])
    if row.group == "iter":
        assert np.any((fail == 0) & (last == 0)) and np.any((fail == 0) & (last == row.maxIter - 1)) and np.any(fail == 1), (row.id, fail, last)
    if row.group == "ncw" and row.ncw >= 63:                             # converged and failed codewords interleave
        assert np.sum(np.diff(fail.astype(int)) != 0) >= 8, (row.id, fail)
    _check_group(row.group)


def compare(row, got, label=""):
    """A decode of the row against the restatement at the bounds of tests/fec_cases.py; returns the measured figure."""
    return fc.compare_decode(got, expected(row), row.prec, f"{label} {row.id}", nan=row.inf)


# ---- calcLLR
def _llr_row(M, dtype, n, seed, snr_dB=12.0, shaping=0.0, zero_px=False, tag="", emu=True):
    parts = [f"M{M}", dtype, f"n{n}"] + (["shaped"] if shaping else []) + (["zeropx"] if zero_px else []) + ([tag] if tag else [])
    return LlrRow("-".join(parts), M, dtype, n, snr_dB, shaping, zero_px, seed, emu)


def _llr_rows():
    rows = []
    for i, M in enumerate((2, 4, 8, 32, 1024)):                          # one bit .. all ten, the whole LDS table
        for j, dtype in enumerate(("complex64", "complex128")):
            rows.append(_llr_row(M, dtype, (255, 257)[(i + j) % 2], 500 + 2 * i + j, shaping=(0.0, 0.5)[(i + j) % 2]))
    rows.append(_llr_row(8, "complex128", 300, 520, shaping=0.5, zero_px=True))
    rows.append(_llr_row(32, "complex64", 300, 521, zero_px=True))
    for i, n in enumerate((1, 255, 256, 257)):
        rows.append(_llr_row(4, ("complex128", "complex64")[i % 2], n, 530 + i, tag="size"))
    rows.append(_llr_row(2, "complex64", LLR_GRID + 1, 540, tag="stride"))   # the grid-stride loop takes a second round
    rows.append(_llr_row(1024, "complex128", 257, 541, snr_dB=47.0, tag="underflow"))
    return rows


LLR_ROWS = _llr_rows()
assert len({r.id for r in LLR_ROWS}) == len(LLR_ROWS)
EMU_LLR_ROWS = [r for r in LLR_ROWS if r.emu]


def constellation(M):
    """(points, bitMap) of a 2^ceil(b / 2) x 2^floor(b / 2) rectangular QAM with a Gray code per axis: square QAM where M is a
    square, +-1 for M = 2 (symbol 0, bit 0, at -1)."""
    b = M.bit_length() - 1
    bi, bq = (b + 1) // 2, b // 2
    pts, bits = [], []
    for i in range(1 << bi):
        for q in range(1 << bq):
            pts.append(complex(2 * i - ((1 << bi) - 1), 2 * q - ((1 << bq) - 1)))
            gi, gq = i ^ (i >> 1), q ^ (q >> 1)
            bits.append([(gi >> (bi - 1 - k)) & 1 for k in range(bi)] + [(gq >> (bq - 1 - k)) & 1 for k in range(bq)])
    return np.array(pts, dtype=np.complex128), np.array(bits, dtype=np.int64).reshape(M, b)


@functools.lru_cache(maxsize=None)
def llr_signals(row):
    """A calcLLR row in the form of an ``llr_*.npz`` fixture (rxSymb, sigma2, constSymb, bitMap, px, llr, cfg): the expectation
    ``llr`` is fr.calc_llr; read-only, built once per process."""
    rng = np.random.default_rng(row.seed)
    const, bitMap = constellation(row.M)
    px = np.exp(-row.shaping * np.abs(const) ** 2 / np.mean(np.abs(const) ** 2)) * (1 + row.shaping * np.arange(row.M) / row.M)
    if row.zero_px:
        px[row.M // 2 + 1] = 0.0
    px = px / px.sum()
    const = const / np.sqrt(np.sum(np.abs(const) ** 2 * px))
    sigma2 = 10 ** (-row.snr_dB / 10)
    tx = const[rng.choice(row.M, size=row.n, p=px)]
    rx = (tx + np.sqrt(sigma2 / 2) * (rng.normal(size=row.n) + 1j * rng.normal(size=row.n))).astype(row.dtype)
    with np.errstate(divide="ignore"):
        llr = fr.calc_llr(rx, sigma2, const, bitMap, px)
    g = dict(rxSymb=rx, sigma2=sigma2, constSymb=const, bitMap=bitMap, px=px, llr=llr, cfg=dict(name=row.id))
    for a in g.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return g


def check_llr_conditions(row):
    g = llr_signals(row)
    want = g["llr"]
    b = row.M.bit_length() - 1
    assert g["constSymb"].shape == (row.M,) and g["bitMap"].shape == (row.M, b) and g["rxSymb"].shape == (row.n,)
    assert len({tuple(r) for r in g["bitMap"].tolist()}) == row.M       # a labelling: every word once
    assert want.shape == (row.n * b,) and not np.any(np.isnan(want))
    assert (np.sum(g["px"] == 0) == 1) == row.zero_px and (np.ptp(g["px"]) > 1e-3) == bool(row.shaping or row.zero_px)
    if row.id.endswith("underflow"):
        # infinite where a sum underflowed to nothing; the finite ones far from the subnormal range, where exp loses digits
        fin = np.isfinite(want)
        assert np.sum(~fin) >= 100 and np.sum(fin) >= 100 and np.max(np.abs(want[fin])) < 690, row.id
    else:
        assert np.all(np.isfinite(want)), row.id
    assert np.any(want > 0) and np.any(want < 0)
    if row.n > LLR_GRID:
        assert row.n == LLR_GRID + 1


def compare_llr(row, got, label=""):
    fc.compare_llr(got, llr_signals(row), f"{label} {row.id}")
