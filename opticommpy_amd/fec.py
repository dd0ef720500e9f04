"""Soft-decision FEC on the device: the soft demapper ``calcLLR`` and the LDPC belief-propagation decoder ``decodeLDPC``.

Drop-ins for ``calcLLR`` (optic/comm/metrics.py:198-239) and ``decodeLDPC`` (optic/comm/fec.py:347-758 with
``sumProductAlgorithm`` and ``minSumAlgorithm``), the two calls that end the reference's receive chain
(examples/test_fec.ipynb), plus ``readAlist`` (fec.py:811-838).  A ``DeviceArray`` in gives ``DeviceArray``s out, so

    llr = oa.calcLLR(symbols_d, sigma2, constSymb, bitMap, px)            # DeviceArray, length n log2 M
    bits, post, frameErrors = oa.decodeLDPC(llr.reshape(Nwords, -1), param, transposed=True)

runs without a host copy.  The schedule, the edge order and the arithmetic are fixed in opticommpy_amd/csrc/fec_kernels.h:
min-sum is bit-equal to the reference in the same ``prec``, sum-product differs from it by rounding only (prefix and suffix
products instead of the reference's ordered O(d_c^2) product).

Two engines run the same node bodies in the same order and return the same bits (``param.engine``: 'auto', 'lds', 'global'):
'lds' decodes a codeword in one workgroup with every message in LDS, 'global' keeps the messages in device memory for graphs that
do not fit; 'auto' takes 'lds' whenever the graph fits in a workgroup's 160 KiB.  The global engine never waits for the host inside
a decode unless ``param.syncEvery = k`` asks it to read the convergence flags every ``k`` iterations and stop early (default 0).

Scope and limits (anything else raises ``ValueError`` before the library is loaded; there is no CPU fallback):

* ``param.H``: anything with CSR ``indptr``, ``indices`` and ``shape`` (a ``scipy.sparse.csr_matrix`` is one, and so is what
  ``readAlist`` returns), or a dense 0/1 array.  scipy is not needed.  The edges of a check are taken in ascending column index;
* ``param.alg`` 'SPA' or 'MSA'; ``param.prec`` float32 (the default) or float64; ``param.maxIter`` >= 1 (default 25);
* ``n_ <= n`` (``n_ < n``: the last ``n - n_`` variables are punctured), every check degree 1 .. 64, every variable degree <= 64;
  a check of degree 1 under MSA yields infinite messages (and NaN back on that edge, taken as negative), as in the reference;
* ``calcLLR``: ``M`` a power of two, 2 .. 1024, ``bitMap`` of shape ``(M, log2 M)`` with entries 0 and 1.

Deviations from the reference, on purpose:

* ``transposed=True`` takes and returns ``(numCodewords, n_)`` arrays (what ``calcLLR(...).reshape(Nwords, -1)`` gives: a
  ``DeviceArray`` has no ``.T``).  It has one now (``opticommpy_amd/device.py``: a transposed copy), so the reference's own line
  ``.reshape(Nwords, -1).T`` runs on the device too; ``transposed=True`` stays and saves that copy;
* ``returnIter=True`` also returns ``lastIter`` (uint32), which the reference computes and only logs;
* ``frameErrors`` and ``lastIter`` are numpy arrays whatever the input is (``numCodewords`` values);
* an unsupported ``alg`` or a missing ``H`` raises (the reference logs an error and fails later);
* ``calcLLR`` computes in double whatever it is given (the reference's arithmetic is single precision when ``rxSymb`` and
  ``constSymb`` are both complex64), and sums ``p0`` / ``p1`` over the constellation in ascending order.

The transmit side of the same loop: ``encodeLDPC`` (fec.py:153-251 with ``encodeDVBS2``, ``encoder``, ``encodeTriang``) and
``modulateGray`` (optic/comm/modulation.py:334-366), with the host helpers ``par2gen``, ``triangP1P2`` and ``writeAlist``:

    cw = oa.encodeLDPC(bits_d, param, transposed=True)                    # (N, k) uint8 in, (N, n) uint8 out, DeviceArrays
    symb = oa.modulateGray(cw.reshape(-1), 16, 'qam')                     # the notebook's codedBits.T.flatten(), complex128

The arithmetic is GF(2) and a table lookup, so every result is the reference's bit for bit.  ``param.mode``, ``n``, ``R``, ``H``,
``G``, ``systematic``, ``P1``, ``P2`` and ``path`` are read and written back as the reference does (``param.H`` as a ``CSR``, which
``decodeLDPC`` takes).  The Gaussian eliminations behind ``par2gen`` / ``triangP1P2`` run once per code on the host, on bit-packed
rows, in the reference's pivot order; the device holds the parity rows as 64-bit words (``G`` and ``P1`` / ``P2``) or the CSR of
``A = H[:, :k]`` (DVB-S2), found again by digest.  Limits: ``N <= 65535``; ``k <= 32768`` for the dense forms, ``k <= 131072`` for
DVB-S2; ``modulateGray``: ``M`` a power of two, 2 .. 1024, 'qam' (square), 'psk', 'pam' or 'ook'.

Deviations of the encoder from the reference, on purpose:

* ``transposed=True`` takes ``(N, k)`` and returns ``(N, n)``, as ``decodeLDPC``'s keyword does;
* with ``param.P1`` and ``param.P2`` already set the reference returns ``None`` (so does its second call with one ``param``): here
  they encode;
* an unsupported ``mode``, a missing file or a missing ``H`` raises (the reference logs an error and fails later); a triangularised
  matrix whose last column holds no one, where the reference fails inside ``numpy.min``, counts as not triangularisable:
  ``triangP1P2`` returns ``(None, None, None)`` and the generator matrix is used;
* what ``triangP1P2`` / ``par2gen`` make of a matrix is kept per matrix (the reference repeats a failed triangularisation on every
  call);
* host ``bits`` holding anything but 0 / 1 raise; a ``DeviceArray`` is used as ``b & 1``;
* ``modulateGray`` returns complex128 whatever the table's type (the reference: complex64, float32 for 'pam' / 'ook').

Not here: ``calcExtrLLR``, layered schedules, Hamming codes, a device version of the eliminations.
"""
import ctypes as C
import hashlib
import os

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["calcLLR", "decodeLDPC", "readAlist", "encodeLDPC", "modulateGray", "par2gen", "triangP1P2", "writeAlist"]

MAX_DEGREE = _lib.FEC_MAX_DEGREE
MAX_CODEWORDS = 65535
_REAL = ("float64", "float32")
_CPLX = ("complex128", "complex64")


class CSR:
    """The ones of a sparse 0/1 matrix, row by row: ``indices[indptr[i]:indptr[i + 1]]`` are the columns of row ``i``, ascending."""

    def __init__(self, indptr, indices, shape):
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        self.indices = np.ascontiguousarray(indices, dtype=np.int32)
        self.shape = (int(shape[0]), int(shape[1]))

    @property
    def nnz(self):
        return int(self.indices.size)

    def toarray(self):
        H = np.zeros(self.shape, dtype=np.uint8)
        H[np.repeat(np.arange(self.shape[0]), np.diff(self.indptr)), self.indices] = 1
        return H

    def __repr__(self):
        return f"CSR(shape={self.shape}, nnz={self.nnz})"


def _csr_from_pairs(rows, cols, shape):
    """CSR of the ones at (rows, cols); a pair named twice is one entry, as an assignment into a dense matrix makes it."""
    m, n = shape
    flat = np.unique(np.asarray(rows, dtype=np.int64) * n + np.asarray(cols, dtype=np.int64))
    r = flat // n
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=m), out=indptr[1:])
    return CSR(indptr, flat - r * n, shape)


def readAlist(filename):
    """Read an ALIST file (fec.py:811-838): line 0 is ``n m``, lines 4 .. 4 + n - 1 list the checks of every variable, 1-based,
    padded with zeros; blank lines are dropped first.  Returns the parity-check matrix as a ``CSR``; the dense matrix is never
    built."""
    with open(filename, "r") as f:
        lines = [line.strip() for line in f if line.strip()]
    n, m = map(int, lines[0].split())
    rows, cols = [], []
    for j, line in enumerate(lines[4:4 + n]):
        for entry in map(int, line.split()):
            if entry > 0:
                if entry > m:
                    raise ValueError(f"{filename}: variable {j} names check {entry} of {m}")
                rows.append(entry - 1)
                cols.append(j)
    return _csr_from_pairs(rows, cols, (m, n))


def _as_csr(H):
    """(indptr, indices, m, n) of a parity-check matrix in any accepted form, int32, the columns of every row ascending."""
    if H is None:
        raise ValueError("param.H is None: a parity-check matrix is needed")
    if all(hasattr(H, a) for a in ("indptr", "indices", "shape")):
        if getattr(H, "format", "csr") != "csr":
            raise ValueError(f"param.H is a sparse matrix in {H.format!r} format: CSR is needed (H.tocsr())")
        m, n = int(H.shape[0]), int(H.shape[1])
        indptr, indices = np.asarray(H.indptr, dtype=np.int64), np.asarray(H.indices, dtype=np.int64)
        if indptr.shape != (m + 1,) or indptr[0] != 0 or indptr[-1] != indices.size or np.any(np.diff(indptr) < 0):
            raise ValueError("param.H: indptr does not describe the rows of indices")
        if indices.size and (indices.min() < 0 or indices.max() >= n):
            raise ValueError("param.H: a column index lies outside the matrix")
        data = getattr(H, "data", None)
        if data is not None and np.size(data) == indices.size and not np.all(np.asarray(data) != 0):
            keep = np.asarray(data) != 0                                # stored zeros are no edges
            rows = np.repeat(np.arange(m), np.diff(indptr))[keep]
            return _as_csr(_csr_from_pairs(rows, indices[keep], (m, n)))
        inner = np.ones(indices.size, dtype=bool)
        inner[indptr[:-1][np.diff(indptr) > 0]] = False                 # first entry of every non-empty row
        if indices.size > 1 and np.any((np.diff(indices) <= 0) & inner[1:]):
            rows = np.repeat(np.arange(m), np.diff(indptr))
            return _as_csr(_csr_from_pairs(rows, indices, (m, n)))
        return indptr.astype(np.int32), indices.astype(np.int32), m, n
    D = np.asarray(H)
    if D.ndim != 2:
        raise ValueError("param.H must be a matrix")
    if not np.all((D == 0) | (D == 1)):
        raise ValueError("a dense param.H must hold 0 and 1 only")
    rows, cols = np.nonzero(D)
    return _as_csr(_csr_from_pairs(rows, cols, D.shape))


def build_graph(indptr, indices, n):
    """The four edge maps of fec.py:388-411 from H's CSR: the edge id is the position in ``indices``; a variable's edges are
    listed in ascending edge id, which is ascending check index."""
    indices = np.asarray(indices, dtype=np.int32)
    var_offsets = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(indices, minlength=n), out=var_offsets[1:])
    return dict(check_offsets=np.ascontiguousarray(indptr, dtype=np.int32), edge_var=np.ascontiguousarray(indices),
                var_offsets=var_offsets, var_edge_indices=np.argsort(indices, kind="stable").astype(np.int32))


# what _code_of made of the matrices seen last, found again by comparing the CSR arrays themselves (a memcmp, where the edge maps
# and the digest of a 64 800-bit code cost more than its decode)
_SEEN = []
_SEEN_CAP = 8


def _code_of(H):
    """Everything a decode needs of ``param.H``, checked: dict with ``m``, ``n``, ``E``, ``graph`` (the four edge maps) and
    ``digest`` (of the canonical CSR: the key of the device-side graph cache)."""
    if H is None:
        raise ValueError("param.H is None: a parity-check matrix is needed")
    raw = None
    if all(hasattr(H, a) for a in ("indptr", "indices", "shape")) and getattr(H, "format", "csr") == "csr":
        data = getattr(H, "data", None)
        if data is None or bool(np.all(np.asarray(data) != 0)):
            raw = (np.asarray(H.indptr), np.asarray(H.indices), (int(H.shape[0]), int(H.shape[1])))
            for k, ent in enumerate(_SEEN):
                if ent["shape"] == raw[2] and np.array_equal(ent["indptr"], raw[0]) and np.array_equal(ent["indices"], raw[1]):
                    _SEEN.append(_SEEN.pop(k))
                    return ent["code"]
    indptr, indices, m, n = _as_csr(H)
    dc = np.diff(indptr)
    if m < 1 or np.any(dc == 0):
        raise ValueError("param.H has a check of degree 0")
    if dc.max() > MAX_DEGREE:
        raise ValueError(f"a check has degree {int(dc.max())}: at most {MAX_DEGREE} is supported")
    graph = build_graph(indptr, indices, n)
    dv = np.diff(graph["var_offsets"])
    if dv.max() > MAX_DEGREE:
        raise ValueError(f"a variable has degree {int(dv.max())}: at most {MAX_DEGREE} is supported")
    h = hashlib.blake2b(digest_size=16)
    h.update(np.array([m, n], dtype=np.int64).tobytes())
    h.update(graph["check_offsets"].tobytes())
    h.update(graph["edge_var"].tobytes())
    code = dict(m=m, n=n, E=int(indices.size), graph=graph, digest=h.hexdigest())
    if raw is not None:
        _SEEN.append(dict(shape=raw[2], indptr=raw[0].copy(), indices=raw[1].copy(), code=code))
        del _SEEN[:-_SEEN_CAP]
    return code


def _llr_array(llrs):
    if _dev.is_device(llrs):
        if llrs.dtype.name not in _REAL:
            raise TypeError(f"device array llrs has dtype {llrs.dtype.name}: float64 or float32 expected")
    else:
        llrs = np.asarray(llrs)
        if llrs.dtype.name not in _REAL:
            llrs = llrs.astype(np.float64)
    if llrs.ndim != 2:
        raise ValueError("llrs must have two dimensions: (n_, numCodewords), or (numCodewords, n_) with transposed=True")
    return llrs


def _prepare(llrs, param, transposed=False):
    """Every check and every host-side quantity of a decode, without touching the library: a dict with ``llrs`` (2-D), ``params``
    (``_lib.LdpcParams``), ``graph`` (the four edge maps), ``m``, ``n``, ``E``, ``digest``, ``prec``."""
    H = getattr(param, "H", None)
    maxIter = getattr(param, "maxIter", 25)
    alg = getattr(param, "alg", "SPA")
    prec = getattr(param, "prec", np.float32)
    engine = getattr(param, "engine", "auto")
    syncEvery = getattr(param, "syncEvery", 0)
    if H is None:
        raise ValueError("param.H is None: a parity-check matrix is needed")
    if alg not in _lib.FEC_ALGS:
        raise ValueError(f"Unsupported algorithm: {alg!r}. Supported algorithms are: SPA, MSA.")
    try:
        prec = np.dtype(prec)
    except TypeError:
        raise ValueError(f"prec must be float32 or float64, not {prec!r}") from None
    if prec.name not in _REAL:
        raise ValueError(f"prec must be float32 or float64, not {prec.name}")
    if int(maxIter) != maxIter or maxIter < 1 or maxIter > 65535:
        raise ValueError(f"maxIter = {maxIter}: an integer between 1 and 65535 is needed")
    if engine not in _lib.FEC_ENGINES:
        raise ValueError(f"engine must be one of {', '.join(_lib.FEC_ENGINES)}, not {engine!r}")
    if int(syncEvery) != syncEvery or syncEvery < 0:
        raise ValueError(f"syncEvery = {syncEvery}: 0 (never) or a number of iterations is needed")

    llrs = _llr_array(llrs)
    n_, ncw = (llrs.shape[1], llrs.shape[0]) if transposed else (llrs.shape[0], llrs.shape[1])
    code = _code_of(H)
    m, n, E = code["m"], code["n"], code["E"]
    if n_ > n:
        raise ValueError(f"llrs has {n_} rows per codeword, the code has n = {n} variables")
    if n_ < 1 or ncw < 1 or ncw > MAX_CODEWORDS:
        raise ValueError(f"llrs of shape {tuple(llrs.shape)}: between 1 and {MAX_CODEWORDS} codewords of at least one LLR are needed")
    if engine == "lds" and _lib.fec_lds_bytes(E, n, prec.name) > _lib.FEC_LDS_BUDGET:
        raise ValueError(f"engine = 'lds': the graph needs {_lib.fec_lds_bytes(E, n, prec.name)} bytes of LDS, a workgroup has "
                         f"{_lib.FEC_LDS_BUDGET}: use 'global' or 'auto'")
    params = _lib.LdpcParams(n_=int(n_), numCodewords=int(ncw), maxIter=int(maxIter), alg=_lib.FEC_ALGS[alg], prec=_lib.FEC_PRECS[prec.name],
                             in_dtype=_lib.FEC_PRECS[llrs.dtype.name], transposed=int(bool(transposed)), engine=_lib.FEC_ENGINES[engine],
                             sync_every=int(syncEvery))
    return dict(llrs=llrs, params=params, graph=code["graph"], m=m, n=n, E=E, digest=code["digest"], prec=prec)


# graph handles of ssf_ldpc_graph_create by (device, digest of H's CSR): a code is uploaded once, as edc keeps its filter designs
_GRAPHS = {}
_GRAPH_CAP = 16


def graph_cache_info():
    """(device, digest) keys of the graphs held on the device, oldest first."""
    return list(_GRAPHS)


def release_graphs():
    """Free every cached graph."""
    lib = _lib.load()
    while _GRAPHS:
        lib.ssf_ldpc_graph_destroy(_GRAPHS.pop(next(iter(_GRAPHS))))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _create_graph(lib, device, q):
    g = q["graph"]
    handle = C.c_void_p()
    rc = lib.ssf_ldpc_graph_create(device, q["m"], q["n"], q["E"], _ip(g["check_offsets"]), _ip(g["edge_var"]), _ip(g["var_offsets"]),
                                   _ip(g["var_edge_indices"]), C.byref(handle))
    _lib.raise_for(lib, None, rc)
    return handle


def _graph_handle(lib, device, q):
    """The device graph of a prepared call: created on first use, then found by (device, digest); the least recently used of more
    than ``_GRAPH_CAP`` is destroyed."""
    key = (device, q["digest"])
    handle = _GRAPHS.pop(key, None)
    if handle is None:
        handle = _create_graph(lib, device, q)
        while len(_GRAPHS) >= _GRAPH_CAP:
            lib.ssf_ldpc_graph_destroy(_GRAPHS.pop(next(iter(_GRAPHS))))
    _GRAPHS[key] = handle                                               # most recently used last
    return handle


def decodeLDPC(llrs, param, *, transposed=False, returnIter=False):
    """Decode LDPC codewords by belief propagation (optic/comm/fec.py:684-758).

    ``llrs`` of shape ``(n_, numCodewords)`` -- ``(numCodewords, n_)`` with ``transposed`` -- float64 or float32, numpy or
    ``DeviceArray``; ``param.H``, ``param.maxIter`` (25), ``param.alg`` ('SPA'), ``param.prec`` (float32) as in the reference,
    ``param.engine`` ('auto').  Returns ``(decodedBits int8, outputLLRs prec, frameErrors int8)`` and, with ``returnIter``,
    ``lastIter`` (uint32): the first two of the kind and orientation of ``llrs``, the others numpy arrays of ``numCodewords``."""
    from .models import _state
    q = _prepare(llrs, param, transposed)
    lib = _lib.load()
    x, p = q["llrs"], q["params"]
    handle = _graph_handle(lib, _state["device"], q)
    on_dev = _dev.is_device(x)
    xp, keep = _dev.arg(x, x.dtype)
    post = _dev.empty(on_dev, x.shape, q["prec"])
    bits = _dev.empty(on_dev, x.shape, np.int8)
    fail = np.empty(p.numCodewords, dtype=np.int8)
    last = np.empty(p.numCodewords, dtype=np.uint32)
    rc = lib.ssf_ldpc_decode(_state["device"], handle, C.byref(p), xp, _dev.out_ptr(post), _dev.out_ptr(bits),
                             fail.ctypes.data_as(C.c_void_p), last.ctypes.data_as(C.c_void_p))
    _lib.raise_for(lib, None, rc)
    del keep
    return (bits, post, fail, last) if returnIter else (bits, post, fail)


def _prepare_llr(rxSymb, σ2, constSymb, bitMap, px):
    """The checks and host-side tables of calcLLR, without touching the library."""
    const = np.asarray(constSymb).reshape(-1).astype(np.complex128)
    M = int(const.size)
    if M < 2 or M > 1024 or M & (M - 1):
        raise ValueError(f"the constellation has {M} symbols: a power of two between 2 and 1024 is needed")
    b = M.bit_length() - 1
    bm = np.asarray(bitMap)
    if bm.shape != (M, b):
        raise ValueError(f"bitMap has shape {bm.shape}: ({M}, {b}) expected")
    if not np.all((bm == 0) | (bm == 1)):
        raise ValueError("bitMap must hold 0 and 1 only")
    p = np.asarray(px, dtype=np.float64).reshape(-1)
    if p.size != M:
        raise ValueError(f"px has {p.size} entries for {M} symbols")
    σ2 = float(σ2)
    if not (σ2 > 0 and np.isfinite(σ2)):
        raise ValueError(f"the noise variance must be positive and finite, not {σ2}")
    if _dev.is_device(rxSymb):
        if rxSymb.dtype.name not in _CPLX:
            raise TypeError(f"device array rxSymb has dtype {rxSymb.dtype.name}: complex128 or complex64 expected")
        x = rxSymb
    else:
        x = np.asarray(rxSymb)
        if x.dtype.name not in _CPLX:
            x = x.astype(np.complex128)
    if x.ndim != 1:
        raise ValueError("rxSymb must have one dimension")
    return dict(x=x, M=M, b=b, sigma2=σ2, table=np.ascontiguousarray(const).view(np.float64),
                bitmap=np.ascontiguousarray(bm, dtype=np.int32), px=np.ascontiguousarray(p))


def calcLLR(rxSymb, σ2, constSymb, bitMap, px):
    """LLRs of the bits of ``rxSymb`` for a circular AWGN channel (optic/comm/metrics.py:198-239): float64 of length
    ``len(rxSymb) log2 M`` in the order ``i b + indBit``, numpy or ``DeviceArray`` as ``rxSymb`` is."""
    from .models import _state
    q = _prepare_llr(rxSymb, σ2, constSymb, bitMap, px)
    lib = _lib.load()
    x = q["x"]
    xp, keep = _dev.arg(x, x.dtype)
    out = _dev.empty(_dev.is_device(x), (x.shape[0] * q["b"],), np.float64)
    rc = lib.ssf_calc_llr(_state["device"], x.shape[0], _lib.METRICS_DTYPES[x.dtype.name], q["M"], q["sigma2"],
                          q["table"].ctypes.data_as(C.POINTER(C.c_double)), _ip(q["bitmap"]),
                          q["px"].ctypes.data_as(C.POINTER(C.c_double)), xp, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


# ------------------------------------------------------------------ GF(2) on the host: rows packed eight bits to a byte
def _dense01(H, what="H"):
    """A 0/1 matrix in any accepted form (CSR-like, dense array, ``numpy.matrix``) as a dense uint8 array."""
    if all(hasattr(H, a) for a in ("indptr", "indices", "shape")):
        indptr, indices, m, n = _as_csr(H)
        D = np.zeros((m, n), dtype=np.uint8)
        D[np.repeat(np.arange(m), np.diff(indptr)), indices] = 1
        return D
    D = np.asarray(H)
    if D.ndim != 2:
        raise ValueError(f"{what} must be a matrix")
    if not np.all((D == 0) | (D == 1)):
        raise ValueError(f"{what} must hold 0 and 1 only")
    return np.ascontiguousarray(D, dtype=np.uint8)


def _col(Mp, j):
    """Column ``j`` of a matrix whose rows are packed (``np.packbits(M, axis=1)``), as 0 / 1."""
    return (Mp[:, j >> 3] >> (7 - (j & 7))) & 1


def _swap_rows(Mp, a, b):
    if a != b:
        Mp[[a, b]] = Mp[[b, a]]


def _swap_cols(Mp, a, b):
    d = (_col(Mp, a) ^ _col(Mp, b)).astype(np.uint8)                    # rows where the two columns differ: flip both bits
    Mp[:, a >> 3] ^= d << np.uint8(7 - (a & 7))
    Mp[:, b >> 3] ^= d << np.uint8(7 - (b & 7))


def _unpack(Mp, n):
    if n == 0:
        return np.zeros((Mp.shape[0], 0), dtype=np.uint8)
    return np.unpackbits(Mp, axis=1, count=n)


def _mul2(A, B):
    """``(A @ B) % 2`` of two 0/1 matrices: row i of the product is the XOR of the packed rows of B that row i of A names."""
    A, B = np.asarray(A, dtype=np.uint8), np.asarray(B, dtype=np.uint8)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=np.uint8)
    if 0 in out.shape or A.shape[1] == 0:
        return out
    Bp = np.packbits(B, axis=1)
    for i in range(A.shape[0]):
        out[i] = np.unpackbits(np.bitwise_xor.reduce(Bp[A[i] != 0], axis=0), count=B.shape[1])
    return out


def gaussElim(M):
    """Gaussian elimination over GF(2) in the reference's pivot order (fec.py:102-150): for every row the first column at or after
    ``lead`` with a one at or below the row, the topmost such row swapped up, every other row with a one there cleared."""
    M = _dense01(M, "M")
    rowCount, columnCount = M.shape
    Mp = np.packbits(M, axis=1)
    lead = 0
    for r in range(rowCount):
        if lead >= columnCount:
            break
        while True:
            nz = np.flatnonzero(_col(Mp[r:], lead))
            if nz.size:
                break
            lead += 1
            if lead == columnCount:
                break
        if lead == columnCount:
            break
        _swap_rows(Mp, r, r + int(nz[0]))
        rows = np.flatnonzero(_col(Mp, lead))
        Mp[rows[rows != r]] ^= Mp[r]
        lead += 1
    return _unpack(Mp, columnCount)


def par2gen(H):
    """``(G, colSwaps, Hm)`` of a parity-check matrix as the reference's ``par2gen`` returns them (fec.py:43-99): ``G = [I_k | P]``
    (uint8), the column order ``colSwaps`` (the columns of the reduced matrix with more than one entry, then those with exactly
    one) and ``Hm = H[:, colSwaps]``, the matrix the codewords of ``G`` satisfy."""
    H = _dense01(H)
    n = H.shape[1]
    k = n - H.shape[0]
    Hs = gaussElim(H)
    weight = Hs.sum(axis=0, dtype=np.int64)
    indP, indI = np.flatnonzero(weight > 1), np.flatnonzero(weight == 1)
    colSwaps = np.hstack((indP, indI))
    Hm = Hs[:, colSwaps]
    G = np.hstack((np.eye(k, dtype=np.uint8), Hm[:, 0:k].T))
    return G, colSwaps, H[:, colSwaps]


def inverseMatrixGF2(A):
    """``(Ainv, True)``, or ``(partial, False)`` for a singular matrix, by Gauss-Jordan in the reference's pivot order
    (fec.py:841-890)."""
    A = _dense01(A, "A")
    n = A.shape[0]
    if n == 0:
        return np.zeros((0, 0), dtype=np.uint8), True
    Ap, Ip = np.packbits(A, axis=1), np.packbits(np.eye(n, dtype=np.uint8), axis=1)
    for i in range(n):
        if not _col(Ap[i:i + 1], i)[0]:
            nz = np.flatnonzero(_col(Ap[i + 1:], i))
            if not nz.size:
                return _unpack(Ip, n), False
            j = i + 1 + int(nz[0])
            _swap_rows(Ap, i, j)
            _swap_rows(Ip, i, j)
        rows = np.flatnonzero(_col(Ap, i))
        rows = rows[rows != i]
        Ap[rows] ^= Ap[i]
        Ip[rows] ^= Ip[i]
    return _unpack(Ip, n), True


def triangularize(H):
    """``(triangH, rowPerm, colPerm)`` in the reference's order (fec.py:893-952): for every ``i`` the first one of the rows
    ``i ..`` in row-major order among the columns ``i ..`` is swapped to ``(i, i)`` and the ones below it are cleared."""
    H = _dense01(H)
    m, n = H.shape
    T = np.packbits(H, axis=1)
    rowPerm, colPerm = np.arange(m, dtype=np.int32), np.arange(n, dtype=np.int32)
    for i in range(min(m, n)):
        sub = T[i:, i >> 3:]
        has = ((sub[:, 0] & (0xFF >> (i & 7))) != 0) | sub[:, 1:].any(axis=1)
        nz = np.flatnonzero(has)
        if not nz.size:
            continue
        r = i + int(nz[0])
        c = i + int(np.argmax(np.unpackbits(T[r], count=n)[i:]))
        if r != i:
            _swap_rows(T, i, r)
            rowPerm[[i, r]] = rowPerm[[r, i]]
        if c != i:
            _swap_cols(T, i, c)
            colPerm[[i, c]] = colPerm[[c, i]]
        below = np.flatnonzero(_col(T[i + 1:], i)) + i + 1
        T[below] ^= T[i]
    return _unpack(T, n), rowPerm, colPerm


def triangP1P2(H):
    """``(P1, P2, Hm)`` of Richardson and Urbanke's encoder as the reference's ``triangP1P2`` returns them (fec.py:955-1016): ``P1``
    ``(g, k)`` and ``P2`` ``(m - g, k)`` uint8, ``Hm = H[:, colSwaps]``; ``(None, None, None)`` when ``T`` or ``D~`` is singular."""
    H = _dense01(H)
    triangH, _, colSwaps = triangularize(H)
    m, n = triangH.shape
    k = n - m
    idx = np.flatnonzero(triangH[:, -1] == 1)
    if not idx.size:
        return None, None, None
    g = m - int(idx.min()) - 1
    E, T = triangH[m - g:, n - (m - g):], triangH[0:m - g, n - (m - g):]
    A, B = triangH[0:m - g, 0:k], triangH[0:m - g, k:k + g]
    Cm, D = triangH[m - g:, 0:k], triangH[m - g:, k:k + g]
    T_inv, found = inverseMatrixGF2(T)
    if not found:
        return None, None, None
    X = _mul2(E, T_inv)
    C_tilde, D_tilde = _mul2(X, A) ^ Cm, _mul2(X, B) ^ D
    D_tilde_inv, found = inverseMatrixGF2(D_tilde)
    if not found:
        return None, None, None
    P1 = _mul2(D_tilde_inv, C_tilde)
    P2 = _mul2(T_inv, A ^ _mul2(B, P1))
    return P1, P2, H[:, colSwaps]


def writeAlist(H, filename):
    """Write a parity-check matrix in ALIST format, line for line as the reference does (fec.py:761-808); ``readAlist`` reads it
    back."""
    H = _dense01(H)
    m, n = H.shape
    varDegrees, checkDegrees = H.sum(axis=0, dtype=np.int64), H.sum(axis=1, dtype=np.int64)
    maxColDeg, maxRowDeg = int(varDegrees.max()), int(checkDegrees.max())
    with open(filename, "w") as f:
        f.write(f"{n} {m}\n")
        f.write(f"{maxColDeg} {maxRowDeg}\n")
        f.write(" ".join(str(int(d)) for d in varDegrees) + "\n")
        f.write(" ".join(str(int(d)) for d in checkDegrees) + "\n")
        for j in range(n):
            conn = (np.flatnonzero(H[:, j]) + 1).tolist()
            f.write(" ".join(str(i) for i in conn + [0] * (maxColDeg - len(conn))) + "\n")
        for i in range(m):
            conn = (np.flatnonzero(H[i, :]) + 1).tolist()
            f.write(" ".join(str(j) for j in conn + [0] * (maxRowDeg - len(conn))) + "\n")


def _csr_of_dense(D):
    rows, cols = np.nonzero(D)
    return _csr_from_pairs(rows, cols, D.shape)


def _generator_of(H):
    """``(G, CSR of Hm)`` of ``par2gen``, kept per matrix."""
    def build(Hc):
        G, _, Hm = par2gen(Hc)
        return G, _csr_of_dense(Hm)
    return _memo("par2gen", H, build)


def _triangular_of(H):
    """``(P1, P2, CSR of Hm)`` of ``triangP1P2``, or ``(None, None, None)``, kept per matrix."""
    def build(Hc):
        P1, P2, Hm = triangP1P2(Hc)
        return P1, P2, None if Hm is None else _csr_of_dense(Hm)
    return _memo("triang", H, build)


# ------------------------------------------------------------------ encodeLDPC
MAX_K_DENSE = _lib.ENC_MAX_K_DENSE
MAX_K_SPARSE = _lib.ENC_MAX_K_SPARSE
ENC_MODES = ("DVBS2", "IEEE_802.11nD2", "AR4JA")
_BIT_TYPES = ("uint8", "int8")

# what the eliminations made of the matrices seen last: (kind, shape, indptr, indices, value), found again by comparing the CSR
_ENC_SEEN = []


def _same(a, b):
    """``np.array_equal`` of two arrays; contiguous ones of one type are compared as 64-bit words (no boolean array of the size of
    the matrix in between: this comparison is most of what a call costs on the host)."""
    if a.shape != b.shape:
        return False
    if a.dtype != b.dtype or a.dtype.hasobject or not (a.flags.c_contiguous and b.flags.c_contiguous):
        return bool(np.array_equal(a, b))
    x, y = a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8)
    n8 = x.size & ~7
    return bool(np.array_equal(x[:n8].view(np.uint64), y[:n8].view(np.uint64)) and np.array_equal(x[n8:], y[n8:]))


def _seen(kind, shape, arrays):
    for pos, ent in enumerate(_ENC_SEEN):
        if ent[0] == kind and ent[1] == shape and all(_same(a, np.asarray(b)) for a, b in zip(ent[2], arrays)):
            _ENC_SEEN.append(_ENC_SEEN.pop(pos))
            return ent
    return None


def _keep(kind, shape, arrays, value):
    _ENC_SEEN.append((kind, shape, [np.array(a) for a in arrays], value))
    del _ENC_SEEN[:-4 * _SEEN_CAP]
    return value


def _memo(kind, H, build):
    """``build(H)`` once per matrix and kind ('triang', 'par2gen', 'A'): kept for the matrices seen last.  A CSR is first compared
    as it stands (a memcmp), as ``_code_of`` does; only an unknown one is checked and put in canonical order."""
    if all(hasattr(H, a) for a in ("indptr", "indices", "shape")) and getattr(H, "format", "csr") == "csr":
        data = getattr(H, "data", None)
        if data is None or bool(np.all(np.asarray(data) != 0)):
            ent = _seen(kind, (int(H.shape[0]), int(H.shape[1])), (np.asarray(H.indptr), np.asarray(H.indices)))
            if ent is not None:
                return ent[3]
    indptr, indices, m, n = _as_csr(H)
    ent = _seen(kind, (m, n), (indptr, indices))
    if ent is not None:
        return ent[3]
    return _keep(kind, (m, n), (indptr, indices), build(CSR(indptr, indices, (m, n))))


def _memo_dense(kind, blocks, build):
    """``build()`` once per tuple of dense matrices (``param.G``, or ``param.P1`` and ``param.P2``), compared value for value."""
    blocks = [np.asarray(b) for b in blocks]
    shape = tuple(b.shape for b in blocks)
    ent = _seen(kind, shape, blocks)
    return ent[3] if ent is not None else _keep(kind, shape, blocks, build())


def _pack_words(P):
    """Rows of a 0/1 matrix as little-endian 64-bit words: bit ``l`` of word ``w`` is column ``64 w + l``."""
    P = np.asarray(P, dtype=np.uint8)
    rows, k = P.shape
    W = (k + 63) // 64
    padded = np.zeros((rows, W * 64), dtype=np.uint8)
    padded[:, :k] = P
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").reshape(rows, W)


def _dense_plan(blocks, k, systematic):
    """The dense form of an encoder: one or two ``(rows, k)`` 0/1 blocks."""
    if k > MAX_K_DENSE:
        raise ValueError(f"k = {k}: the dense encoder takes at most {MAX_K_DENSE} message bits")
    words = [_pack_words(b) for b in blocks]
    h = hashlib.blake2b(digest_size=16)
    h.update(np.array([_lib.ENC_DENSE, k, int(bool(systematic))] + [w.shape[0] for w in words], dtype=np.int64).tobytes())
    for w in words:
        h.update(w.tobytes())
    rows = sum(w.shape[0] for w in words)
    return dict(form=_lib.ENC_DENSE, k=int(k), m1=words[0].shape[0], m2=words[1].shape[0] if len(words) > 1 else 0,
                systematic=int(bool(systematic)), nnz=0, blocks=words, digest=h.hexdigest(), full=rows + (k if systematic else 0))


def _generator_plan(G, systematic):
    def build():
        D = _dense01(G, "param.G")
        kG, nG = D.shape
        if systematic:
            if nG <= kG:
                raise ValueError(f"param.G of shape {D.shape}: a systematic generator matrix has more columns than rows")
            return _dense_plan([np.ascontiguousarray(D[:, kG:].T)], kG, True)
        return _dense_plan([np.ascontiguousarray(D.T)], kG, False)
    return _memo_dense(("G", bool(systematic)), [G], build)


def _parity_plan(P1, P2):
    return _memo_dense("P1P2", [P1, P2], lambda: _dense_plan([_dense01(P1, "param.P1"), _dense01(P2, "param.P2")], np.asarray(P1).shape[1], True))


def _accumulator_plan(H, n):
    """The sparse form: the CSR of ``A = H[:, :k]``, ``k = n - m`` (fec.py:205-212)."""
    def build(Hc):
        m, nH = Hc.shape
        k = n - m
        if k < 1 or k > nH:
            raise ValueError(f"param.n = {n} with a parity-check matrix of shape {Hc.shape}: k = n - m = {k} message bits")
        if k > MAX_K_SPARSE or m > _lib.ENC_MAX_M_SPARSE:
            raise ValueError(f"k = {k}, m = {m}: the DVB-S2 encoder takes at most {MAX_K_SPARSE} message bits and "
                             f"{_lib.ENC_MAX_M_SPARSE} checks")
        keep = Hc.indices < k
        indptr = np.zeros(m + 1, dtype=np.int64)
        np.cumsum(np.bincount(np.repeat(np.arange(m), np.diff(Hc.indptr))[keep], minlength=m), out=indptr[1:])
        indptr = indptr.astype(np.int32)
        indices = np.ascontiguousarray(Hc.indices[keep], dtype=np.int32)
        h = hashlib.blake2b(digest_size=16)
        h.update(np.array([_lib.ENC_SPARSE, k, m], dtype=np.int64).tobytes())
        h.update(indptr.tobytes())
        h.update(indices.tobytes())
        return dict(form=_lib.ENC_SPARSE, k=int(k), m1=int(m), m2=0, systematic=1, nnz=int(indices.size), indptr=indptr, indices=indices,
                    digest=h.hexdigest(), full=int(k + m))
    return _memo(("A", int(n)), H, build)


def _bits_array(bits):
    if _dev.is_device(bits):
        if bits.dtype.name not in _BIT_TYPES:
            raise TypeError(f"device array bits has dtype {bits.dtype.name}: uint8 or int8 expected")
        return bits
    b = np.asarray(bits)
    if b.dtype != np.bool_ and not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"bits has dtype {b.dtype.name}: an integer or bool array is needed")
    if not np.all((b == 0) | (b == 1)):
        raise ValueError("bits must hold 0 and 1 only")
    return np.ascontiguousarray(b, dtype=np.uint8)


def _prepare_encode(bits, param, transposed=False):
    """Every check, every write-back and every host-side matrix of an encode, without touching the library: a dict with ``bits``
    (2-D), ``plan`` (the encoder's form and arrays), ``params`` (``_lib.EncodeParams``), ``k``, ``n_out``, ``N``."""
    mode = getattr(param, "mode", "DVBS2")
    n = getattr(param, "n", 64800)
    R = getattr(param, "R", "4/5")
    H = getattr(param, "H", None)
    G = getattr(param, "G", None)
    systematic = getattr(param, "systematic", True)
    P1 = getattr(param, "P1", None)
    P2 = getattr(param, "P2", None)
    path = getattr(param, "path", None)
    if mode not in ENC_MODES:
        raise ValueError(f"Unsupported mode: {mode!r}. Supported modes are: DVBS2, IEEE_802.11nD2, AR4JA.")
    if int(n) != n or n < 1:
        raise ValueError(f"n = {n}: a codeword length is needed")
    n = int(n)
    bits = _bits_array(bits)
    if bits.ndim != 2:
        raise ValueError("bits must have two dimensions: (k, N), or (N, k) with transposed=True")
    k_in, N = (bits.shape[1], bits.shape[0]) if transposed else (bits.shape[0], bits.shape[1])
    if N < 1 or N > MAX_CODEWORDS or k_in < 1:
        raise ValueError(f"bits of shape {tuple(bits.shape)}: between 1 and {MAX_CODEWORDS} messages of at least one bit are needed")

    given = P1 is not None and P2 is not None and mode == "IEEE_802.11nD2"
    uses_G = G is not None and mode == "AR4JA"
    if H is None and not (given or uses_G):
        if path is None:
            raise ValueError("param.H is None and param.path names no folder of ALIST files: a parity-check matrix is needed")
        H = readAlist(os.path.join(path, f"LDPC_{mode}_{n}b_R{R[0]}{R[2]}.txt"))
        param.H = H

    if mode == "DVBS2":
        plan, n_out = _accumulator_plan(H, n), n
    elif given:
        plan = _parity_plan(P1, P2)
        n_out = plan["full"]
    elif mode == "IEEE_802.11nD2":
        tri = _triangular_of(H)
        if tri[0] is None:
            if G is None:
                G, param.H = _generator_of(H)
                param.G = G
            plan = _generator_plan(G, systematic)
            n_out = min(n, plan["full"])
        else:
            param.P1, param.P2 = tri[0], tri[1]
            param.H = tri[2]
            plan = _parity_plan(tri[0], tri[1])
            n_out = plan["full"]
    else:
        if G is None:
            G, param.H = _generator_of(H)
            param.G = G
        plan = _generator_plan(G, systematic)
        n_out = min(n, plan["full"])
    if k_in != plan["k"]:
        raise ValueError(f"bits of shape {tuple(bits.shape)}: the code takes k = {plan['k']} message bits per codeword"
                         + ("" if transposed else " (rows; transposed=True takes them along the second axis)"))
    params = _lib.EncodeParams(numCodewords=int(N), n=int(n_out), transposed=int(bool(transposed)), reserved=0)
    return dict(bits=bits, plan=plan, params=params, k=plan["k"], n_out=int(n_out), N=int(N))


# encoder handles of ssf_ldpc_encoder_create by (device, digest of the plan): a code is uploaded once, as _GRAPHS keeps the graphs
_ENCODERS = {}


def encoder_cache_info():
    """(device, digest) keys of the encoders held on the device, oldest first."""
    return list(_ENCODERS)


def release_encoders():
    """Free every cached encoder."""
    lib = _lib.load()
    while _ENCODERS:
        lib.ssf_ldpc_encoder_destroy(_ENCODERS.pop(next(iter(_ENCODERS))))


def _encoder_handle(lib, device, plan):
    key = (device, plan["digest"])
    handle = _ENCODERS.pop(key, None)
    if handle is None:
        desc = _lib.EncoderDesc(form=plan["form"], k=plan["k"], m1=plan["m1"], m2=plan["m2"], systematic=plan["systematic"], nnz=plan["nnz"])
        handle = C.c_void_p()
        if plan["form"] == _lib.ENC_DENSE:
            b = plan["blocks"]
            rc = lib.ssf_ldpc_encoder_create(device, C.byref(desc), b[0].ctypes.data_as(C.c_void_p),
                                             b[1].ctypes.data_as(C.c_void_p) if len(b) > 1 else None, None, None, C.byref(handle))
        else:
            rc = lib.ssf_ldpc_encoder_create(device, C.byref(desc), None, None, _ip(plan["indptr"]), _ip(plan["indices"]), C.byref(handle))
        _lib.raise_for(lib, None, rc)
        while len(_ENCODERS) >= _GRAPH_CAP:
            lib.ssf_ldpc_encoder_destroy(_ENCODERS.pop(next(iter(_ENCODERS))))
    _ENCODERS[key] = handle                                             # most recently used last
    return handle


def encodeLDPC(bits, param, *, transposed=False):
    """Encode messages with an LDPC code (optic/comm/fec.py:153-251).

    ``bits`` of shape ``(k, N)`` -- ``(N, k)`` with ``transposed`` -- numpy integer / bool, or a ``DeviceArray`` of uint8 / int8;
    ``param.mode`` ('DVBS2'), ``n`` (64800), ``R`` ('4/5'), ``H``, ``G``, ``systematic`` (True), ``P1``, ``P2``, ``path`` as in the
    reference, which this follows branch by branch and write-back by write-back.  Returns the codewords, uint8 of shape ``(n, N)``
    -- ``(N, n)`` -- of the kind ``bits`` is."""
    from .models import _state
    q = _prepare_encode(bits, param, transposed)
    lib = _lib.load()
    x, p = q["bits"], q["params"]
    handle = _encoder_handle(lib, _state["device"], q["plan"])
    on_dev = _dev.is_device(x)
    xp, keep = _dev.arg(x, x.dtype)
    out = _dev.empty(on_dev, (q["N"], q["n_out"]) if transposed else (q["n_out"], q["N"]), np.uint8)
    rc = lib.ssf_ldpc_encode(_state["device"], handle, C.byref(p), xp, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out


# ------------------------------------------------------------------ modulateGray
def _prepare_mod(bits, M, constType):
    """The checks and the table of modulateGray, without touching the library."""
    from .wdm_tx import grayMapping
    if constType == "ook":
        M = 2                                                           # (the reference warns and does the same)
        const = np.arange(0, 2, dtype=np.float32)
    else:
        if int(M) != M or M < 2 or M > 1024 or int(M) & (int(M) - 1):
            raise ValueError(f"M = {M}: a power of two between 2 and 1024 is needed")
        if constType not in ("qam", "psk", "pam"):
            raise ValueError(f"constType must be 'qam', 'psk', 'pam' or 'ook', not {constType!r}")
        const = grayMapping(int(M), constType)
    M = int(M)
    b = M.bit_length() - 1
    bits = _bits_array(bits)
    if bits.ndim != 1:
        raise ValueError("bits must have one dimension")
    if bits.shape[0] < b or bits.shape[0] % b:
        raise ValueError(f"{bits.shape[0]} bits are no whole number of symbols of {b} bits")
    return dict(bits=bits, M=M, b=b, nsymb=bits.shape[0] // b, table=np.ascontiguousarray(const.astype(np.complex128)).view(np.float64))


def modulateGray(bits, M, constType):
    """Map bits to Gray-labelled constellation symbols (optic/comm/modulation.py:334-366): ``bits`` 1-D of ``nSymb log2 M`` values,
    the first bit of a symbol the most significant, numpy integer / bool or a ``DeviceArray`` of uint8 / int8; returns ``nSymb``
    complex128 symbols of the unnormalised constellation, numpy or ``DeviceArray`` as ``bits`` is."""
    from .models import _state
    q = _prepare_mod(bits, M, constType)
    lib = _lib.load()
    x = q["bits"]
    xp, keep = _dev.arg(x, x.dtype)
    out = _dev.empty(_dev.is_device(x), (q["nsymb"],), np.complex128)
    rc = lib.ssf_modulate(_state["device"], q["nsymb"], q["M"], q["table"].ctypes.data_as(C.POINTER(C.c_double)), xp, _dev.out_ptr(out))
    _lib.raise_for(lib, None, rc)
    del keep
    return out
