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
  ``DeviceArray`` has no ``.T``);
* ``returnIter=True`` also returns ``lastIter`` (uint32), which the reference computes and only logs;
* ``frameErrors`` and ``lastIter`` are numpy arrays whatever the input is (``numCodewords`` values);
* an unsupported ``alg`` or a missing ``H`` raises (the reference logs an error and fails later);
* ``calcLLR`` computes in double whatever it is given (the reference's arithmetic is single precision when ``rxSymb`` and
  ``constSymb`` are both complex64), and sums ``p0`` / ``p1`` over the constellation in ascending order.

Not here: ``encodeLDPC``, ``calcExtrLLR``, layered schedules, Hamming codes.
"""
import ctypes as C
import hashlib

import numpy as np

from . import _lib
from . import device as _dev

__all__ = ["calcLLR", "decodeLDPC", "readAlist"]

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
