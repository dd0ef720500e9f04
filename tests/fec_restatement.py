"""A numpy statement of the reference's soft-decision FEC: ``calcLLR`` (optic/comm/metrics.py:198-239) and the flooding
belief-propagation decoders behind ``decodeLDPC`` (optic/comm/fec.py:347-758), vectorised over nodes and codewords.  The loops
run over the position inside a node (the d-th edge of every check, the d-th edge of every variable), so every sum and product is
taken in the reference's order and in ``prec``:

* the edges of check ``c`` are its columns in ascending order; a variable sums ``llr + sum C->V`` over its edges in ascending
  check index, left to right, and sends that sum minus the edge's own message;
* MSA: first minimum (strict ``<``), second minimum, product of signs with ``val >= 0 -> +1`` and anything else, NaN included,
  ``-1`` (fec.py:609, 622): bit-equal to the reference.  A check of degree 1 sends +-inf, its variable answers ``inf - inf``;
* SPA: for every edge the product of ``tanh(x / 2)`` over the check's other edges in ascending order starting from 1.0 (the
  reference's O(d_c^2) product), clipped to +-0.999999 where the message is 2 atanh(0.999999) evaluated in double, ``2 atanh``
  otherwise.  The device forms the same products from prefix and suffix products: another rounding.

tests/test_fec_restatement.py pins this file to the reference's recorded results; the GPU tests then use it for graphs too large
to store."""
import numpy as np

CLIP_LLR = 200
CLIP_PROD = 0.999999


def padded(offsets, values):
    """(index matrix, validity mask) of a ragged list: row r holds values[offsets[r]:offsets[r + 1]], padded with 0."""
    deg = np.diff(offsets)
    pos = np.arange(int(deg.max()))[None, :]
    valid = pos < deg[:, None]
    idx = np.where(valid, offsets[:-1, None] + pos, 0)
    return (idx if values is None else np.where(valid, values[idx], 0)), valid


def edge_maps(indptr, indices, n):
    """check_offsets, var_offsets, var_edge_indices as fec.py:388-411 builds them, by the same walk over the checks."""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    var_offsets = np.zeros(n + 1, dtype=np.int32)
    var_offsets[1:] = np.cumsum(np.bincount(indices, minlength=n))
    var_edge_indices = np.zeros(len(indices), dtype=np.int32)
    count = np.zeros(n, dtype=np.int64)
    for e, v in enumerate(indices):
        var_edge_indices[var_offsets[v] + count[v]] = e
        count[v] += 1
    return indptr.astype(np.int32), var_offsets, var_edge_indices


def decode(indptr, indices, shape, llrs, alg="SPA", maxIter=25, prec=np.float32):
    """``decodeLDPC`` for ``llrs`` of shape (n_, numCodewords): (decodedBits int8, outputLLRs prec, frameErrors int8, lastIter
    uint32)."""
    prec = np.dtype(prec).type
    m, n = int(shape[0]), int(shape[1])
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    llrs = np.clip(np.asarray(llrs), -CLIP_LLR, CLIP_LLR)
    n_, ncw = llrs.shape
    if n_ < n:
        llrs = np.pad(llrs, ((0, n - n_), (0, 0)), mode="constant")
    llr = llrs.astype(prec)
    E = len(indices)
    cidx, cvalid = padded(indptr, None)                                  # (m, dc): edge ids of every check
    var_offsets = np.concatenate(([0], np.cumsum(np.bincount(indices, minlength=n))))
    vidx, vvalid = padded(var_offsets, np.argsort(indices, kind="stable"))   # (n, dv): edge ids of every variable, ascending check
    cvar = np.where(cvalid, indices[cidx], 0)                            # (m, dc): variables of every check
    dc, dv = cidx.shape[1], vidx.shape[1]
    one, two, sat = prec(1.0), prec(2.0), prec(2.0 * np.arctanh(CLIP_PROD))

    v2c = llr[indices, :]                                                # (E, ncw)
    c2v = np.zeros((E, ncw), dtype=prec)
    final = np.zeros((n, ncw), dtype=prec)
    fail = np.ones(ncw, dtype=np.int8)
    last = np.full(ncw, maxIter - 1, dtype=np.uint32)
    active = np.ones(ncw, dtype=bool)
    for it in range(maxIter):
        a = np.flatnonzero(active)
        x = v2c[:, a]
        if alg == "SPA":
            t = np.tanh(x / two)
            out = np.zeros_like(x)
            for i in range(dc):
                prod = np.full((m, len(a)), one, dtype=prec)
                for j in range(dc):
                    if j != i:
                        prod = np.where(cvalid[:, j, None], prod * t[cidx[:, j]], prod)
                with np.errstate(divide="ignore", invalid="ignore"):
                    msg = two * np.arctanh(prod)
                msg = np.where(prod >= prec(CLIP_PROD), sat, np.where(prod <= prec(-CLIP_PROD), -sat, msg)).astype(prec)
                rows = cvalid[:, i]
                out[cidx[rows, i]] = msg[rows]
        elif alg == "MSA":
            min1 = np.full((m, len(a)), np.inf, dtype=prec)
            min2 = np.full((m, len(a)), np.inf, dtype=prec)
            arg = np.full((m, len(a)), -1, dtype=np.int64)
            sign = np.ones((m, len(a)), dtype=np.int64)
            for j in range(dc):
                ok = cvalid[:, j, None]
                val = x[cidx[:, j]]
                mag = np.abs(val)
                sign = np.where(ok & ~(val >= 0), -sign, sign)            # fec.py:609: 1 if val >= 0 else -1, so NaN is negative
                lower = ok & (mag < min1)
                second = ok & ~lower & (mag < min2)
                min2 = np.where(lower, min1, np.where(second, mag, min2))
                min1 = np.where(lower, mag, min1)
                arg = np.where(lower, j, arg)
            out = np.zeros_like(x)
            for j in range(dc):
                val = x[cidx[:, j]]
                s = np.where(val >= 0, sign, -sign)
                mag = np.where(arg == j, min2, min1)
                rows = cvalid[:, j]
                out[cidx[rows, j]] = (s * mag).astype(prec)[rows]
        else:
            raise ValueError(alg)
        c2v[:, a] = out
        total = llr[:, a].copy()
        for k in range(dv):
            total = np.where(vvalid[:, k, None], total + out[vidx[:, k]], total)
        nxt = np.zeros_like(x)
        for k in range(dv):
            rows = vvalid[:, k]
            nxt[vidx[rows, k]] = (total - out[vidx[:, k]])[rows]
        v2c[:, a] = nxt
        final[:, a] = total
        bits = (total < 0).astype(np.uint8)
        parity = np.zeros((m, len(a)), dtype=np.uint8)
        for j in range(dc):
            parity ^= np.where(cvalid[:, j, None], bits[cvar[:, j]], 0).astype(np.uint8)
        good = ~parity.any(axis=0)
        fail[a[good]] = 0
        last[a[good]] = it
        active[a[good]] = False
        if not active.any():
            break
    out_llr = final[:n_]
    decoded = ((-np.sign(out_llr) + 1) // 2).astype(np.int8)
    return decoded, out_llr, fail, last


def calc_llr(rxSymb, sigma2, constSymb, bitMap, px):
    """``calcLLR``: p0 and p1 summed over the constellation in ascending order."""
    rx = np.asarray(rxSymb).astype(np.complex128)
    const = np.asarray(constSymb).reshape(-1).astype(np.complex128)
    bitMap, px = np.asarray(bitMap), np.asarray(px, dtype=np.float64).reshape(-1)
    b = bitMap.shape[1]
    p0, p1 = np.zeros((len(rx), b)), np.zeros((len(rx), b))
    for mth in range(len(const)):
        prob = np.exp((-np.abs(rx - const[mth]) ** 2) / sigma2) * px[mth]
        p0 += np.where(bitMap[mth] == 0, prob[:, None], 0.0)
        p1 += np.where(bitMap[mth] == 1, prob[:, None], 0.0)
    with np.errstate(divide="ignore"):
        return (np.log(p0) - np.log(p1)).reshape(-1)
