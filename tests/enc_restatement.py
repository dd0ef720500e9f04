"""An independent numpy restatement of the encoders and of modulateGray, written from the reference's definitions
(optic/comm/fec.py:254-344 encodeDVBS2 and encoder, 1019-1072 encodeTriang; optic/comm/modulation.py:35-198, 334-366) and not
from the kernels: integer matrix products reduced modulo 2, ``np.bitwise_xor.accumulate`` for the accumulator and ``const[index]``
for the mapper.  tests/test_enc_restatement.py holds it to every recorded fixture; the shape tests hold the kernels to it where
no fixture reaches."""
import numpy as np


def product(P, bits):
    """``(P @ bits) % 2``: P (rows, k), bits (k, N)."""
    return ((np.asarray(P, dtype=np.int64) @ np.asarray(bits, dtype=np.int64)) % 2).astype(np.uint8)


def encode_generator(G, bits, systematic=True, n=None):
    """``encoder(G, bits, systematic)[0:n]``: every row of G^T times the message; a systematic code copies the message instead of
    multiplying it by the first k rows."""
    G = np.asarray(G)
    cw = product(G.T, bits)
    if systematic:
        cw[:G.shape[0]] = bits
    return cw[:n]


def encode_triang(P1, P2, bits):
    return np.vstack((np.asarray(bits, dtype=np.uint8), product(P1, bits), product(P2, bits)))


def encode_dvbs2(A, bits):
    """``encodeDVBS2``: the parities of the rows of A, then the running XOR along the checks."""
    return np.vstack((np.asarray(bits, dtype=np.uint8), np.bitwise_xor.accumulate(product(A, bits), axis=0)))


def gray_table(M, constType):
    """The constellation indexed by the integer its Gray label spells (grayMapping): point i of the reference's own point order
    carries the label ``i ^ (i >> 1)``; single precision, as the reference stores it."""
    i = np.arange(M)
    if constType == "ook":
        M, i = 2, np.arange(2)
        pts = i.astype(np.float32)
    elif constType == "pam":
        pts = (2 * i - (M - 1)).astype(np.float32)
    elif constType == "psk":
        pts = np.exp(1j * np.arange(0, 2 * np.pi, 2 * np.pi / M)).astype(np.complex64)
    elif constType == "qam":
        side = int(round(np.sqrt(M)))
        assert side * side == M
        row, col = i // side, i % side
        col = np.where(row % 2 == 1, side - 1 - col, col)                # every other row runs right to left
        pts = ((2 * col - (side - 1)) + 1j * ((side - 1) - 2 * row)).astype(np.complex64)
    else:
        raise ValueError(constType)
    table = np.empty_like(pts)
    table[i ^ (i >> 1)] = pts
    return table


def modulate(bits, M, constType):
    """``const[bitarray2dec(bits.reshape(-1, b).T)]``, the first bit of a symbol the most significant."""
    table = gray_table(M, constType)
    b = int(np.log2(len(table)))
    index = np.asarray(bits, dtype=np.int64).reshape(-1, b) @ (1 << np.arange(b - 1, -1, -1))
    return table[index]
