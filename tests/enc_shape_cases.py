"""The shape rows of the encoder tests: small seeded codes at every size at which the kernels of engine_enc.hip take another path,
with what tests/enc_restatement.py makes of them.  The sizes follow the kernels' geometry as ``_lib`` exports it: the codeword
tile and the rows per workgroup of the dense kernel, a wave's and a workgroup's span of the accumulator's scan, the lanes of a
workgroup of the mapper.  tests/test_enc_emu.py walks every row with the emulator, tests/test_gpu_enc_shapes.py on the GPU; both
compare with ``np.array_equal``.

Dense rows reach the kernel through the public interface: a systematic ``G = [I | P^T]`` under mode 'AR4JA', ``P1`` / ``P2`` given
under 'IEEE_802.11nD2' (two blocks), an arbitrary ``G`` with ``systematic=False``.  Accumulator rows are ``H = [A | dual diagonal]``
under 'DVBS2'."""
from collections import namedtuple

import numpy as np

import enc_restatement as er
from enc_cases import Param
from opticommpy_amd import _lib

TILE, ROWS, WAVE, SPAN, BLOCK = _lib.ENC_TILE, _lib.ENC_ROWS, _lib.ENC_WAVE_SPAN, _lib.ENC_SPAN, _lib.ENC_BLOCK
CARRY = _lib.ENC_CARRY_SPAN

# kind: 'sys' (systematic G), 'two' (P1 of m1 rows and P2), 'gt' (systematic=False; rows = n), 'acc' (DVB-S2);
# special: 'zero_one' (an all-zero and an all-one row of P), 'empty' (empty rows of A, the first and the last among them),
# 'run' (one parity, then empty rows: a run of ones whose carry crosses every wave and every span), 'crop' (n below the full length)
Row = namedtuple("Row", "id kind k rows N m1 special seed")


def _dense_rows():
    rows, seed = [], 100
    base = dict(k=65, rows=ROWS + 1, N=TILE + 1)
    for k in (1, 63, 64, 65, 129):
        rows.append(dict(base, k=k))
    for r in (1, ROWS - 1, ROWS, ROWS + 1):
        rows.append(dict(base, rows=r))
    for N in (1, TILE - 1, TILE, TILE + 1):
        rows.append(dict(base, N=N))
    out = []
    for r in rows:
        seed += 1
        out.append(Row(f"sys_k{r['k']}_r{r['rows']}_N{r['N']}", "sys", r["k"], r["rows"], r["N"], 0, "", seed))
    out.append(Row("sys_k129_r2R1_N2T1", "sys", 129, 2 * ROWS + 1, 2 * TILE + 1, 0, "", 150))       # several workgroups each way
    out.append(Row("sys_zero_one_rows", "sys", 130, ROWS + 2, 5, 0, "zero_one", 151))
    out.append(Row("sys_cropped", "sys", 70, 40, 5, 0, "crop", 152))                                # the puncturing of AR4JA
    out.append(Row("two_m1_1", "two", 65, ROWS + 1, TILE + 1, 1, "", 153))                          # P1 of one row, P2 of the rest
    out.append(Row("two_m1_7_k64", "two", 64, 30, 3, 7, "", 154))
    out.append(Row("gt_k65", "gt", 65, ROWS + 1, TILE + 1, 0, "", 155))                             # systematic=False
    out.append(Row("gt_k1_r1_N1", "gt", 1, 1, 1, 0, "", 156))
    return out


def _accumulator_rows():
    out, seed = [], 200
    for m in (1, 63, 64, 65, WAVE + 1, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3):
        if m in [r.rows for r in out]:
            continue
        seed += 1
        out.append(Row(f"acc_m{m}", "acc", 70, m, 3, 0, "", seed))
    out.append(Row("acc_empty_rows", "acc", 129, SPAN + WAVE + 2, 4, 0, "empty", 250))
    out.append(Row("acc_run_of_ones", "acc", 64, 2 * SPAN + 3, 2, 0, "run", 251))
    # 64 ballots of 64 checks get their carries from one ballot of totals: one check less, exactly, one more, and a run of ones across
    for m in (CARRY - 1, CARRY, CARRY + 1):
        out.append(Row(f"acc_m{m}", "acc", 70, m, 2, 0, "", 260 + m - CARRY))
    out.append(Row("acc_run_across_carry_span", "acc", 64, CARRY + SPAN + 1, 2, 0, "run", 263))
    out.append(Row("acc_k1_N17", "acc", 1, 5, 17, 0, "", 252))
    return out


ROWS_DENSE = _dense_rows()
ROWS_ACC = _accumulator_rows()
ENC_ROWS = ROWS_DENSE + ROWS_ACC

ModRow = namedtuple("ModRow", "id M constType nsymb dtype seed")
MOD_ROWS = [ModRow(f"psk2_n{n}", 2, "psk", n, "uint8", 300 + i) for i, n in enumerate((1, 63, 64, 65, 3 * BLOCK + 1))] + \
           [ModRow(f"qam1024_n{n}", 1024, "qam", n, "uint8", 310 + i) for i, n in enumerate((1, 63, 64, 65, 3 * BLOCK + 1))] + \
           [ModRow("qam16_int8", 16, "qam", 3 * BLOCK + 1, "int8", 320), ModRow("qam1024_int8", 1024, "qam", 65, "int8", 321),
            ModRow("ook_n65", 2, "ook", 65, "uint8", 322), ModRow("pam8_n65", 8, "pam", 65, "int8", 323)]


def make(row):
    """``(param, bits, want)`` of a row: the parameters for ``encodeLDPC``, the messages ``(k, N)`` and the restatement's codewords."""
    rng = np.random.default_rng(row.seed)
    bits = rng.integers(0, 2, size=(row.k, row.N)).astype(np.uint8)
    if row.N > 1:
        bits[:, -1] = 1                                                 # an all-one message among them
    if row.kind == "acc":
        m, k = row.rows, row.k
        A = (rng.random((m, k)) < min(0.5, 4.0 / k + 0.05)).astype(np.uint8)
        if row.special == "empty":
            A[[0, 1, WAVE - 1, WAVE, SPAN, m - 1]] = 0
        if row.special == "run":
            A[:] = 0
            A[0, 0] = 1
            bits[0, :] = 1
        D = np.eye(m, dtype=np.uint8) + np.eye(m, k=-1, dtype=np.uint8)
        prm = Param(mode="DVBS2", n=k + m, H=np.hstack((A, D)))
        return prm, bits, er.encode_dvbs2(A, bits)
    P = rng.integers(0, 2, size=(row.rows, row.k)).astype(np.uint8)
    if row.special == "zero_one":
        P[[0, ROWS]] = 0
        P[[1, ROWS + 1]] = 1
    if row.kind == "sys":
        G = np.hstack((np.eye(row.k, dtype=np.uint8), P.T))
        n = row.k + row.rows // 2 if row.special == "crop" else row.k + row.rows
        return Param(mode="AR4JA", n=n, G=G), bits, er.encode_generator(G, bits, True, n)
    if row.kind == "gt":
        G = np.ascontiguousarray(P.T)                                   # (k, rows): no identity anywhere
        return Param(mode="AR4JA", n=row.rows, G=G, systematic=False), bits, er.encode_generator(G, bits, False, row.rows)
    P1, P2 = P[:row.m1], P[row.m1:]
    return Param(mode="IEEE_802.11nD2", n=row.k + row.rows, P1=P1, P2=P2), bits, er.encode_triang(P1, P2, bits)


def check_conditions(row, prm, bits, want):
    """A row must reach what its name promises."""
    full = row.rows if row.kind == "gt" else row.k + row.rows
    assert want.dtype == np.uint8 and want.shape == ((row.k + row.rows // 2 if row.special == "crop" else full), row.N)
    if row.kind != "gt":
        assert np.array_equal(want[:row.k], bits)
    if row.special == "zero_one":
        assert not want[row.k].any() and not want[row.k + ROWS].any()
        assert np.array_equal(want[row.k + 1], bits.sum(axis=0) % 2) and np.array_equal(want[row.k + ROWS + 1], bits.sum(axis=0) % 2)
    if row.special == "run":
        assert want[row.k:].all() and row.rows > 2 * SPAN                # the carry is 1 across every wave and span boundary
    if row.special == "empty":
        A = np.asarray(prm.H)[:, :row.k]
        empty = np.flatnonzero(A.sum(axis=1) == 0)
        assert {0, WAVE, SPAN, row.rows - 1} <= set(empty.tolist())
        assert want[row.k:].any() and not want[row.k:].all()
    if row.kind == "acc" and not row.special and row.rows > 8 and row.k > 8:
        assert want[row.k:].any() and not want[row.k:].all()


def mod_make(row):
    """``(bits, want)`` of a mapper row: the bits in the row's dtype and the restatement's symbols as complex128."""
    b = 1 if row.constType == "ook" else int(np.log2(row.M))
    bits = np.random.default_rng(row.seed).integers(0, 2, size=row.nsymb * b).astype(row.dtype)
    return bits, er.modulate(bits, row.M, row.constType).astype(np.complex128)
