"""Literal shape rows of the syncDataSequences / movingAverage / bert kernels, run by the host emulator (tests/test_syncdata_emu.py)
and on the GPU (tests/test_gpu_syncdata.py) against tests/syncdata_restatement.py.

B is the rows of a column one workgroup of the extraction scans (1024), T the outputs per workgroup of the windowed mean (1024), 256
the lanes of a workgroup of bert's passes and 1024 their most workgroups; the rows sit at those edges (the constants are asserted
against the package in the tests, so that the rows follow the build).  Rows are a few hundred to a few thousand samples; the two
bert rows at 256 * 1024 samples are where the grid-stride loop starts to take a second round."""
import numpy as np

B, T, BLOCK, BERT_BLOCKS = 1024, 1024, 256, 1024

# ---- extraction: x[i, m] is non-zero where i % SpS == 0, except every `zero_every`-th symbol (0: none); n_out = n // SpS + 1
#      kept = ceil(n / SpS) minus the zero symbols
EXTRACT_ROWS = [
    dict(name="kept_B-1", n=B - 1, modes=1, SpS=1, zero_every=0, seed=1),
    dict(name="kept_B", n=B, modes=1, SpS=1, zero_every=0, seed=2),
    dict(name="kept_B+1", n=B + 1, modes=2, SpS=1, zero_every=0, seed=3),
    dict(name="kept_2B+1", n=2 * B + 1, modes=1, SpS=1, zero_every=0, seed=4),
    dict(name="sps2_kept_B+1", n=2 * B + 2, modes=2, SpS=2, zero_every=0, seed=5),             # kept = n_out - 1
    dict(name="sps2_fills_every_row", n=2 * B + 1, modes=1, SpS=2, zero_every=0, seed=6),       # kept = n_out
    dict(name="sps16", n=16 * 130 + 5, modes=1, SpS=16, zero_every=0, seed=7),
    dict(name="zeros_among_symbols", n=3000, modes=2, SpS=2, zero_every=7, seed=8),
    dict(name="eight_modes", n=B + 300, modes=8, SpS=2, zero_every=5, seed=9),
    dict(name="two_rows", n=2, modes=1, SpS=1, zero_every=0, seed=10),
    dict(name="nothing_kept_in_a_workgroup", n=3 * B, modes=1, SpS=1, zero_every=0, seed=11, blank=(B, 2 * B)),
]


def extract_input(row):
    """(n, modes) complex128; column m is shifted by m rows so that the columns' counts differ."""
    rng = np.random.default_rng(row["seed"])
    n, m = row["n"], row["modes"]
    x = np.zeros((n, m), dtype=np.complex128)
    for k in range(m):
        idx = np.arange(0, n, row["SpS"])
        v = rng.normal(size=len(idx)) + 1j * rng.normal(size=len(idx))
        v[np.abs(v) == 0] = 1.0
        if row["zero_every"]:
            v[(k + 1)::row["zero_every"]] = 0.0
        x[idx, k] = v
    if "blank" in row:
        x[row["blank"][0]:row["blank"][1]] = 0.0
    return x


# ---- tiling: period P = nTx * SpS; rows in every relation of len(rx) to P, and every dtype pair
def _tiling():
    rows = []
    nTx, SpS = 37, 3
    P = nTx * SpS
    for label, n_rx in (("P-1", P - 1), ("P", P), ("P+1", P + 1), ("2P", 2 * P), ("2P+3", 2 * P + 3), ("short", P // 2)):
        rows.append(dict(name=f"len_{label}", nTx=nTx, SpS=SpS, n_rx=n_rx, modes=2, rx_dtype="complex128", tx_dtype="complex128"))
    rows.append(dict(name="two_symbols", nTx=2, SpS=4, n_rx=29, modes=1, rx_dtype="float64", tx_dtype="float64"))
    rows.append(dict(name="unstuffed", nTx=50, SpS=1, n_rx=260, modes=8, rx_dtype="complex128", tx_dtype="complex128"))
    rows.append(dict(name="beyond_one_workgroup", nTx=700, SpS=2, n_rx=3001, modes=1, rx_dtype="complex128", tx_dtype="float64"))
    for i, (a, b) in enumerate((a, b) for a in ("float64", "complex128", "complex64") for b in ("float64", "complex128", "complex64")):
        rows.append(dict(name=f"{a}_{b}", nTx=21, SpS=2, n_rx=100 + i, modes=1 + i % 3, rx_dtype=a, tx_dtype=b))
    return rows


TILE_ROWS = _tiling()


def tile_input(row):
    rng = np.random.default_rng(1000 + len(row["name"]) + row["n_rx"])

    def draw(n, dtype):
        v = rng.normal(size=(n, row["modes"]))
        if np.dtype(dtype).kind == "c":
            v = v + 1j * rng.normal(size=v.shape)
        return v.astype(dtype)
    return draw(row["n_rx"], row["rx_dtype"]), draw(row["nTx"], row["tx_dtype"])


# ---- the whole call: a delayed, repeated, noisy copy; perm / turns: what the channel does to the modes
SYNC_ROWS = [
    dict(name="f64_f64_1d", M=4, constType="pam", modes=0, reference="symbols", syncMode="amp", SpS=2, nTx=300, n_rx=1000, delay=77,
         rx_dtype="float64", tx_dtype="float64", seed=21),
    dict(name="f64_f64_real_mode", M=4, constType="pam", modes=1, reference="symbols", syncMode="real", SpS=2, nTx=300, n_rx=1000, delay=77,
         rx_dtype="float64", tx_dtype="float64", seed=22),
    dict(name="c128_f64_amp", M=4, constType="pam", modes=1, reference="symbols", syncMode="amp", SpS=2, nTx=300, n_rx=1000, delay=41,
         rx_dtype="complex128", tx_dtype="float64", seed=23),
    dict(name="f64_c128_amp", M=4, constType="pam", modes=1, reference="symbols", syncMode="amp", SpS=2, nTx=300, n_rx=1000, delay=41,
         rx_dtype="float64", tx_dtype="complex128", seed=24),
    dict(name="c64_c64_2d", M=16, constType="qam", modes=2, reference="symbols", syncMode="amp", SpS=2, nTx=300, n_rx=1000, delay=53,
         rx_dtype="complex64", tx_dtype="complex64", seed=25, perm=[1, 0]),
    dict(name="c64_c128_signal", M=16, constType="qam", modes=2, reference="signal", syncMode="amp", SpS=2, nTx=300, n_rx=1000, delay=53,
         rx_dtype="complex64", tx_dtype="complex128", seed=26),
    dict(name="c128_c64_real", M=16, constType="qam", modes=2, reference="symbols", syncMode="real", SpS=2, nTx=300, n_rx=1000, delay=53,
         rx_dtype="complex128", tx_dtype="complex64", seed=27, turns=[1, 3]),
    dict(name="f64_signal_1d", M=4, constType="pam", modes=0, reference="signal", syncMode="amp", SpS=2, nTx=400, n_rx=1100, delay=67,
         rx_dtype="float64", tx_dtype="float64", seed=28),
    dict(name="eight_modes_permuted", M=16, constType="qam", modes=8, reference="symbols", syncMode="amp", SpS=2, nTx=150, n_rx=500, delay=31,
         rx_dtype="complex128", tx_dtype="complex128", seed=29, perm=[3, 0, 7, 1, 6, 2, 5, 4]),
    dict(name="six_modes_signal", M=16, constType="qam", modes=6, reference="signal", syncMode="amp", SpS=2, nTx=150, n_rx=500, delay=31,
         rx_dtype="complex128", tx_dtype="complex128", seed=33, perm=[3, 0, 5, 1, 4, 2]),        # the most columns decimate takes at once
    dict(name="seven_modes_signal", M=16, constType="qam", modes=7, reference="signal", syncMode="amp", SpS=2, nTx=150, n_rx=500, delay=31,
         rx_dtype="complex128", tx_dtype="complex128", seed=34, perm=[3, 0, 5, 6, 1, 4, 2]),     # groups of 4 and 3 columns
    dict(name="eight_modes_signal", M=16, constType="qam", modes=8, reference="signal", syncMode="real", SpS=2, nTx=150, n_rx=500, delay=31,
         rx_dtype="complex128", tx_dtype="complex128", seed=35, perm=[3, 0, 7, 1, 6, 2, 5, 4], turns=[0, 1, 2, 3, 0, 1, 2, 3]),
    dict(name="kept_beyond_B", M=4, constType="pam", modes=1, reference="symbols", syncMode="amp", SpS=2, nTx=900, n_rx=2 * B + 2 + 1, delay=201,
         rx_dtype="float64", tx_dtype="float64", seed=30),
    dict(name="sps16", M=4, constType="pam", modes=1, reference="symbols", syncMode="amp", SpS=16, nTx=60, n_rx=2100, delay=301,
         rx_dtype="float64", tx_dtype="float64", seed=31),
    dict(name="ook_zeros_dropped", M=2, constType="ook", modes=2, reference="symbols", syncMode="amp", SpS=2, nTx=350, n_rx=1000, delay=83,
         rx_dtype="float64", tx_dtype="float64", seed=32),
]
SIGMA = 0.02


def sync_param(row):
    import types
    return types.SimpleNamespace(SpS=row["SpS"], reference=row["reference"], syncMode=row["syncMode"], pulseType="rrc", rollOff=0.01,
                                 nFilterTaps=256, constType="pam" if row["constType"] == "ook" else row["constType"], M=row["M"])


def sync_input(row):
    """(rx, tx): periodic shaping of the symbols (a circular convolution over one period), rolled, cut and made noisy."""
    import opticommpy_amd as oa
    import types
    rng = np.random.default_rng(row["seed"])
    cols, SpS, nTx = max(row["modes"], 1), row["SpS"], row["nTx"]
    if row["constType"] == "ook":
        table = np.array([0.0, 1.0])
    else:
        table = oa.grayMapping(row["M"], row["constType"]).astype(np.complex128 if row["constType"] != "pam" else np.float64)
        table = table / np.sqrt(np.mean(np.abs(table) ** 2))
    sym = table[rng.integers(0, len(table), size=(nTx, cols))]
    kind = ("rrc", 0.1) if row["reference"] == "symbols" else ("nrz", 0.1)
    pulse = oa.pulseShape(types.SimpleNamespace(pulseType=kind[0], SpS=SpS, nFilterTaps=64, rollOff=kind[1]))
    P = nTx * SpS
    up = np.zeros((P, cols), dtype=sym.dtype)
    up[::SpS] = sym
    h = np.zeros(P)
    for t, v in enumerate(pulse):
        h[(t - (len(pulse) - 1) // 2) % P] += v
    wave = np.fft.ifft(np.fft.fft(up, axis=0) * np.fft.fft(h)[:, None], axis=0)
    wave = wave.real.copy() if sym.dtype.kind != "c" else wave
    tx = sym if row["reference"] == "symbols" else wave
    reps = -(-row["n_rx"] // P) + 1
    rx = np.roll(np.tile(wave, (reps, 1)), row["delay"], axis=0)[:row["n_rx"]]
    rx = rx[:, row.get("perm", list(range(cols)))]
    if "turns" in row:
        rx = rx * (1j ** np.array(row["turns"]))[None, :]
    if np.dtype(row["rx_dtype"]).kind == "c":
        rx = rx + (rng.normal(size=rx.shape) + 1j * rng.normal(size=rx.shape)) * SIGMA
    else:
        rx = rx + rng.normal(size=rx.shape) * SIGMA
    rx, tx = rx.astype(row["rx_dtype"]), tx.astype(row["tx_dtype"])
    if row["modes"] == 0:
        rx, tx = rx[:, 0], tx[:, 0]
    return np.ascontiguousarray(rx), np.ascontiguousarray(tx)


# ---- windowed mean
MA_ROWS = [
    dict(n=T - 1, cols=1, N=2, dtype="float64", seed=41),
    dict(n=T, cols=1, N=3, dtype="float64", seed=42),
    dict(n=T + 1, cols=3, N=T, dtype="float64", seed=43),
    dict(n=2 * T + 1, cols=1, N=T + 1, dtype="complex128", seed=44),
    dict(n=2 * T + 1, cols=3, N=500, dtype="complex128", seed=45),
    dict(n=T + 1, cols=1, N=2048, dtype="float64", seed=46),
    dict(n=T + 1, cols=1, N=2048, dtype="complex128", seed=47),
    dict(n=T - 1, cols=3, N=2047, dtype="complex64", seed=48),
    dict(n=300, cols=1, N=301, dtype="float64", seed=49),                # N > n
    dict(n=2, cols=1, N=2, dtype="float64", seed=50),
    dict(n=2, cols=3, N=5, dtype="complex128", seed=51),
    dict(n=1, cols=1, N=4, dtype="float64", seed=52),
    dict(n=3 * T, cols=1, N=500, dtype="float64", seed=53),
]


def ma_input(row):
    rng = np.random.default_rng(row["seed"])
    x = rng.normal(size=(row["n"], row["cols"])) + 0.5
    if np.dtype(row["dtype"]).kind == "c":
        x = x + 1j * rng.normal(size=x.shape)
    x = x.astype(row["dtype"])
    return x[:, 0].copy() if row["cols"] == 1 else x


# ---- bert: n at the edges of the reduction; `ones`: how many bits are 1 (None: about half)
BERT_ROWS = [
    dict(n=BLOCK - 1, ones=None, bits_dtype="int64", seed=61),
    dict(n=BLOCK, ones=None, bits_dtype="int32", seed=62),
    dict(n=BLOCK + 1, ones=None, bits_dtype="int8", seed=63),
    dict(n=3, ones=1, bits_dtype="uint8", seed=64),
    dict(n=1000, ones=1, bits_dtype="bool", seed=65),                     # one class holds a single sample
    dict(n=1000, ones=999, bits_dtype="uint8", seed=66),
    dict(n=BLOCK * BERT_BLOCKS, ones=None, bits_dtype="uint8", seed=67),
    dict(n=BLOCK * BERT_BLOCKS + 1, ones=None, bits_dtype="int64", seed=68),
]


def bert_input(row):
    rng = np.random.default_rng(row["seed"])
    n = row["n"]
    if row["ones"] is None:
        bits = rng.integers(0, 2, size=n)
        bits[0], bits[-1] = 1, 0
    else:
        bits = np.zeros(n, dtype=np.int64)
        bits[rng.choice(n, size=row["ones"], replace=False)] = 1
    Irx = np.where(bits == 1, 1.0, 0.1) + rng.normal(size=n) * np.where(bits == 1, 0.2, 0.1)
    return Irx, bits.astype(row["bits_dtype"])
