"""Synthetic shape rows of the sampling-clock kernels, judged by tests/clock_restatement.py alone (no reference needed): every size
at which a kernel takes another path.  tests/test_clock_emu.py walks them on the emulator, tests/test_gpu_clock_shapes.py on the GPU.

Clock recovery rows use random complex input and large loop gains, so that ``t_nco`` crosses +-1 often; the seeds were found by a
search on the CPU with the restatement, and ``gardner_expect`` re-asserts the property each row was searched for.  With C the
kernel's chunk length (clock_kernels.h: kChunk = 256, read back from the emulator by the tests) and F its flush length (kFlush = 64):
input lengths 1 .. 5 (the loop runs zero or one time), C - 1, C, C + 1, 2 C + 3; at least three gaps of each sign in one row; a gap
of each sign within two inputs of a chunk boundary and within two outputs of a flush boundary; the negative gap that takes n to Ln
(the dropped write); 1, 2, 3, 4 and 64 columns; columns that end at different n with one column all zeros; both precisions and
both detector forms.
"""
import numpy as np

import clock_restatement as rs

C, F = 256, 64
RATIO_ADC = 0.5 * (1 + 105e-6)


def gardner_input(seed, n, cols, dtype="complex128", zero_col=None, scale=None):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, cols)) + 1j * rng.normal(size=(n, cols))) / np.sqrt(2)
    if scale is not None:
        x = x * np.asarray(scale)[None, :]
    if zero_col is not None:
        x[:, zero_col] = 0
    return x.astype(dtype)


# name: seed, n, cols, dtype, parameters, the property searched for
GARDNER_ROWS = {}
for _n in (1, 2, 3, 4, 5):
    GARDNER_ROWS[f"len{_n}"] = dict(seed=None, n=_n, cols=2, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500),
                                    want="tiny")
for _n in (C - 1, C, C + 1, 2 * C + 3):
    GARDNER_ROWS[f"len{_n}"] = dict(seed=None, n=_n, cols=2, dtype="complex64" if _n % 2 else "complex128",
                                    p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500), want="gaps")
GARDNER_ROWS.update({
    "three_each": dict(seed=None, n=2 * C + 3, cols=1, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500),
                       want="three_each"),
    "three_each_ted_c64": dict(seed=None, n=2 * C + 3, cols=3, dtype="complex64", p=dict(kp=0.3, ki=0.01, isNyquist=False, lpad=7, maxPPM=0),
                               want="three_each"),
    "chunk_border": dict(seed=None, n=2 * C + 3, cols=1, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500),
                         want="chunk_border"),
    "flush_border": dict(seed=None, n=2 * C + 3, cols=1, dtype="complex64", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500),
                         want="flush_border"),
    "dropped_write": dict(seed=None, n=40, cols=1, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500),
                          want="dropped"),
    "cols4": dict(seed=None, n=C + 1, cols=4, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=False, lpad=0, maxPPM=500), want="gaps"),
    "cols64": dict(seed=None, n=C + 70, cols=64, dtype="complex64", p=dict(kp=0.08, ki=0.002, isNyquist=True, lpad=1, maxPPM=500), want="gaps"),
    "uneven_ends": dict(seed=None, n=3 * C, cols=3, dtype="complex128", zero_col=1, p=dict(kp=0.15, ki=0.005, isNyquist=True, lpad=1, maxPPM=500),
                        want="uneven"),
})
# seeds the search found (tools: python tests/clock_shape_cases.py)
SEARCHED = {'len1': 1000, 'len2': 1000, 'len3': 1000, 'len4': 1000, 'len5': 1000, 'len255': 1003, 'len256': 1000, 'len257': 1003, 'len515': 1024,
            'three_each': 1003, 'three_each_ted_c64': 1001, 'chunk_border': 4399, 'flush_border': 1026, 'dropped_write': 1009, 'cols4': 1000,
            'cols64': 1001, 'uneven_ends': 1002}


def _holds(want, info, Ln):
    gaps = info["gaps"]
    pos = [g for col in gaps for g in col if g[0] > 0]
    neg = [g for col in gaps for g in col if g[0] < 0]
    if not info["tmax"] < 3.0:          # the loop stays a loop: no run of more than two steps back, nothing overflows
        return False
    if want == "tiny":
        return True
    if want == "gaps":
        return len(pos) >= 1 and len(neg) >= 1
    if want == "three_each":
        return all(sum(1 for g in col if g[0] > 0) >= 3 and sum(1 for g in col if g[0] < 0) >= 3 for col in gaps[:1])
    if want == "chunk_border":          # the input index m at a gap within two of the first chunk border, m = 2 + C
        return any(abs(g[2] - (2 + C)) <= 2 for g in pos) and any(abs(g[2] - (2 + C)) <= 2 for g in neg)
    if want == "flush_border":          # the output index n at a gap within two of a multiple of F (beyond the first)
        near = lambda g: g[1] >= F - 2 and min(g[1] % F, F - g[1] % F) <= 2      # noqa: E731
        return any(near(g) for g in pos) and any(near(g) for g in neg)
    if want == "dropped":
        return len(info["dropped"]) >= 1
    if want == "uneven":
        return len(set(info["last_n"])) == len(info["last_n"])
    raise KeyError(want)


def gardner_row(name):
    r = dict(GARDNER_ROWS[name])
    r["seed"] = SEARCHED[name]
    r["x"] = gardner_input(r["seed"], r["n"], r["cols"], r["dtype"], r.get("zero_col"))
    return r


_EXPECT = {}


def gardner_expect(name):
    """(row, restated signal, timing values, info), computed once; asserts the property the row stands for."""
    if name not in _EXPECT:
        r = gardner_row(name)
        p = r["p"]
        out, tv, info = rs.gardner(r["x"], p["kp"], p["ki"], p["isNyquist"], p["lpad"], p["maxPPM"])
        assert _holds(r["want"], info, info["Ln"]), (name, r["want"], info["gaps"], info["last_n"], info["dropped"])
        for a in (r["x"], out, tv):
            a.setflags(write=False)
        _EXPECT[name] = (r, out, tv, info)
    return _EXPECT[name]


def search(name, first=1000, tries=4000):
    r = dict(GARDNER_ROWS[name])
    p = r["p"]
    for seed in range(first, first + tries):
        x = gardner_input(seed, r["n"], r["cols"], r["dtype"], r.get("zero_col"))
        _, _, info = rs.gardner(x, p["kp"], p["ki"], p["isNyquist"], p["lpad"], p["maxPPM"])
        if _holds(r["want"], info, info["Ln"]):
            return seed
    return None


# ---- interpolation: N, columns, dtype, outFs / inFs
INTERP_ROWS = [(1, 1, "float64", 2.0), (2, 2, "complex128", RATIO_ADC), (3, 3, "float32", 2.0), (255, 1, "complex64", 1.0), (256, 1, "float64", 1.0),
               (257, 1, "complex128", 1.0), (255, 4, "float32", RATIO_ADC), (256, 5, "complex64", 1 / 3), (257, 2, "float64", 2.0),
               (128, 2, "complex128", 1.0), (1 << 19, 1, "float32", 2.0 * (1 + 1e-6))]      # the last: more elements than one pass of the grid


def interp_input(i):
    N, cols, dtype, ratio = INTERP_ROWS[i]
    rng = np.random.default_rng(300 + i)
    x = rng.normal(size=(N, cols))
    if dtype.startswith("complex"):
        x = x + 1j * rng.normal(size=(N, cols))
    return x.astype(dtype), 64e9, 64e9 * ratio


# ---- quantizer: a (maxV, minV) pair whose np.arange table holds 2 ** nBits + 1 levels
LONG_TABLE = dict(nBits=3, maxV=1.4994487522902058, minV=-0.8960718336144597)       # found by long_table(): 9 levels


def long_table(nBits=3, tries=20000):
    rng = np.random.default_rng(500)
    for _ in range(tries):
        minV, maxV = sorted(rng.uniform(-2, 2, size=2))
        if len(rs.quant_levels(nBits, maxV, minV)) == 2 ** nBits + 1:
            return float(maxV), float(minV)
    return None


# ---- min / max: sizes around the block length and beyond one pass of the grid, the extremes in imaginary parts only
MINMAX_ROWS = [(1, "complex128"), (127, "complex128"), (128, "complex128"), (129, "complex64"), (255, "float64"), (256, "float64"), (257, "float32"),
               (256 * 4096 // 2 + 3, "complex128")]


def minmax_input(i):
    n, dtype = MINMAX_ROWS[i]
    rng = np.random.default_rng(400 + i)
    x = rng.uniform(-1, 1, size=(n, 1))
    if dtype.startswith("complex"):
        x = x + 1j * rng.uniform(-1, 1, size=(n, 1))
        x[rng.integers(0, n), 0] = 0.25 + 3.5j          # the maximum, in an imaginary part only
        if n > 1:
            x[(rng.integers(0, n - 1) + 1 + int(np.argmax(x.imag))) % n, 0] = -0.5 - 2.5j
    return x.astype(dtype)


if __name__ == "__main__":
    import sys
    print({name: search(name) for name in (sys.argv[1:] or GARDNER_ROWS)})
    print("long table", long_table())
