"""Synthetic shape rows of the sampling-clock kernels, judged by tests/clock_restatement.py alone (no reference needed): every size
at which a kernel takes another path.  tests/test_clock_emu.py walks them on the emulator, tests/test_gpu_clock_shapes.py on the GPU.

Clock recovery rows use random complex input and large loop gains, so that ``t_nco`` crosses +-1 often; the seeds were found by a
search on the CPU with the restatement, and ``gardner_expect`` re-asserts the property each row was searched for.  With C the
kernel's chunk length (clock_kernels.h: kChunk = 256, read back from the emulator by the tests) and F its flush length (kFlush = 64):
input lengths 1 .. 5 (the loop runs zero or one time), C - 1, C, C + 1, 2 C + 3; at least three gaps of each sign in one row; a gap
of each sign within two inputs of a chunk boundary and within two outputs of a flush boundary; the negative gap that takes n to Ln
(the dropped write); 1, 2, 3, 4 and 64 columns; columns that end at different n with one column all zeros; both precisions and
both detector forms.

The second set holds the kernel's own chunk, ring and flush code to the restatement:

* fall rows (constructed, not searched): the input is zero but for two equal samples, so the detector fires once, ``t_nco`` jumps to
  a chosen positive value and the loop steps back ``ceil(t_nco) - 1`` outputs in a row.  ``flush_base`` states the flush base f the
  kernel has at a peak, ``kernel_status`` whether it must accept a column's falls (the lowest n of every fall is at least f + 2, or
  f is still 0) or refuse it; two more constructed rows put ``t_nco`` exactly on +1 and on -1, where no gap is taken;
* border rows (searched): a gap of each sign with the input index m exactly 1 before, on and 1 after the first chunk border 2 + C,
  and with the output index n exactly 1 before, on and 1 after a flush border (LAG = 2 F, 3 F) and the ring's wrap (256, 512);
* padding rows (searched): zero padding that straddles a chunk border and the four-sample overlap, that fills a whole chunk, that
  is all but five samples; the loop ended by Ln and ended by the input; 5 and 7 columns.

Interpolation rows with explicit output times (``interp_times_row``), and the clock-drift table (``DRIFT_ROWS``) follow below.
"""
import numpy as np

import clock_restatement as rs

C, F, LAG = 256, 64, 128
RATIO_ADC = 0.5 * (1 + 105e-6)


def gardner_input(seed, n, cols, dtype="complex128", zero_col=None, scale=None):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, cols)) + 1j * rng.normal(size=(n, cols))) / np.sqrt(2)
    if scale is not None:
        x = x * np.asarray(scale)[None, :]
    if zero_col is not None:
        x[:, zero_col] = 0
    return x.astype(dtype)


# ---- what k_gardner keeps of its outputs.  After every step it runs ``while (n >= f + LAG) flush(f), f += F``: f is 0 until n first
# reaches LAG and then the multiple of F with f + LAG - F <= hi < f + LAG, hi the furthest n so far.  A step back that leaves
# n < f + 2 with f > 0 ends the column with kGardnerBackrun (out[n - 2] has left LDS).
def flush_base(hi):
    return 0 if hi < LAG else F * ((hi - LAG) // F + 1)


def kernel_status(falls):
    """0 (kGardnerOk) or 1 (kGardnerBackrun) for a column with these falls (n_peak, depth).  The furthest n so far is the highest
    peak so far: n rises between two falls and a fall begins where it stops rising."""
    hi = 0
    for n_peak, depth in falls:
        hi = max(hi, n_peak)
        f = flush_base(hi)
        if f > 0 and n_peak - depth < f + 2:
            return 1
    return 0


def final_m(info, k):
    """The input index a column ended at: m moves on with every step but a step back."""
    g = info["gaps"][k]
    return info["last_n"][k] - sum(1 for q in g if q[0] < 0) + sum(1 for q in g if q[0] > 0)


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
FIRST_ROWS = tuple(GARDNER_ROWS)

# ---- border rows: (index, border, offset, sign) -- a gap of that sign taken with m (index 2 of a gap) or n (index 1) at border + offset
BORDER_CELLS = {}
for _label, _index, _border in (("chunk", 2, 2 + C), ("flush128", 1, LAG), ("flush192", 1, LAG + F), ("wrap256", 1, 256), ("wrap512", 1, 512)):
    for _off in (-1, 0, 1):
        for _sign in (1, -1):
            BORDER_CELLS[f"{_label}_{'m1' if _off < 0 else 'p' + str(_off)}_{'pos' if _sign > 0 else 'neg'}"] = (_index, _border, _off, _sign)
# The detector updates t_nco at even n only and a negative gap keeps n's parity, so a negative gap is taken at even n alone (an odd n
# is reached by a step of one, which leaves t_nco within [-1, 1], or by a step back, which leaves it positive): the cells with a
# negative gap at an odd n do not exist, and a search of 20000 seeds each found none.  They have no row.
UNREACHABLE = tuple(name for name, (_index, _border, _off, _sign) in BORDER_CELLS.items() if _index == 1 and _sign < 0 and (_border + _off) % 2)
for _i, (_name, _cell) in enumerate(BORDER_CELLS.items()):
    if _name in UNREACHABLE:
        continue
    GARDNER_ROWS[_name] = dict(seed=None, n=2 * C + 60 if _cell[1] == 512 else 2 * C + 3, cols=1, dtype="complex64" if _i % 2 else "complex128",
                               p=dict(kp=0.3, ki=0.01, isNyquist=_i % 4 < 2, lpad=1, maxPPM=500), want="cell", cell=_cell)

# ---- padding rows: the zeros behind the data against the chunk border (m = 2 + C reads x[C .. C + 3]; chunk 1 is x[C .. 2 C + 3])
for _n in (2 * C, 2 * C + 1):
    for _lpad in (0, 3, 4, 5):
        _ends = "Ln" if (_lpad + _n) % 2 else "input"
        GARDNER_ROWS[f"pad{_lpad}_len{_n}"] = dict(seed=None, n=_n, cols=2, dtype="complex64" if _lpad % 2 else "complex128",
                                                   p=dict(kp=0.3, ki=0.01, isNyquist=_lpad < 4, lpad=_lpad, maxPPM=20000 if _ends == "Ln" else 0),
                                                   want="gaps", ends=_ends)
GARDNER_ROWS.update({
    # chunk 1 and chunk 2 lie wholly behind the data: the fetch reads nothing
    f"pad{C + 8}_len{C - 3}": dict(seed=None, n=C - 3, cols=2, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=C + 8, maxPPM=0),
                                   want="gaps", ends="input"),
    f"pad{2 * C}_len5": dict(seed=None, n=5, cols=1, dtype="complex64", p=dict(kp=0.3, ki=0.01, isNyquist=False, lpad=2 * C, maxPPM=0),
                             want="long", ends="input"),
    "cols5": dict(seed=None, n=C + 1, cols=5, dtype="complex64", p=dict(kp=0.3, ki=0.01, isNyquist=True, lpad=1, maxPPM=500), want="gaps"),
    "cols7": dict(seed=None, n=C + 1, cols=7, dtype="complex128", p=dict(kp=0.3, ki=0.01, isNyquist=False, lpad=1, maxPPM=500), want="gaps"),
})
PADDING_ROWS = tuple(name for name in GARDNER_ROWS if name.startswith("pad"))

# seeds the search found (tools: python tests/clock_shape_cases.py)
SEARCHED = {'len1': 1000, 'len2': 1000, 'len3': 1000, 'len4': 1000, 'len5': 1000, 'len255': 1003, 'len256': 1000, 'len257': 1003, 'len515': 1024,
            'three_each': 1003, 'three_each_ted_c64': 1001, 'chunk_border': 4399, 'flush_border': 1026, 'dropped_write': 1009, 'cols4': 1000,
            'cols64': 1001, 'uneven_ends': 1002}
SEARCHED.update({'chunk_m1_pos': 1512, 'chunk_m1_neg': 1036, 'chunk_p0_pos': 1009, 'chunk_p0_neg': 1067, 'chunk_p1_pos': 1064, 'chunk_p1_neg': 1070,
                 'flush128_m1_pos': 4020, 'flush128_p0_pos': 1036, 'flush128_p0_neg': 1115, 'flush128_p1_pos': 1605, 'flush192_m1_pos': 1076,
                 'flush192_p0_pos': 1001, 'flush192_p0_neg': 1095, 'flush192_p1_pos': 4469, 'wrap256_m1_pos': 2886, 'wrap256_p0_pos': 1478,
                 'wrap256_p0_neg': 1026, 'wrap256_p1_pos': 2195, 'wrap512_m1_pos': 1654, 'wrap512_p0_pos': 1007, 'wrap512_p0_neg': 1151,
                 'wrap512_p1_pos': 1737, 'pad0_len512': 1202, 'pad3_len512': 1038, 'pad4_len512': 1000, 'pad5_len512': 1002, 'pad0_len513': 1014,
                 'pad3_len513': 1152, 'pad4_len513': 1001, 'pad5_len513': 1000, 'pad264_len253': 1024, 'pad512_len5': 1000, 'cols5': 1077,
                 'cols7': 1000})

# ---- fall rows.  The burst: two samples amp (1 + 0.5j) at pos, pos + 1 (Gardner's detector) or pos + 1, pos + 2 (the Nyquist form),
# pos even: the detector fires at n = pos + 2 alone and the loop falls by AMP's depth.  The amplitudes are the middle of the
# interval a scan with the restatement found for each depth (t_nco lands near depth + 0.5); kp = 0.3, ki = 0.
FALL_P = dict(kp=0.3, ki=0.0, lpad=1, maxPPM=0)
AMP = {False: {3: 3.0403, 4: 3.4573, 61: 12.8177, 62: 12.92, 63: 13.0231, 100: 16.3709, 120: 17.9219},
       True: {3: 1.6485, 4: 1.7591, 61: 3.3848, 62: 3.3983, 63: 3.4118, 100: 3.8267, 120: 4.005}}


def _fall(n, bursts, nyquist, dtype, want="fall", **more):
    """bursts: per column (n_peak, depth) or None (a column of zeros)."""
    return dict(seed=None, n=n, cols=len(bursts), dtype=dtype, p=dict(FALL_P, isNyquist=nyquist), want=want, bursts=bursts, **more)


for _nyq, _d in ((False, "ted"), (True, "nyq")):
    for _t in ("complex128", "complex64"):
        _s = f"{_d}_{'c128' if _t == 'complex128' else 'c64'}"
        for _depth in (3, 4, 61, 62):                   # the worst phase: n_peak = f + F, right after a flush
            GARDNER_ROWS[f"fall{_depth}_at192_{_s}"] = _fall(400, [(192, _depth)], _nyq, _t)
        # one more and the kernel refuses: column 1 alone
        GARDNER_ROWS[f"refuse63_at192_{_s}"] = _fall(400, [(192, 3), (192, 63), (192, 62)], _nyq, _t, want="refuse", status=[0, 1, 0])
    _t, _u = ("complex128", "complex64") if _nyq else ("complex64", "complex128")
    GARDNER_ROWS.update({
        f"fall62_at448_{_d}": _fall(700, [(448, 62)], _nyq, _t),                    # the ring's second lap
        f"fall120_at318_{_d}": _fall(600, [(318, 120)], _nyq, _u),                  # a favourable phase: f = 192, the fall ends at 198
        f"fall3_at4_{_d}": _fall(60, [(4, 3)], _nyq, _t, low=1),                    # n reaches 1 (the detector's out[n - 2] is place 255) and recovers
        f"fall4_at4_{_d}": _fall(60, [(4, 4)], _nyq, _u, low=0, last_n=[0]),        # n reaches 0: the column ends, the result has no rows
        f"fall4_at4_beside_{_d}": _fall(60, [(4, 4), (4, 3)], _nyq, _t, low=0),     # ... beside a column that runs to its end
        f"fall100_at120_{_d}": _fall(500, [(120, 100)], _nyq, _u),                  # inside the first flush period: f = 0, any depth
        # a searched random tail behind the burst: the ring places rewritten on the way down are read again on the way up
        f"fall62_tail_{_d}": _fall(700, [(192, 62)], _nyq, _t, tail=260),
    })
FALL_ROWS = tuple(name for name in GARDNER_ROWS if "bursts" in GARDNER_ROWS[name])
# t_nco exactly on a threshold: with t_nco = 0 an output is its input sample, so two samples of 2 give Gardner's detector -4 at the even
# n = 12 (a = b = 2, c = 0) and +4 at n = 12 (a = 0, b = c = 2); kp = 0.25 makes t_nco exactly 1 and -1, which is no gap
GARDNER_ROWS.update({
    "exactly_plus_one": dict(seed=None, n=40, cols=1, dtype="complex128", p=dict(kp=0.25, ki=0.0, isNyquist=False, lpad=1, maxPPM=0),
                             want="threshold", samples={10: 2.0, 11: 2.0}, tv_at=(13, 1.0)),
    "exactly_minus_one": dict(seed=None, n=40, cols=1, dtype="complex64", p=dict(kp=0.25, ki=0.0, isNyquist=False, lpad=1, maxPPM=0),
                              want="threshold", samples={11: 2.0, 12: 2.0}, tv_at=(13, -1.0)),
})
SEARCHED.update({"exactly_plus_one": None, "exactly_minus_one": None})
SEARCHED.update({name: None for name in FALL_ROWS})
SEARCHED.update({"fall62_tail_ted": 1000, "fall62_tail_nyq": 1001})


def burst_input(r, seed):
    nyquist = r["p"]["isNyquist"]
    x = np.zeros((r["n"], r["cols"]), dtype=np.complex128)
    for k, b in enumerate(r["bursts"]):
        if b is not None:
            first = b[0] - 2 + (1 if nyquist else 0)
            x[first:first + 2, k] = AMP[nyquist][b[1]] * (1 + 0.5j)
    if r.get("tail"):
        rng = np.random.default_rng(seed)
        m = r["n"] - r["tail"]
        x[r["tail"]:, 0] = (rng.normal(size=m) + 1j * rng.normal(size=m)) / np.sqrt(2)
    return x.astype(r["dtype"])


def _holds(r, info):
    want, gaps = r["want"], info["gaps"]
    pos = [g for col in gaps for g in col if g[0] > 0]
    neg = [g for col in gaps for g in col if g[0] < 0]
    nSamples = r["n"] + r["p"]["lpad"]
    if "ends" in r:                     # what ended the loop of column 0: the output length or the input
        n, m = info["last_n"][0], final_m(info, 0)
        if r["ends"] == "Ln" and not (n >= info["Ln"] - 1 and m < nSamples - 2):
            return False
        if r["ends"] == "input" and not (m >= nSamples - 2 and n < info["Ln"] - 1):
            return False
    if want in ("fall", "refuse"):      # rows with conditions of their own
        if not info["tmax"] < np.inf:
            return False
        for k, b in enumerate(r["bursts"]):
            if (info["falls"][k][:1] != [b]) if b is not None else info["falls"][k]:
                return False
        status = [kernel_status(col) for col in info["falls"]]
        if status != r.get("status", [0] * r["cols"]):
            return False
        if "low" in r and min(n_peak - depth for n_peak, depth in info["falls"][0]) != r["low"]:
            return False
        if "last_n" in r and info["last_n"] != r["last_n"]:
            return False
        if r.get("tail"):               # gaps of each sign beyond the peak, and no second deep fall
            later = [g for g in gaps[0] if g[1] > r["bursts"][0][0]]
            return sum(g[0] > 0 for g in later) >= 2 and sum(g[0] < 0 for g in later) >= 2 and max(d for _, d in info["falls"][0][1:]) < 3
        return True
    if want == "threshold":             # |t_nco| was exactly 1 once, and the output n = 12 that met it took no gap
        return info["margin"] == 0.0 and info["tmax"] < 3.0 and not any(g[1] == 12 for g in pos + neg)
    if not info["tmax"] < 3.0:          # the loop stays a loop: no run of more than two steps back, nothing overflows
        return False
    if want == "tiny":
        return True
    if want == "gaps":
        return len(pos) >= 1 and len(neg) >= 1
    if want == "long":                  # the loop ran on through the padding, into the second chunk
        return min(info["last_n"]) > C + 2
    if want == "cell":
        index, border, off, sign = r["cell"]
        return any(g[0] == sign and g[index] == border + off for g in pos + neg)
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


def _input(r, seed):
    if "bursts" in r:
        return burst_input(r, seed)
    if "samples" in r:
        x = np.zeros((r["n"], r["cols"]), dtype=r["dtype"])
        for i, v in r["samples"].items():
            x[i, :] = v
        return x
    return gardner_input(seed, r["n"], r["cols"], r["dtype"], r.get("zero_col"))


def gardner_row(name):
    r = dict(GARDNER_ROWS[name], name=name)
    r["seed"] = SEARCHED[name]
    r["x"] = _input(r, r["seed"])
    return r


_EXPECT = {}


def gardner_expect(name):
    """(row, restated signal, timing values, info), computed once; asserts the property the row stands for."""
    if name not in _EXPECT:
        r = gardner_row(name)
        p = r["p"]
        out, tv, info = rs.gardner(r["x"], p["kp"], p["ki"], p["isNyquist"], p["lpad"], p["maxPPM"])
        assert _holds(r, info), (name, r["want"], info["gaps"], info["falls"], info["last_n"], info["dropped"])
        assert "tv_at" not in r or tv[r["tv_at"][0], 0] == r["tv_at"][1], (name, tv[:20, 0])
        for a in (r["x"], out, tv):
            a.setflags(write=False)
        _EXPECT[name] = (r, out, tv, info)
    return _EXPECT[name]


def reach(r, info):
    """Rows of the full output that may hold something: to the furthest n a column ended at, and to the highest peak a column fell
    from (the first rows, as before, end at or beyond every peak)."""
    rows = max(0, max(info["last_n"]))
    if r["name"] not in FIRST_ROWS:
        rows = max([rows] + [n_peak + 1 for col in info["falls"] for n_peak, _ in col])
    return min(rows, info["Ln"])


def search(name, first=1000, tries=4000):
    r = dict(GARDNER_ROWS[name])
    p = r["p"]
    for seed in range(first, first + tries):
        _, _, info = rs.gardner(_input(r, seed), p["kp"], p["ki"], p["isNyquist"], p["lpad"], p["maxPPM"])
        if _holds(r, info):
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


# ---- interpolation at explicit output times (clock._interp with t_re / t_im, as the jitter of adc and dac reaches it)
# rates at which the index guess errs both ways, upwards only and downwards only.  The kernel's factor is 1 / inTs with inTs = 1 / inFs,
# which at 64e9 is the double below inFs: there floor(t inFs) is too high 123 times on a row's times and never too low, the kernel's
# own guess too low 126 times and never too high.  guess_errors counts with the kernel's factor.
RATE_BOTH, RATE_HIGH, RATE_LOW = 10e9 * (1 + 1e-6), 10e9, 64e9


def guess_errors(t, inFs, N):
    """(too low, too high): how often interp_index's guess floor(t (1 / inTs)), clamped to [0, N - 1], misses the index a binary
    search over tin = arange(N) inTs finds, over the times inside [tin[0], tin[N - 1]] (the others never reach interp_index).
    Too low runs the first correction loop, too high the second."""
    inTs = 1 / inFs
    tin = np.arange(0, N) * inTs
    t = np.asarray(t, dtype=np.float64)
    t = t[(t >= 0) & (t <= tin[N - 1])]
    j = np.clip(np.searchsorted(tin, t, side="right") - 1, 0, N - 1)
    g = np.clip(np.floor(t * (1.0 / inTs)), 0, N - 1)
    return int(np.sum(g < j)), int(np.sum(g > j))


def _times(kind, tin, inTs, rng):
    N, end = len(tin), tin[-1]
    if kind == "neighbours":            # every input time and its two neighbouring doubles, shuffled
        t = np.concatenate([tin, np.nextafter(tin, -np.inf), np.nextafter(tin, np.inf)])
        return rng.permutation(t)
    if kind == "chosen":                # before the start, -0.0, the ends, beyond the end, NaN; not sorted
        return np.array([end, -1e-12, -0.0, 0.0, 2 * end + inTs, np.nan, np.nextafter(end, np.inf), -inTs, 0.5 * end, np.nextafter(0.0, 1.0),
                         np.nextafter(end, 0.0), np.inf, -np.inf, 0.25 * inTs, end], dtype=np.float64)
    if kind == "exact":                 # every input time, shuffled: each output is an input sample as it is
        return rng.permutation(tin)
    raise KeyError(kind)


# name: N, columns, dtype, inFs, kind of times, form ("real", "complex", "components"), what the row asserts of the index guess
TIMES_ROWS = {}
for _t in ("float32", "float64", "complex64", "complex128"):
    _form = "complex" if _t.startswith("complex") else "real"
    TIMES_ROWS[f"both_ways_{_t}"] = dict(N=300, cols=2, dtype=_t, inFs=RATE_BOTH, kind="neighbours", form=_form, guess="both")
    TIMES_ROWS[f"high_only_{_t}"] = dict(N=300, cols=1, dtype=_t, inFs=RATE_HIGH, kind="neighbours", form=_form, guess="high")
    TIMES_ROWS[f"low_only_{_t}"] = dict(N=300, cols=1, dtype=_t, inFs=RATE_LOW, kind="neighbours", form=_form, guess="low")
for _N in (1, 2, 300):
    TIMES_ROWS[f"chosen_N{_N}_real"] = dict(N=_N, cols=2, dtype="float64" if _N != 2 else "float32", inFs=RATE_BOTH, kind="chosen", form="real")
    TIMES_ROWS[f"chosen_N{_N}_complex"] = dict(N=_N, cols=1, dtype="complex128" if _N != 2 else "complex64", inFs=RATE_BOTH, kind="chosen",
                                               form="complex")
    TIMES_ROWS[f"chosen_N{_N}_components"] = dict(N=_N, cols=3, dtype="complex128", inFs=RATE_LOW, kind="chosen", form="components")
TIMES_ROWS.update({
    # the imaginary parts at times of their own: of every pair one is an input time exactly and the other its neighbouring double
    "components_exact_and_not_c128": dict(N=300, cols=2, dtype="complex128", inFs=RATE_BOTH, kind="neighbours", form="components", split=True),
    "components_exact_and_not_c64": dict(N=300, cols=1, dtype="complex64", inFs=RATE_LOW, kind="neighbours", form="components", split=True),
    # an infinite sample: at an input time numpy hands x[j] on (the rule's slope times zero would be NaN beside it)
    "exact_beside_inf_real": dict(N=9, cols=2, dtype="float32", inFs=RATE_BOTH, kind="exact", form="real", inf_at=4),
    "exact_beside_inf_complex": dict(N=9, cols=1, dtype="complex128", inFs=RATE_LOW, kind="exact", form="complex", inf_at=4),
    # the three forms on one input at one set of times (the library takes the real form for real data alone: the input's real parts)
    "forms_real": dict(N=257, cols=2, dtype="complex128", inFs=RATE_BOTH, kind="neighbours", form="real", same_input=True, real_parts=True),
    "forms_complex": dict(N=257, cols=2, dtype="complex128", inFs=RATE_BOTH, kind="neighbours", form="complex", same_input=True),
    "forms_components": dict(N=257, cols=2, dtype="complex128", inFs=RATE_BOTH, kind="neighbours", form="components", same_input=True),
})
_TIMES = {}


def interp_times_row(name):
    """(row, x, inFs, outFs, t_re, t_im or None, expected output), computed once.  outFs is chosen so that the output holds the
    row's times and at least one more, drawn around the input's span; the expected output is np.interp's: of complex data under
    the complex form numpy's complex rule, else numpy's real rule on the parts (rs.clock_interp, as rs.adc_core takes them)."""
    if name in _TIMES:
        return _TIMES[name]
    r = TIMES_ROWS[name]
    N, inFs = r["N"], r["inFs"]
    inTs = 1 / inFs
    rng = np.random.default_rng(700 if r.get("same_input") else 600 + sorted(TIMES_ROWS).index(name))
    x = rng.normal(size=(N, r["cols"]))
    if r["dtype"].startswith("complex"):
        x = x + 1j * rng.normal(size=(N, r["cols"]))
    x = x.astype(r["dtype"])
    tin = np.arange(0, N) * inTs
    t = _times(r["kind"], tin, inTs, rng)
    outFs = inFs * (len(t) + 1.5) / N
    n_out = len(rs.out_times(N, inFs, outFs)[1])
    assert n_out > len(t)
    t_re = np.concatenate([t, rng.uniform(-2 * inTs, tin[-1] + 2 * inTs, size=n_out - len(t))])
    if "inf_at" in r:                   # the times beyond the row's own lie outside the input's span: no segment's rule runs
        x[r["inf_at"], :] = np.inf
        t_re[len(t):] = np.where(t_re[len(t):] < 0.5 * tin[-1], -inTs, tin[-1] + inTs)
    t_im = None
    if r["form"] == "components":
        t_im = rng.permutation(t_re)
        if r.get("split"):              # exact | below | above  ->  below | above | exact (the same shuffle for both)
            order = rng.permutation(3 * N)
            base = np.concatenate([tin, np.nextafter(tin, -np.inf), np.nextafter(tin, np.inf)])
            other = np.concatenate([np.nextafter(tin, -np.inf), np.nextafter(tin, np.inf), tin])
            t_re, t_im = np.concatenate([base[order], t_re[3 * N:]]), np.concatenate([other[order], t_re[3 * N:][::-1]])
            exact_re, exact_im = np.isin(t_re[:3 * N], tin), np.isin(t_im[:3 * N], tin)
            assert np.all(t_re[:3 * N] != t_im[:3 * N]) and np.sum(exact_re & ~exact_im) >= N - 1 and np.sum(~exact_re & exact_im) >= N - 1
    low, high = guess_errors(t, inFs, N)
    if r.get("guess") == "both":
        assert low >= 1 and high >= 1, (name, low, high)
    if r.get("guess") == "high":
        assert low == 0 and high >= 1, (name, low, high)
    if r.get("guess") == "low":
        assert low >= 1 and high == 0, (name, low, high)
    if r.get("real_parts"):
        x = np.ascontiguousarray(np.real(x))
    if r["form"] == "complex":
        want = rs.clock_interp(x, inFs, outFs, t_re)
    elif x.dtype.kind == "c":
        want = (rs.clock_interp(np.real(x), inFs, outFs, t_re) + 1j * rs.clock_interp(np.imag(x), inFs, outFs, t_re if t_im is None else t_im))
        want = want.astype(x.dtype)
    else:
        want = rs.clock_interp(x, inFs, outFs, t_re)
    for a in (x, t_re, want) + (() if t_im is None else (t_im,)):
        a.setflags(write=False)
    _TIMES[name] = (r, x, inFs, outFs, t_re, t_im, want)
    return _TIMES[name]


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


# ---- clock drift.  k_drift_peaks gives difference index i to lane (i - 1) % 256 of its one workgroup (wave (i - 1) % 256 // 64),
# folds a wave by shuffles and the four waves through LDS.  A column is a list of (difference index, height): |t[i+1] - t[i]| is the
# height there and 0 elsewhere, the steps alternating in sign so that t stays small.  Every value is a multiple of 2 ** -4: sums
# and means are exact in any order and the result equals rs.clock_drift bit for bit.
def drift_column(n, jumps, offset=0.0):
    d = np.zeros(max(n - 1, 0))
    for k, (i, h) in enumerate(sorted(jumps)):
        assert 0 <= i < n - 1 and h * 16 == int(h * 16)
        d[i] = h if k % 2 == 0 else -h
    return np.concatenate([[0.0], np.cumsum(d)]) + offset


def _edge_peaks(n):
    """Peaks around the lane, wave and trip borders that fit a column of n values: two columns, no two peaks adjacent."""
    nd = n - 1
    a = {i for i in (1, 63, 65, 255, 257, nd - 2) if 1 <= i <= nd - 2}
    a = [(i, 1.0) for i in sorted(a) if i - 1 not in a]
    b = [(i, 0.75) for i in (64, 256) if 1 <= i <= nd - 2]
    return a, b


# name: n, columns as (jumps, offset), the peaks every column must have by scipy's rule (asserted by drift_expect)
DRIFT_ROWS = {}
for _n, _cols in ((2, 1), (3, 3), (4, 5), (257, 1), (258, 3), (259, 5), (513, 3), (1025, 5)):
    _a, _b = _edge_peaks(_n)
    _spec = [(_a, 1.0), (_b, -3.0), ([(1, 0.5)] if _n > 3 else [], 0.0), (_b, 0.0), (_a, -0.5)][:_cols]
    DRIFT_ROWS[f"n{_n}"] = dict(n=_n, cols=_spec, peaks=[[i for i, _ in j] for j, _ in _spec])
DRIFT_ROWS.update({
    "two_waves": dict(n=300, cols=[([(10, 1.0), (100, 1.0)], 1.0)], peaks=[[10, 100]]),                 # lanes 9 (wave 0) and 99 (wave 1)
    "one_lane": dict(n=600, cols=[([(20, 1.0), (276, 1.0)], 1.0)], peaks=[[20, 276]]),                  # lane 19, its first and second trip
    "wave3_only": dict(n=300, cols=[([(200, 1.0), (250, 1.0)], 1.0), ([(5, 1.0)], 0.0)], peaks=[[200, 250], [5]]),      # lanes 199 and 249
    "plateau_255_257": dict(n=400, cols=[([(50, 1.0), (255, 0.75), (256, 0.75), (257, 0.75)], 1.0)], peaks=[[50, 256]]),
    "plateau_to_the_end": dict(n=300, cols=[([(30, 1.0), (60, 1.0), (296, 1.0), (297, 1.0), (298, 1.0)], 1.0)], peaks=[[30, 60]]),
    "height_half": dict(n=300, cols=[([(40, 0.5), (90, 0.5), (170, 0.4375)], 1.0)], peaks=[[40, 90]]),
    "mean_zero": dict(n=259, cols=[([(1, 1.0), (256, 1.0)], 2.0), ([(1, 1.0), (256, 1.0)], 2.0)], negate=1, peaks=[[1, 256], [1, 256]]),
    "mean_negative": dict(n=513, cols=[([(64, 1.0), (256, 1.0), (510, 1.0)], -5.0), ([(3, 1.0)], 1.0), ([(100, 2.0), (101, 1.0), (300, 1.0)], 0.0)],
                          peaks=[[64, 256, 510], [3], [100, 300]]),
})


def _mixed600():
    """Peaks at the array's ends, a plateau, fewer than two peaks, a negative mean, a mean per column (values not multiples of
    2 ** -4: the peaks are the same whatever the last bit of the mean)."""
    t = np.zeros((600, 4))
    t[100:, 0] += 1.0
    t[350:, 0] -= 1.0
    t[500:, 0] += 1.0                                            # three gaps: periods 250 and 150
    t[2:, 1] -= 1.0
    t[598:, 1] += 1.0                                            # gaps at the first and the last difference a peak can sit on
    t[:, 1] -= 5.0
    t[300:, 2] += 1.0                                            # one gap: nan
    t[10:, 3] += 0.7
    t[12:, 3] += 0.7                                             # a plateau of two equal differences apart... and a second peak
    t[200:, 3] += 0.9
    return t


DRIFT_ROWS["mixed600"] = dict(n=600, cols=None, peaks=[[99, 349, 499], [1, 597], [299], [9, 11, 199]])
_DRIFT = {}


def drift_expect(name):
    """(row, t, expected ppm with the mean over all columns, expected ppm with a mean per column), computed once; asserts the peaks."""
    if name not in _DRIFT:
        r = DRIFT_ROWS[name]
        t = _mixed600() if r["cols"] is None else np.stack([drift_column(r["n"], j, o) for j, o in r["cols"]], axis=1)
        if "negate" in r:
            t[:, r["negate"]] = -t[:, r["negate"]]
            assert np.sum(t) == 0.0
        assert t.shape == (r["n"], len(r["peaks"]))
        for k, peaks in enumerate(r["peaks"]):
            if r["n"] >= 3:
                assert rs.local_maxima(np.abs(np.diff(t[:, k] - np.mean(t))), 0.5).tolist() == peaks, (name, k)
            else:
                assert not peaks
        want = rs.clock_drift(t)
        per_column = np.array([rs.clock_drift(t[:, k])[0] for k in range(t.shape[1])])
        t.setflags(write=False)
        _DRIFT[name] = (r, t, want, per_column)
    return _DRIFT[name]


def same_bits(a, b):
    """Equal as numpy's results are: NaN in the same places (a complex NaN is numpy's NaN + 0j), everything else bit for bit."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    part = {"complex64": np.float32, "complex128": np.float64}.get(a.dtype.name, a.dtype)
    a, b = np.ascontiguousarray(a).view(part), np.ascontiguousarray(b).view(part)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].tobytes(), b[~np.isnan(b)].tobytes()))


def check_coverage():
    """Every cell, depth, phase, padding case, guess direction and drift geometry the tables claim has a row of its name that is
    built for it; gardner_expect, interp_times_row and drift_expect assert that a row has the property."""
    rows = GARDNER_ROWS
    assert all(SEARCHED[name] is not None for name in rows if "samples" not in rows[name] and (name not in FALL_ROWS or rows[name].get("tail")))
    assert rows["exactly_plus_one"]["tv_at"][1] == 1.0 and rows["exactly_minus_one"]["tv_at"][1] == -1.0
    for label, index, border in (("chunk", 2, 2 + C), ("flush128", 1, LAG), ("flush192", 1, LAG + F), ("wrap256", 1, 256), ("wrap512", 1, 512)):
        assert border == 2 + C or (border % F == 0 and border >= LAG)
        for off, o in ((-1, "m1"), (0, "p0"), (1, "p1")):
            for sign, s in ((1, "pos"), (-1, "neg")):
                if index == 1 and sign < 0 and off:         # a negative gap at an odd n: no such cell (UNREACHABLE)
                    assert f"{label}_{o}_{s}" in UNREACHABLE and f"{label}_{o}_{s}" not in rows and border % 2 == 0
                    continue
                assert rows[f"{label}_{o}_{s}"]["want"] == "cell" and rows[f"{label}_{o}_{s}"]["cell"] == (index, border, off, sign)
    assert len(UNREACHABLE) == 8 and len(BORDER_CELLS) - len(UNREACHABLE) == 22
    assert kernel_status([(192, 62)]) == 0 and kernel_status([(192, 63)]) == 1 and kernel_status([(320, 120)]) == 1
    assert kernel_status([(318, 120)]) == 0 and kernel_status([(120, 118)]) == 0 and kernel_status([(200, 3), (192, 63)]) == 1
    for d in ("ted", "nyq"):
        for t in ("c128", "c64"):
            for depth in (3, 4, 61, 62):
                assert rows[f"fall{depth}_at192_{d}_{t}"]["bursts"] == [(192, depth)] and flush_base(192) + F == 192
            r = rows[f"refuse63_at192_{d}_{t}"]
            assert r["want"] == "refuse" and r["status"] == [0, 1, 0] and r["bursts"][1] == (192, 63)
        assert rows[f"fall62_at448_{d}"]["bursts"] == [(448, 62)] and flush_base(448) + F == 448 and 448 > 256
        assert rows[f"fall120_at318_{d}"]["bursts"] == [(318, 120)] and 318 % F == F - 2 and flush_base(318) + 2 <= 318 - 120
        assert rows[f"fall3_at4_{d}"]["low"] == 1 and rows[f"fall4_at4_{d}"]["last_n"] == [0] and rows[f"fall4_at4_{d}"]["cols"] == 1
        assert rows[f"fall4_at4_beside_{d}"]["bursts"] == [(4, 4), (4, 3)]
        assert rows[f"fall100_at120_{d}"]["bursts"] == [(120, 100)] and flush_base(120) == 0
        assert rows[f"fall62_tail_{d}"]["tail"] > 192 and rows[f"fall62_tail_{d}"]["bursts"] == [(192, 62)]
    assert {rows[name]["dtype"] for name in FALL_ROWS} == {"complex128", "complex64"}
    for n in (2 * C, 2 * C + 1):
        for lpad in (0, 3, 4, 5):
            assert (rows[f"pad{lpad}_len{n}"]["n"], rows[f"pad{lpad}_len{n}"]["p"]["lpad"]) == (n, lpad)
    assert (rows[f"pad{C + 8}_len{C - 3}"]["n"], rows[f"pad{C + 8}_len{C - 3}"]["p"]["lpad"]) == (C - 3, C + 8)
    assert (rows[f"pad{2 * C}_len5"]["n"], rows[f"pad{2 * C}_len5"]["p"]["lpad"]) == (5, 2 * C)
    assert {rows[name]["ends"] for name in PADDING_ROWS} == {"Ln", "input"}
    assert {(rows[name]["ends"], rows[name]["p"]["maxPPM"] > 0) for name in PADDING_ROWS} == {("Ln", True), ("input", False)}
    assert rows["cols5"]["cols"] == 5 and rows["cols7"]["cols"] == 7
    for t in ("float32", "float64", "complex64", "complex128"):
        assert [TIMES_ROWS[f"{g}_{t}"]["guess"] for g in ("both_ways", "high_only", "low_only")] == ["both", "high", "low"]
    for N in (1, 2, 300):
        assert {TIMES_ROWS[f"chosen_N{N}_{f}"]["form"] for f in ("real", "complex", "components")} == {"real", "complex", "components"}
    assert all(TIMES_ROWS[name]["split"] for name in ("components_exact_and_not_c128", "components_exact_and_not_c64"))
    assert [TIMES_ROWS[f"forms_{f}"]["form"] for f in ("real", "complex", "components")] == ["real", "complex", "components"]
    assert {DRIFT_ROWS[f"n{n}"]["n"] for n in (2, 3, 4, 257, 258, 259, 513, 1025)} == {2, 3, 4, 257, 258, 259, 513, 1025}
    assert {len(r["peaks"]) for r in DRIFT_ROWS.values()} >= {1, 3, 5}
    owned = {i for r in DRIFT_ROWS.values() for col in r["peaks"] for i in col}
    assert owned >= {1, 63, 64, 65, 255, 256, 257, 510, 1022} and DRIFT_ROWS["n513"]["peaks"][0][-1] == 513 - 1 - 2
    lane, wave = (lambda i: (i - 1) % 256), (lambda i: (i - 1) % 256 // 64)
    a, b = DRIFT_ROWS["two_waves"]["peaks"][0]
    assert wave(a) != wave(b)
    a, b = DRIFT_ROWS["one_lane"]["peaks"][0]
    assert lane(a) == lane(b) and b == a + 256
    assert {wave(i) for i in DRIFT_ROWS["wave3_only"]["peaks"][0]} == {3}
    assert DRIFT_ROWS["plateau_255_257"]["peaks"] == [[50, 256]] and [i for i, _ in DRIFT_ROWS["plateau_255_257"]["cols"][0][0]][1:] == [255, 256, 257]
    assert DRIFT_ROWS["plateau_to_the_end"]["cols"][0][0][-1][0] == DRIFT_ROWS["plateau_to_the_end"]["n"] - 2
    assert sorted(h for _, h in DRIFT_ROWS["height_half"]["cols"][0][0]) == [0.4375, 0.5, 0.5]
    assert np.mean(drift_expect("mean_zero")[1]) == 0 and np.mean(drift_expect("mean_negative")[1]) < 0


if __name__ == "__main__":
    import sys
    print({name: search(name, tries=20000) for name in (sys.argv[1:] or [n for n in GARDNER_ROWS if n not in FALL_ROWS])})
    print("long table", long_table())
