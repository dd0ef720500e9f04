"""Fixtures, shape rows and the host walk of the IM/DD transmitter and AWGN tests.

The fixtures (tests/golden/imddtx, written by tools/gen_golden_imddtx.py from the reference) and what they must show so that no test
passes emptily are re-asserted by check_conditions.  The shape rows are the smallest sizes at which the kernels can go wrong; their
expected values come from tests/imddtx_restatement.py.  ``Emu`` puts the g++ walk of the kernel bodies (tests/emu/emu_imddtx.cpp) in
the place of the library, so that the public functions -- their checks, draws and layouts -- run without a GPU."""
import glob
import json
import os
import subprocess

import numpy as np

import imddtx_restatement as ir
from opticommpy_amd import _lib, imddtx
from opticommpy_amd.utils import parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imddtx")
BOUND = 1e-12               # of the largest sample of the reference: the bound of the WDM transmitter's tests

PAM_CASES = ["default", "rrc", "pam2", "pam8", "sps1", "sps3", "sps16", "pol2", "mb", "mzm", "retparam"]
MOD_CASES = ["mzm_default", "mzm_er10", "mzm_er80_array", "mzm_complex_drive", "mzm_complex_scalar", "pm_scalar", "pm_array_complex",
             "iqm_default", "iqm_biased", "iqm_real_drive", "mzm_2d"]
AWGN_CASES = ["complex_on_complex", "real_on_complex", "complex_on_real", "real_on_real", "two_columns", "two_columns_real",
              "defaults_global_stream", "real_global_stream"]


def check_files():
    have = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
    want = sorted(["pam_" + c for c in PAM_CASES] + ["mod_" + c for c in MOD_CASES] + ["awgn_" + c for c in AWGN_CASES] + ["sources", "cell_ook"])
    assert have == want


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg"]))
    return g


def make_param(d):
    p = parameters()
    for k, v in d.items():
        setattr(p, k, v)
    return p


def rel_peak(got, want):
    """Largest deviation over the largest sample of the reference."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def host(x):
    return x.get() if hasattr(x, "get") else np.asarray(x)


# ------------------------------------------------------------------ the calls of the fixtures
def mod_call(g, fn=None, convert=lambda a: a):
    """The modulator call of a mod_* fixture through the functions of ``fn`` (the package by default); ``convert`` is applied to
    the array arguments (to_device for the DeviceArray route)."""
    fn = fn or imddtx
    kind, d = g["cfg"]["kind"], g["cfg"]["param"]
    Ei = g["Ei"]
    Ei = (complex(Ei) if np.iscomplexobj(Ei) else float(Ei)) if Ei.shape == () else convert(np.ascontiguousarray(Ei, dtype=np.complex128))
    u = convert(g["u"])
    if kind == "pm":
        return fn.pm(Ei, u, d["Vpi"])
    return getattr(fn, kind)(Ei, u, make_param(d) if d else None)


def mod_restated(g):
    kind, d = g["cfg"]["kind"], g["cfg"]["param"]
    Ei = g["Ei"] if g["Ei"].shape != () else g["Ei"][()]
    if kind == "pm":
        return ir.narrow(ir.pm(Ei, g["u"], d["Vpi"]))
    if kind == "mzm":
        return ir.narrow(ir.mzm(Ei, g["u"], d.get("Vpi", 2), d.get("Vb", -1), d.get("ER", 60)))
    return ir.narrow(ir.iqm(Ei, g["u"], **d))


def pam_restated(symbTx, pulse, d):
    """pamTransmitter's field from its own symbols: (N, nPolModes), flattened for one mode."""
    keys = ("mzmScale", "mzmVpi", "mzmVb", "mzmER", "power")
    kw = {k: d[k] for k in keys if k in d}
    cols = [ir.narrow(ir.pam_field(symbTx[:, m], pulse, d.get("SpS", 16), **kw)[0]) for m in range(symbTx.shape[1])]
    out = np.stack(cols, axis=1)
    return out.reshape(-1) if out.shape[1] == 1 else out


def awgn_seed_global(g):
    """Put numpy's global stream where the generator had it before the reference's call."""
    if int(g["global_seed"]) >= 0:
        np.random.seed(int(g["global_seed"]))


def awgn_restated(g):
    d = g["cfg"]["param"]
    zi = g["zi"] if d.get("complexNoise", True) else None
    return ir.narrow(ir.awgn(g["sig"], g["zr"], zi, d.get("Fs", 1) / d.get("B", 1), 10 ** (d.get("snr", 20) / 10)))


def check_conditions():
    """What tools/gen_golden_imddtx.py asserted when it wrote the fixtures."""
    for c in PAM_CASES:
        g = load("pam_" + c)
        assert float(np.min(g["peak_margin"])) >= 1e-9, c
        sps = g["cfg"]["param"].get("SpS", 16)
        for m in range(g["symbTx"].shape[1]):
            assert ir.peak_margin(ir.shaped(g["symbTx"][:, m], g["pulse"], sps)) >= 1e-9, (c, m)
    g = load("pam_mzm")
    d = g["cfg"]["param"]
    other = pam_restated(g["symbTx"], g["pulse"], dict(d, mzmER=80))
    assert np.max(np.abs(g["sigTxo"] - other)) > 1e-3 * np.max(np.abs(other))
    a, b = load("mod_mzm_er10"), load("mod_mzm_er10")
    b["cfg"] = dict(b["cfg"], param=dict(b["cfg"]["param"], ER=80))
    assert np.max(np.abs(a["out"] - mod_restated(b))) > 1e-3 * np.max(np.abs(a["out"]))
    for c in AWGN_CASES:
        g = load("awgn_" + c)
        cplx = g["cfg"]["param"].get("complexNoise", True)
        pn = np.mean(np.abs(g["out"] - g["sig"]) ** 2)
        want = float(g["sigma2"]) * (1 if cplx else 0.5)
        assert abs(pn / want - 1) <= 0.1, (c, pn, want)


# ------------------------------------------------------------------ shape rows
# pamTransmitter through the public function: what is set on the parameter object
PAM_ROWS = {f"N{n}": dict(nBits=2 * n, SpS=1, pulseType="rrc", nFilterTaps=8, seed=100 + n) for n in (1, 2, 255, 256, 257)}
PAM_ROWS.update({f"sps{s}": dict(nBits=2 * (40 + s), SpS=s, seed=200 + s) for s in range(1, 18)})
PAM_ROWS.update({
    "one_symbol": dict(nBits=2, SpS=16, seed=301),
    "N_equals_ntaps": dict(nBits=32, SpS=4, pulseType="rrc", nFilterTaps=64, seed=302),
    "taps_longer_than_signal": dict(nBits=16, SpS=4, pulseType="rc", nFilterTaps=100, pulseRollOff=0.3, seed=303),
    "two_blocks": dict(nBits=2 * 300, SpS=1, pulseType="rrc", nFilterTaps=16, seed=304),
    "pol1": dict(nBits=200, SpS=5, nPolModes=1, seed=305),
    "pol2": dict(nBits=200, SpS=5, nPolModes=2, seed=306, mzmER=25, mzmVb=1.1),
    "pol3": dict(nBits=200, SpS=5, nPolModes=3, seed=307, power=1.5, M=2),
})
# the signal path with chosen symbols and one tap (the shaped signal is the symbol stream): where the peak sits
PEAK_ROWS = {"peak_first": (700, 0), "peak_last": (700, 699), "peak_last_lane_of_block": (700, _lib.TX_BLOCK - 1),
             "peak_first_of_second_block": (700, _lib.TX_BLOCK), "peak_alone": (1, 0), "peak_negative": (513, 512)}
EW_SPAN = _lib.TX_EW_BLOCKS * _lib.TX_BLOCK          # elements one sweep of an element-wise launch covers


def peak_row(rid):
    n, at = PEAK_ROWS[rid]
    rng = np.random.default_rng(n + at)
    s = rng.uniform(-0.7, 0.7, n)
    s[at] = -1.3 if rid == "peak_negative" else 1.3
    return s


def run_peak_row(rid, device_output=False):
    """(field, expected) of a peak row through the backend in place."""
    from opticommpy_amd import device as dev
    s = peak_row(rid)
    kw = dict(mzmScale=0.4, mzmVpi=3.0, mzmVb=1.2, mzmER=30.0, power=0.5)
    out = dev.empty(device_output, (len(s), 1), np.complex128)
    amp = float(np.sqrt(1e-3 * 10 ** (kw["power"] / 10)))
    imddtx._backend.pam_tx(len(s), 1, 1, np.ones(1), np.ascontiguousarray(s.reshape(1, -1)), kw["mzmScale"], kw["mzmVpi"], -kw["mzmVb"],
                           kw["mzmER"], amp, out)
    return host(out).reshape(-1), ir.narrow(ir.pam_field(s, np.ones(1), 1, **kw)[0])


def mod_row_inputs(n, kind, seed=0):
    rng = np.random.default_rng(1000 + n % 1000 + seed)
    u = rng.uniform(-20, 20, n) * 2
    if kind == "iqm":
        u = u + 1j * rng.uniform(-20, 20, n) * 2
    Ei = np.sqrt(rng.uniform(0.5, 2, n)) * np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    return Ei, u


MOD_ROW_SIZES = (1, 2, 255, 256, 257)
_SPAN_CACHE = {}


def span_row(n):
    """mzm at one sample either side of the element-wise launch's grid-stride span; the restatement is computed once."""
    if n not in _SPAN_CACHE:
        Ei, u = mod_row_inputs(n, "mzm")
        _SPAN_CACHE[n] = (Ei, u, ir.narrow(ir.mzm(Ei, u, 2, -0.6, 25)))
    return _SPAN_CACHE[n]


# ------------------------------------------------------------------ the host walk in the library's place
def build_emu(exe, flags=("-O2",)):
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-I",
                           os.path.join(ROOT, "opticommpy_amd", "csrc"), os.path.join(ROOT, "tests", "emu", "emu_imddtx.cpp"), "-o", str(exe)])
    return str(exe)


def shaped_host(symbols, pulse, SpS):
    """The pulse-shaping filter in double precision on the host: what the overlap-save launch hands the kernels walked here."""
    return np.stack([ir.narrow(ir.shaped(s, pulse, SpS)) for s in symbols])


class Emu:
    """imddtx._backend with every library call replaced by a run of the emulator program."""

    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.calls = exe, tmp, []

    def _run(self, head, *arrays):
        hd = np.zeros(16, dtype=np.int64)
        hd[:len(head)] = head
        src, dst = os.path.join(str(self.tmp), "in.bin"), os.path.join(str(self.tmp), "out.bin")
        with open(src, "wb") as f:
            f.write(hd.tobytes())
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([self.exe, src, dst])
        self.calls.append(int(hd[0]))
        return np.fromfile(dst, dtype=np.float64)

    @staticmethod
    def _store(out, vals):
        out[...] = vals.view(out.dtype).reshape(out.shape)

    def pam_tx(self, nSymbols, SpS, nPol, pulse, symbols, mzmScale, Vpi, Vb, ER, amp, sig):
        sh = shaped_host(symbols, pulse, SpS)
        self._store(sig, self._run([0, nSymbols * SpS, nPol], np.array([mzmScale, Vpi, Vb, ER, amp]), sh))

    def modulate(self, kind, n, u, Ei, ei0, Vpi, VbI, VbQ, Vphi, ERI, ERQ, out):
        prm = np.array([ei0.real, ei0.imag, Vpi, VbI, VbQ, Vphi, ERI, ERQ])
        arrays = [prm, u] + ([Ei] if Ei is not None else [])
        self._store(out, self._run([1, n, _lib.MOD_KINDS[kind], int(u.dtype.kind == "c"), int(Ei is not None)], *arrays))

    def awgn(self, n, ncols, sig, out, complexNoise, FsB, snr_lin, un, dev_seed):
        arrays = [np.array([FsB, snr_lin]), sig] + ([un] if un is not None else [])
        head = [2, n, ncols, int(sig.dtype.kind == "c"), int(out.dtype.kind == "c"), int(complexNoise), int(un is not None), dev_seed]
        self._store(out, self._run(head, *arrays))

    def stuff(self, rows, w, factor, scale, x, out):
        self._store(out, self._run([3, rows, w, factor], np.array([scale]), x.view(np.float64) if x.dtype.itemsize % 8 == 0 else x))
