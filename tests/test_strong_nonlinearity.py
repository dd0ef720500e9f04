"""The strongly nonlinear regime: nonlinear phase rotations far beyond a quarter turn per step.

Every column-stage kernel turns the angle gamma (8/9) P hz into a rotation through cis_t<T> and forms lim one iteration ahead
through sin_half_angle (opticommpy_amd/csrc/fused_core.h).  Both have a polynomial for small arguments and a separate
reduction for the rest, and on the device the reductions of cis_t<float> and sin_half_angle are code that only hipcc compiles.
Elsewhere in the suite the peak angle per step stays below 0.05 rad; here it is 6 ... 40 rad (and one sample near 1e3 rad).

1. Closed form.  D = 0, alpha = 0, amp = None: the linear operator is the identity and n steps give E exp(+-j c P hz n)
   exactly, c = gamma 8/9 and P = |Ex|^2 + |Ey|^2 of the sample's own pair for the Manakov functions (the pairs of a K = 2
   call share step sizes and the convergence test, not the power: Pch keeps one row per pair, channels.py:388), c = gamma and
   P = |E|^2 for ssfm.  The input sweeps the angle over [0, 40] rad, with samples at k pi/4 and one ulp / 1e-9 to either
   side.  complex128: rel-L2 <= 1e-13 against the closed form evaluated in long double -- two transforms of at most 2^22
   points cost ~ log2(N) 2^-53 each, the angle's own rounding 40 x 2^-52 ~ 1e-14; the bound is ten times that.  complex64: the
   distance of the oracle's complex64 run from the closed form is d_ref; the HIP result must stay within 4 d_ref (the two sides
   round the angle in different places; a wrong quadrant is O(1)).  The oracle's ssfm applies prec as the cupy twin does;
   for manakovDBP its forward complex64 run, mirrored, is the yardstick (_closed_reference says why).
2. Oracle parity with dispersion on: 30 ... 36 dBm, D = 16, 1 ... 3 steps of 0.5 ... 1 km, fixed and adaptive
   (maxNlinPhaseRot = 1.5), manakovDBP on the forward result, K = 2, ssfm.  complex128 under parity_gate, which must come
   back as TOL_C128 (a few steps at these powers are well conditioned; only the reference's 80-step runs are chaotic);
   complex64 within 4 d_ref, d_ref = oracle complex64 against oracle complex128.
3. The reference's own 2 W set-ups (ssfm_ref_spm, ssfm_ref_power) cut to their first 2 and 4 steps: values, not only power.
4. Every stage family (table below), fused and rocFFT engines on the GPU, the emulated kernels on the CPU.

Stage families (fused engine; read off choose_split / choose_nonpow2_split / FusedCore::init / launch_col, pinned by
test_the_lengths_take_the_stage_families_of_the_table):

  complex128 manakovSSF
    2^12      64 x 64, field does not fill the chip: 8-value kernels     k_col8<double, 6, CM_MK>, k_row8<double, 512, 6>
    2^16      256 x 256, 8-value kernels                                 k_col8<double, 8, CM_MK>, k_row8<double, 512, 8>
    2^20      256 x 4096 (BASELINE config 2), 16-value, stage groups     k_col<double, 8, CM_MK, 0, SG_*>, k_row<double, 256, 2, 12>
    48 000    2^7 columns x 375 mixed-radix rows, ragged last tile       k_col_ragged<double, 7, CM_MK>, k_row_mixed
    9 000     120 x 75, both factors mixed-radix                         k_col_mixed<double, CM_MK> (col_mixed_body), k_row_mixed
    200 000   125 x 1600 (2^6 columns would leave the chip idle)         k_col_mixed<double, CM_MK>, k_row_mixed
    6 000     80 x 75: four factors of two, so the mixed-radix columns   k_col_mixed<double, CM_MK>, k_row_mixed
              take it (not the one-launch rows)
    3 000     general engine, one-launch LDS rows (pipeline fused-rows)  k_rows + the elementwise kernels of engine_rocfft.hip
    97, 10 007  general engine, Bluestein (pipeline fused-bluestein)     FusedConv + the same elementwise kernels
  complex64 manakovSSF
    2^14      packed pairs, 128 x 128                                    k_col_pk<7>
    2^16      packed pairs, 256 x 256, 8-value                           k_col_pk8<8>
    2^22      packed pairs, 1024 x 4096 (BASELINE config 3)              k_col_pk<10, 0, SG_*>
    2^14, SSF_C64_PACKED=0   one row per polarisation                    k_col<float, 7, CM_MK>
    9 000     120 x 75 (no packed mixed-radix kernels)                   k_col_mixed<float, CM_MK>
    48 000    2^7 x 375                                                  k_col_ragged<float, 7, CM_MK>
  ssfm
    2^12, 2^16    k_col8<double, LG, CM_NLSE_FIRST / STEP / LAST>        10 125, 6 000   k_col_mixed<double, CM_NLSE_*>
    2^14 complex64    k_col<float, 7, CM_NLSE_*>
  The rocFFT engine runs every length on rocFFT transforms and the elementwise kernels of engine_rocfft.hip.

Measured (fused, rocfft: on an MI355X; emu: the emulated kernels; oracle: the oracle itself against the closed form).  The
bounds are the derived / reference-measured ones above, never these figures.  The complex128 distances sit a few times above
the oracle's own because the transforms' rounding of |E_fd|^2 enters the next angle multiplied by the angle itself
(theta x log2(N) x 2^-53 ~ 40 x 2e-15): that, not the angle's last bit, is what the 1e3 rad sample shows -- 2.0e-12 at 2^16 on
the fused engine, inside 1e3 x 2^-52 x 10 = 2.2e-12 by a tenth.  One step in the family-wide sweep (total angle 40 rad, what
the 1e-13 was derived for); the cases marked 2x0.5km take the same total angle in two steps.

  Closed form, complex128: rel-L2 to the closed form (bound 1e-13) | the 1e3 rad sample alone (bound 2.2e-12)
    case                                        oracle     emu   fused  rocfft |     emu   fused  rocfft
    manakovSSF-4096-complex128                 8.3e-15 2.1e-14 2.1e-14 1.1e-14 | 1.9e-13 1.1e-13 4.0e-13
    manakovSSF-4096-complex128-2x0.5km         1.5e-14 3.8e-14 3.9e-14 2.1e-14 | 1.0e-13 1.2e-13 5.7e-13
    manakovDBP-4096-complex128-2x0.5km         1.5e-14 3.8e-14 3.8e-14 2.1e-14 | 1.0e-13 6.3e-14 5.7e-13
    ssfm-4096-complex128-2x0.5km               1.9e-14 3.7e-14 3.5e-14 2.3e-14 | 2.3e-14 2.9e-13 6.9e-13
    manakovSSF-9000-complex128-2x0.5km         1.4e-14 2.3e-14 2.6e-14 1.7e-14 | 4.2e-13 2.9e-14 1.5e-13
    manakovSSF-65536-complex128                1.1e-14 2.5e-14 2.4e-14 9.5e-15 | 5.3e-13 2.0e-12 2.1e-13
    manakovSSF-48000-complex128                1.5e-14 4.0e-14 3.7e-14 1.1e-14 | 1.5e-12 1.8e-12 1.5e-13
    manakovSSF-9000-complex128                 9.4e-15 1.4e-14 1.5e-14 1.1e-14 | 4.2e-13 1.4e-13 9.0e-14
    manakovSSF-6000-complex128                 1.7e-14 1.7e-14 2.0e-14 1.2e-14 | 6.5e-13 8.7e-13 3.7e-13
    manakovDBP-4096-complex128                 8.1e-15 2.1e-14 2.1e-14 1.1e-14 | 1.9e-13 1.1e-13 5.6e-14
    manakovSSF-4096-complex128-K2              8.2e-15 2.1e-14 2.2e-14 1.0e-14 |    -       -       -
    ssfm-4096-complex128                       1.4e-14 2.7e-14 2.6e-14 1.9e-14 | 6.7e-14 1.8e-13 5.7e-13
    ssfm-65536-complex128                      1.8e-14 3.2e-14 2.8e-14 1.8e-14 | 8.8e-13 1.7e-12 2.9e-13
    ssfm-10125-complex128                      1.8e-14 2.8e-14 3.1e-14 2.1e-14 | 1.0e-12 1.2e-12 1.9e-14
    ssfm-6000-complex128                       1.9e-14 2.2e-14 2.3e-14 1.7e-14 | 7.8e-13 7.3e-13 2.2e-13
    manakovSSF-1048576-complex128              1.3e-14    -    5.4e-14 1.1e-14 |    -    9.1e-13 1.7e-13
    manakovSSF-200000-complex128               1.1e-14    -    3.7e-14 1.0e-14 |    -    1.0e-12 1.5e-13
    manakovSSF-3000-complex128                 1.0e-14    -    3.1e-14 1.2e-14 |    -    5.7e-13 2.3e-13
    manakovSSF-97-complex128                   5.3e-15    -    1.9e-14 7.3e-15 |    -    1.8e-12 2.0e-13
    manakovSSF-10007-complex128                2.9e-14    -    4.8e-14 2.0e-14 |    -    5.7e-13 9.1e-13
  Closed form, complex64: d_ref = oracle complex64 to the closed form; bound 4 d_ref
    case                                         d_ref     emu   fused  rocfft
    manakovSSF-16384-complex64-2x0.5km         4.7e-06 4.4e-06 4.4e-06 1.4e-05
    manakovSSF-16384-complex64                 3.0e-06 3.6e-06 3.6e-06 7.1e-06
    manakovSSF-16384-complex64-unpacked        3.0e-06 3.6e-06 3.6e-06    -
    manakovSSF-9000-complex64                  3.9e-06 3.8e-06 3.8e-06 6.0e-06
    manakovSSF-48000-complex64                 3.5e-06 4.0e-06 4.0e-06 4.9e-06
    manakovDBP-16384-complex64                 3.0e-06 3.6e-06 3.6e-06 7.1e-06
    ssfm-16384-complex64                       5.8e-06 6.0e-06 6.0e-06 1.1e-05
    manakovSSF-65536-complex64                 3.1e-06    -    3.7e-06 7.5e-06
    manakovSSF-4194304-complex64               3.6e-06    -    4.2e-06 9.3e-06
  Dispersion on, complex64: d_ref = oracle complex64 to oracle complex128; bound 4 d_ref
    case                                        peak   d_ref     emu   fused  rocfft
    manakovSSF-16384-complex64-wideband          8.5 6.7e-07 6.7e-07 6.4e-07 1.7e-06
    manakovSSF-16384-complex64                  17.0 1.4e-06 1.6e-06 1.4e-06 3.9e-06
    manakovSSF-16384-complex64-unpacked         17.0 1.4e-06 1.6e-06 1.6e-06    -
    manakovSSF-9000-complex64                   14.9 1.8e-06 1.4e-06 1.3e-06 2.5e-06
    manakovSSF-48000-complex64                  17.7 5.6e-07 7.9e-07 5.9e-07 8.4e-07
    ssfm-16384-complex64                        15.1 1.4e-06 1.3e-06 1.3e-06 3.0e-06
    manakovSSF-65536-complex64                  15.6 1.4e-06    -    1.4e-06 4.1e-06
    manakovSSF-4194304-complex64                21.8 1.5e-06    -    1.6e-06 5.1e-06
  Dispersion on, complex128 (gate = TOL_C128 = 1e-10 in every case): rel-L2 to the oracle
    case                                        peak     emu   fused  rocfft
    manakovSSF-4096-complex128                  11.4 1.0e-14 1.2e-14 5.1e-15
    manakovSSF-16384-complex128-wideband         8.5 5.1e-15 4.7e-15 2.6e-15
    manakovSSF-65536-complex128                 31.2 1.3e-14 1.1e-14 5.1e-15
    manakovSSF-48000-complex128                 17.7 6.4e-15 6.1e-15 2.6e-15
    manakovSSF-9000-complex128                  29.7 4.0e-14 2.7e-14 3.9e-14
    manakovSSF-9000-complex128-3x0.5km          14.9 1.4e-14 1.5e-14 1.1e-14
    manakovSSF-6000-complex128                   6.5 9.0e-15 9.1e-15 9.4e-15
    manakovSSF-4096-complex128-adaptive          1.5 5.3e-15 6.1e-15 3.9e-15
    manakovDBP-4096-complex128-of-forward       11.2 1.9e-14 2.0e-14 7.5e-15
    manakovSSF-4096-complex128-K2               11.4 8.5e-15 9.5e-15 4.5e-15
    ssfm-4096-complex128                        10.1 6.4e-15 6.8e-15 4.0e-15
    ssfm-65536-complex128                       13.4 3.2e-15 3.5e-15 2.2e-15
    ssfm-10125-complex128                       12.4 7.9e-15 8.6e-15 5.1e-15
    ssfm-6000-complex128                        12.9 6.1e-15 5.9e-15 5.1e-15
    manakovSSF-1048576-complex128               20.1    -    8.1e-15 2.2e-15
    manakovSSF-200000-complex128                18.5    -    5.6e-15 2.4e-15
    manakovSSF-3000-complex128                  14.2    -    1.5e-14 4.9e-15
    manakovSSF-97-complex128                     7.4    -    1.4e-14 5.8e-15
    manakovSSF-10007-complex128                 13.0    -    3.0e-14 1.5e-14
"""
import logging

import numpy as np
import pytest

import emu_binding as eb
from helpers import load_golden, make_param, parity_gate, rel_l2, synth_field
from oracle import ssf_oracle as orc

TOL_C128, TOL_C64 = 1e-10, 5e-4
TOL_CLOSED = 1e-13                       # derived in the module docstring
GAMMA = 1.3
QUARTER = np.pi / 4
BASE = dict(Fs=512e9, Fc=193.1e12, gamma=GAMMA, maxIter=10, tol=1e-5, prgsBar=False, saveSpanN=[])
ORC = {"ssfm": orc.ssfm, "manakovSSF": orc.manakovSSF, "manakovDBP": orc.manakovDBP}


@pytest.fixture(autouse=True)
def _quiet_and_reset():
    """The fixed-step cases with dispersion do not converge in maxIter iterations on either side: the reference's warning,
    one per step, is expected."""
    logging.disable(logging.WARNING)
    yield
    logging.disable(logging.NOTSET)
    import opticommpy_amd as oa
    oa.set_engine("auto")


def _coef(func):
    return GAMMA if func == "ssfm" else GAMMA * 8 / 9


def _case_id(c):
    return "-".join(str(c[k]) for k in ("func", "N", "prec") if k in c) + c.get("tag", "")


# ------------------------------------------------------------------------------------------ 1. closed form
def _sweep_angles(n, real, huge):
    """n target angles: k pi/4 +- {0, 1 ulp, 1e-9} for k = 0 ... 16, one exact zero, (complex128 only) one near 1e3 rad, and
    a fine grid over (0, 40] for the rest, dealt over the positions by a fixed permutation so that every tile of every
    stage geometry sees the whole range.  Returns (angles, index of the 1e3 rad sample or None)."""
    sp = []
    for k in range(17):
        b = real(k * QUARTER)
        sp += [b, np.nextafter(b, real(np.inf)), np.nextafter(b, real(-np.inf)), real(float(b) + 1e-9), real(float(b) - 1e-9)]
    sp = [float(x) for x in sp if x >= 0] + [0.0] + ([1.0e3 * (1 + 2.0 ** -30)] if huge else [])
    assert n > len(sp)
    m = n - len(sp)
    a = np.concatenate([np.array(sp), np.linspace(0.0, 40.0, m + 1)[1:]])
    perm = np.random.default_rng(20241).permutation(n)
    out = np.empty(n)
    out[perm] = a
    return out, (int(perm[len(sp) - 1]) if huge else None)


def _sweep_field(func, N, prec, K=1):
    """Deterministic field whose per-sample angle c P hz (hz = 1 km) sweeps _sweep_angles: fixed random phases and, for the
    Manakov functions, a fixed random split of P between x and y.  K pairs get the sweep in different orders."""
    dt = np.dtype(prec).type
    real = np.float32 if dt == np.complex64 else np.float64
    rng = np.random.default_rng(N + 7 * K)
    ang, huge = _sweep_angles(N, real, dt == np.complex128 and K == 1)
    c = _coef(func)
    if func == "ssfm":
        E = np.sqrt(ang / c) * np.exp(2j * np.pi * rng.random(N))
        return E.astype(dt), huge
    cols = []
    for k in range(K):
        a = np.roll(ang, 1237 * k)
        f = 0.2 + 0.6 * rng.random(N)
        cols.append(np.sqrt(f * a / c) * np.exp(2j * np.pi * rng.random(N)))
        cols.append(np.sqrt((1 - f) * a / c) * np.exp(2j * np.pi * rng.random(N)))
    return np.stack(cols, axis=1).astype(dt), huge


def _angles_of(func, E, hz):
    """The per-step angle of every sample, (N, K), from the input alone."""
    E2 = np.asarray(E, dtype=np.complex128).reshape(len(E), -1)
    P = np.abs(E2) ** 2
    if func != "ssfm":
        P = P[:, 0::2] + P[:, 1::2]
    return _coef(func) * P * hz


def _assert_sweep_covers(func, E, hz):
    a = _angles_of(func, E, hz)
    octants = np.unique(np.floor(a / QUARTER).astype(np.int64) % 8)
    assert list(octants) == list(range(8)), octants
    assert np.mean(a > QUARTER) >= 0.9
    assert np.any(a == 0.0) and a.max() >= 39.0
    near = np.abs(a[:, :1] - QUARTER * np.arange(1, 17)[None, :])
    assert np.all(near.min(axis=0) <= 1e-5)                      # a sample at every multiple of pi/4 up to 4 pi


def _closed_form(func, E, hz, nsteps):
    """E exp(sign j c P hz nsteps) in long double, rounded to complex128; same shape as E."""
    E2 = np.asarray(E).reshape(len(E), -1)
    re, im = E2.real.astype(np.longdouble), E2.imag.astype(np.longdouble)
    P = re * re + im * im
    if func == "ssfm":
        c = np.longdouble(GAMMA)
    else:
        c = np.longdouble(GAMMA) * 8 / 9
        P = np.repeat(P[:, 0::2] + P[:, 1::2], 2, axis=1)
    th = (-1 if func == "manakovDBP" else 1) * c * P * np.longdouble(hz) * nsteps
    co, si = np.cos(th), np.sin(th)
    out = (re * co - im * si).astype(np.float64) + 1j * (re * si + im * co).astype(np.float64)
    return out.reshape(np.shape(E))


def _closed_cfg(func, prec, nsteps=1, hz=1.0):
    return dict(BASE, func=func, alpha=0.0, D=0, Ltotal=nsteps * hz, Lspan=nsteps * hz, hz=hz, nlprMethod=False, amp=None, prec=prec)


def _drop(x, idx):
    return x if idx is None else np.delete(x, idx, axis=0)


_oracle_cache = {}


def _cached(key, fn):
    """The last case's oracle results: the engines (and the emulator) of one case run back to back."""
    if key not in _oracle_cache:
        _oracle_cache.clear()
        _oracle_cache[key] = fn()
    return _oracle_cache[key]


def _closed_reference(c):
    func, N, prec = c["func"], c["N"], c["prec"]
    E, huge = _sweep_field(func, N, prec, c.get("K", 1))
    nsteps, hz = c.get("nsteps", 1), c.get("hz", 1.0)
    cfg = _closed_cfg(func, prec, nsteps, hz)
    _assert_sweep_covers(func, E, 1.0)
    assert _angles_of(func, E, hz).max() * nsteps <= 40.0 * (1 + 1e-6) or c["prec"] == "complex128"     # (the 1e3 rad sample)
    exact = _closed_form(func, E, hz, nsteps)
    tr = {}
    if func == "manakovDBP" and prec == "complex64":
        # With numpy >= 2 the oracle's back-propagation leaves single precision at its first `Ex * np.exp(0)` (a float64 scalar
        # promotes the complex64 field), so its complex64 run says nothing about single-precision rounding.  With the identity
        # as linear operator DBP(E) = conj(SSF(conj(E))) exactly: the oracle's forward complex64 run, mirrored, is the yardstick.
        ref = np.conj(orc.manakovSSF(np.conj(E), make_param(orc.parameters, dict(cfg, func="manakovSSF")), trace=tr))
    else:
        ref = ORC[func](E, make_param(orc.parameters, cfg), trace=tr)
    return E, huge, cfg, exact, ref, tr


def _check_lims(lims, ref_lims):
    """lim values against the oracle's where they mean something.  With the identity as linear operator iterate 1 repeats
    iterate 0, so lim_1 is |rounding| / |E| on both sides, ~1e-16 (1e-7 in single precision) with a value that depends on each
    side's rounding: a relative comparison there would compare noise.  Only values above 1e-9 are compared."""
    assert len(lims) == len(ref_lims)
    for got, want in zip(lims, ref_lims):
        got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
        assert len(got) == len(want)
        keep = want > 1e-9
        assert keep.any()
        np.testing.assert_allclose(got[keep], want[keep], rtol=1e-6)


def _check_closed(c, who, out, run_iters, run_lims):
    """`out` (shape of the input) of implementation `who` on closed-form case c."""
    E, huge, cfg, exact, ref, tr = _cached(("closed", _case_id(c)), lambda: _closed_reference(c))
    out = np.asarray(out).reshape(exact.shape)
    d_ref = rel_l2(_drop(ref, huge), _drop(exact, huge))
    d = rel_l2(_drop(out, huge), _drop(exact, huge))
    print(f"STRONG closed {_case_id(c)} {who}: oracle-to-exact {d_ref:.3e}, {who}-to-exact {d:.3e}")
    if c["prec"] == "complex128":
        assert d_ref <= TOL_CLOSED                               # the oracle confirms the closed form (and its sign for manakovDBP)
        assert d <= TOL_CLOSED
        if huge is not None:                                     # the sample near 1e3 rad on its own: its angle's rounding, ten times
            e_h = np.linalg.norm(out[huge] - exact[huge]) / np.linalg.norm(exact[huge])
            print(f"STRONG closed {_case_id(c)} {who}: 1e3 rad sample {e_h:.3e}")
            assert e_h <= 1e3 * 2.0 ** -52 * 10
    else:
        assert d_ref <= 1e-4                                     # single precision, not a wrong closed form
        assert d <= 4 * d_ref
    if c["func"] != "ssfm":
        assert tr["iters"] == [2] * c.get("nsteps", 1)
        if c["prec"] == "complex128":
            assert [int(x) for x in run_iters] == tr["iters"]
            _check_lims(run_lims, tr["lims"])
        else:       # lim_1 is single-precision noise, 1e-6 ... 1e-5 at these lengths, against tol = 1e-5: the suite's complex64 rule
            assert abs(int(np.sum(run_iters)) - int(np.sum(tr["iters"]))) <= 2


def _c(func, N, prec="complex128", **kw):
    return dict(func=func, N=N, prec=prec, **kw)


TWO = dict(nsteps=2, hz=0.5, tag="-2x0.5km")      # two steps of half the length: the same total angle, the step-to-step hand-over
CLOSED_EMU = [_c("manakovSSF", 1 << 12), _c("manakovSSF", 1 << 12, **TWO), _c("manakovDBP", 1 << 12, **TWO),
              _c("ssfm", 1 << 12, **TWO),
              _c("manakovSSF", 1 << 14, "complex64", **TWO), _c("manakovSSF", 9000, **TWO),
              _c("manakovSSF", 1 << 16), _c("manakovSSF", 48000), _c("manakovSSF", 9000),
              _c("manakovSSF", 6000), _c("manakovDBP", 1 << 12), _c("manakovSSF", 1 << 12, K=2, tag="-K2"),
              _c("ssfm", 1 << 12), _c("ssfm", 1 << 16), _c("ssfm", 10125), _c("ssfm", 6000),
              _c("manakovSSF", 1 << 14, "complex64"), _c("manakovSSF", 1 << 14, "complex64", packed=0, tag="-unpacked"),
              _c("manakovSSF", 9000, "complex64"), _c("manakovSSF", 48000, "complex64"), _c("manakovDBP", 1 << 14, "complex64"),
              _c("ssfm", 1 << 14, "complex64")]
CLOSED_GPU = CLOSED_EMU + [_c("manakovSSF", 1 << 20), _c("manakovSSF", 200000), _c("manakovSSF", 3000), _c("manakovSSF", 97),
                           _c("manakovSSF", 10007), _c("manakovSSF", 1 << 16, "complex64"), _c("manakovSSF", 1 << 22, "complex64")]


def _emu_run(c, E, cfg, monkeypatch):
    if "packed" in c:
        monkeypatch.setenv("SSF_C64_PACKED", str(c["packed"]))
    out, info = eb.run(cfg["func"], E, cfg)
    return (out[0] if cfg["func"] == "ssfm" else out.T), info


@pytest.mark.parametrize("c", CLOSED_EMU, ids=_case_id)
def test_closed_form_rotation_on_the_emulated_kernels(c, monkeypatch):
    E, _, cfg, *_ = _cached(("closed", _case_id(c)), lambda: _closed_reference(c))
    out, info = _emu_run(c, E, cfg, monkeypatch)
    _check_closed(c, "emu", out, info["iters"], info["lims"])


def test_the_closed_form_has_the_sign_of_the_oracle_and_a_wrong_quadrant_is_seen():
    """The check is sharp: a rotation into the neighbouring quadrant at the samples above pi/4 (what a slip in a reduction's
    sign logic gives), or the forward sign for manakovDBP, is an O(1) distance."""
    for func in ("manakovSSF", "manakovDBP", "ssfm"):
        E, huge = _sweep_field(func, 4096, "complex128")
        exact = _closed_form(func, E, 1.0, 1)
        ref = ORC[func](E, make_param(orc.parameters, _closed_cfg(func, "complex128")))
        assert rel_l2(ref, exact) <= TOL_CLOSED
        assert rel_l2(ref, np.conj(exact) * (E / np.conj(np.where(E == 0, 1, E)))) > 0.5          # the opposite sign
        big = (_angles_of(func, E, 1.0) > QUARTER).repeat(1 if func == "ssfm" else 2, axis=1).reshape(E.shape)
        assert rel_l2(np.where(big, 1j * exact, exact), exact) > 0.5


# ------------------------------------------------------------------------------------------ 2. oracle parity with dispersion on
def _strong_field(c):
    N, K, prec = c["N"], c.get("K", 1), np.dtype(c["prec"]).type
    if c["func"] == "ssfm":
        return synth_field(N, 1, 41, c["dbm"], prec)[:, 0].copy()
    if K == 1:
        return synth_field(N, 2, 41, c["dbm"], prec)
    return np.concatenate([synth_field(N, 2, 41 + k, c["dbm"] - 3.0 * k, prec) for k in range(K)], axis=1)


def _strong_cfg(c):
    hz, nsteps = c.get("hz", 1.0), c.get("nsteps", 2)
    cfg = dict(BASE, func=c["func"], Fs=c.get("Fs", 64e9), alpha=0.2, D=16, Ltotal=nsteps * hz, Lspan=nsteps * hz, hz=hz,
               nlprMethod=False, amp="ideal", prec=c["prec"])
    if c.get("adaptive"):
        cfg.update(nlprMethod=True, maxNlinPhaseRot=1.5, Ltotal=c["L"], Lspan=c["L"])
    return cfg


def _peak_angle(c, E, cfg):
    """Largest nonlinear angle of the first step, from the input alone (an adaptive step turns max(phi) hz into
    maxNlinPhaseRot exactly)."""
    if c.get("adaptive"):
        return cfg["maxNlinPhaseRot"]
    return float(_angles_of("ssfm" if c["func"] == "ssfm" else "manakovSSF", E, cfg["hz"]).max())


def _strong_reference(c):
    cfg = _strong_cfg(c)
    E = _strong_field(c)
    func = c["func"]
    if func == "manakovDBP":                                      # back-propagation of the forward result
        E = orc.manakovSSF(E, make_param(orc.parameters, dict(cfg, func="manakovSSF"))).astype(E.dtype)
    assert _peak_angle(c, E, cfg) > QUARTER
    tr = {}
    E128, cfg128 = E.astype(np.complex128), dict(cfg, prec="complex128")
    ref = ORC[func](E128, make_param(orc.parameters, cfg128), trace=tr)
    if c["prec"] == "complex128":
        gate = parity_gate(func, E, cfg, TOL_C128)
        assert gate == TOL_C128                                   # well conditioned: the plain tolerance holds
        return E, cfg, ref, tr, gate
    tr64 = {}
    ref64 = ORC[func](E, make_param(orc.parameters, cfg), trace=tr64)
    d_ref = rel_l2(ref64, ref)
    assert d_ref <= TOL_C64
    return E, cfg, ref, tr, d_ref


def _check_strong(c, who, out, run):
    E, cfg, ref, tr, bound = _cached(("strong", _case_id(c)), lambda: _strong_reference(c))
    out = np.asarray(out).reshape(ref.shape)
    d = rel_l2(out, ref)
    print(f"STRONG parity {_case_id(c)} {who}: peak angle {_peak_angle(c, E, cfg):.2f} rad, "
          f"{'gate' if c['prec'] == 'complex128' else 'd_ref'} {bound:.3e}, {who}-to-oracle {d:.3e}, iters {tr.get('iters')}")
    if c["prec"] == "complex128":
        assert d <= bound
    else:
        assert d <= 4 * bound
    assert run["steps"] == tr["steps"]
    if c["func"] == "ssfm":
        return
    if c["prec"] == "complex128":
        assert [int(x) for x in run["iters"]] == tr["iters"]
        # (the oracle answers a 1e-15 perturbation of these inputs with < 1e-12 -- parity_gate above -- so every lim, the ones of
        #  steps that do not converge included, is reproducible far below the suite's usual 1e-6)
        flat, want = np.concatenate([np.asarray(x, dtype=float) for x in run["lims"]]), np.concatenate(tr["lims"])
        np.testing.assert_allclose(flat, want, rtol=1e-6)
        if c.get("adaptive"):
            np.testing.assert_allclose(run["hz"], tr["hz"], rtol=1e-9)
    else:
        assert abs(int(np.sum(run["iters"])) - tr["iterations"]) <= 2


def _s(func, N, prec="complex128", dbm=33.0, **kw):
    return dict(func=func, N=N, prec=prec, dbm=dbm, **kw)


WIDE = dict(dbm=30.0, Fs=512e9, tag="-wideband")   # eight times the bandwidth: dispersion moves the power within one step, the phase
#                                                    of 1 % of the samples changes by more than a quarter turn between iterates
STRONG_EMU = [_s("manakovSSF", 1 << 12), _s("manakovSSF", 1 << 14, **WIDE), _s("manakovSSF", 1 << 14, "complex64", **WIDE),
              _s("manakovSSF", 1 << 16, dbm=36.0, nsteps=1), _s("manakovSSF", 48000, nsteps=1),
              _s("manakovSSF", 9000, dbm=36.0), _s("manakovSSF", 9000, dbm=36.0, hz=0.5, nsteps=3, tag="-3x0.5km"),
              _s("manakovSSF", 6000, dbm=30.0, nsteps=3),
              _s("manakovSSF", 1 << 12, dbm=30.0, adaptive=True, L=1.0, tag="-adaptive"),
              _s("manakovDBP", 1 << 12, tag="-of-forward"), _s("manakovSSF", 1 << 12, dbm=36.0, K=2, hz=0.5, tag="-K2"),
              _s("ssfm", 1 << 12), _s("ssfm", 1 << 16, nsteps=1), _s("ssfm", 10125), _s("ssfm", 6000),
              _s("manakovSSF", 1 << 14, "complex64"), _s("manakovSSF", 1 << 14, "complex64", packed=0, tag="-unpacked"),
              _s("manakovSSF", 9000, "complex64"), _s("manakovSSF", 48000, "complex64", nsteps=1), _s("ssfm", 1 << 14, "complex64")]
STRONG_GPU = STRONG_EMU + [_s("manakovSSF", 1 << 20, nsteps=1), _s("manakovSSF", 200000, nsteps=1), _s("manakovSSF", 3000),
                           _s("manakovSSF", 97), _s("manakovSSF", 10007), _s("manakovSSF", 1 << 16, "complex64"),
                           _s("manakovSSF", 1 << 22, "complex64")]


@pytest.mark.parametrize("c", STRONG_EMU, ids=_case_id)
def test_strong_field_with_dispersion_on_the_emulated_kernels(c, monkeypatch):
    E, cfg, *_ = _cached(("strong", _case_id(c)), lambda: _strong_reference(c))
    out, info = _emu_run(c, E, cfg, monkeypatch)
    _check_strong(c, "emu", out, info)


def test_a_strong_step_moves_the_phase_by_more_than_a_quarter_turn_between_iterates():
    """sin_half_angle's large branch needs |theta_1 - theta_0| > pi/2 on some samples: the first two iterates of the first
    step of the wide-band case (STRONG_EMU: WIDE; its complex64 twin is what reaches the packed kernel's fallback for
    |dtheta| > 1.5), rebuilt from the oracle's public pieces as tests/test_step_helpers.py does."""
    c = next(x for x in STRONG_EMU if x.get("tag") == "-wideband" and x["prec"] == "complex128")
    cfg, E = _strong_cfg(c), _strong_field(c)
    hz = cfg["hz"]
    half = make_param(orc.parameters, dict(L=hz / 2, alpha=cfg["alpha"], D=cfg["D"], Fc=cfg["Fc"], Fs=cfg["Fs"]))
    Ex, Ey = E[:, 0], E[:, 1]
    Pch = Ex * np.conj(Ex) + Ey * np.conj(Ey)
    th0 = orc.nlinPhaseRot(Ex, Ey, Pch, GAMMA) * hz
    Efd = orc.linearFiberChannel(orc.linearFiberChannel(E, half) * np.exp(1j * th0)[:, None], half)
    th1 = orc.nlinPhaseRot(Efd[:, 0], Efd[:, 1], Pch, GAMMA) * hz
    n_large = int(np.sum(np.abs(th1 - th0) > np.pi / 2))
    print(f"STRONG |theta_1 - theta_0| > pi/2 on {n_large} of {len(E)} samples, max {np.abs(th1 - th0).max():.2f} rad")
    assert n_large >= 100 and th0.max() > QUARTER


# ------------------------------------------------------------------------------------------ 3. the reference's 2 W set-ups, first steps
REF_2W = [(name, n) for name in ("ssfm_ref_spm", "ssfm_ref_power") for n in (2, 4)]


def _ref_2w(name, nsteps):
    d, cfg = load_golden(name)
    cfg = dict(cfg, Ltotal=nsteps * cfg["hz"], Lspan=nsteps * cfg["hz"], saveSpanN=[])
    E = d["Ei"]
    assert GAMMA * np.max(np.abs(E) ** 2) * cfg["hz"] > QUARTER and cfg["gamma"] == GAMMA
    gate = parity_gate("ssfm", E, cfg, TOL_C128)
    assert gate is not None                                       # comparable: the chaos is in the 80 steps, not in the first few
    return E, cfg, orc.ssfm(E, make_param(orc.parameters, cfg)), gate


@pytest.mark.parametrize("name,nsteps", REF_2W)
def test_reference_2w_setups_first_steps_on_the_emulated_kernels(name, nsteps):
    E, cfg, ref, gate = _cached(("2w", name, nsteps), lambda: _ref_2w(name, nsteps))
    out, info = eb.run("ssfm", E, cfg)
    d = rel_l2(out[0], ref)
    print(f"STRONG 2W {name} {nsteps} steps emu: gate {gate:.3e}, emu-to-oracle {d:.3e}")
    assert info["steps"] == nsteps and d <= gate


# ------------------------------------------------------------------------------------------ 4. the families of the table
def test_the_lengths_take_the_stage_families_of_the_table():
    """The splits behind the docstring's table, from the engine's own functions (the emulator links the same headers)."""
    import ctypes as C
    e = eb.load()
    e.emu_mixed2_split.argtypes = [C.c_int64, C.c_int] + [C.POINTER(C.c_int)] * 3

    def mix2(N, prec=1):
        n1, n2, cc = C.c_int(0), C.c_int(0), C.c_int(0)
        return (n1.value, n2.value) if e.emu_mixed2_split(N, prec, C.byref(n1), C.byref(n2), C.byref(cc)) else None

    def split(N, prec=1):
        l1, l2 = C.c_int(0), C.c_int(0)
        assert e.emu_split(N, prec, C.byref(l1), C.byref(l2)) == 0
        return l1.value, l2.value
    assert split(1 << 12) == (6, 6) and split(1 << 16) == (8, 8) and split(1 << 20) == (8, 12) and split(1 << 14, 0) == (7, 7)
    assert mix2(48000) is None and e.emu_supported(48000, 1) and mix2(48000, 0) is None          # 2^7 columns x 375: k_col_ragged
    assert mix2(9000) == (120, 75) and mix2(200000) == (125, 1600) and mix2(9000, 0) is not None
    assert mix2(6000) == (80, 75) and mix2(10125) is not None
    for N in (3000, 97, 10007):                                                                  # the general engine's lengths
        assert not e.emu_supported(N, 1)


# ------------------------------------------------------------------------------------------ GPU: the public API, both engines
ENGINES = ["fused", "rocfft"]
PIPELINE = {3000: "fused-rows", 97: "fused-bluestein", 10007: "fused-bluestein"}


def _with_engines(cases):
    """(case, engine) pairs, the engines of a case next to each other; SSF_C64_PACKED selects among the fused engine's kernels only."""
    return [(c, e) for c in cases for e in ENGINES if not (e == "rocfft" and "packed" in c)]


def _pair_id(v):
    return _case_id(v) if isinstance(v, dict) else str(v)


def _gpu_run(c, E, cfg, engine, monkeypatch):
    import opticommpy_amd as oa
    from opticommpy_amd import models
    assert models.engine_supported(engine, c["N"], 1 if c["func"] == "ssfm" else E.shape[1], np.dtype(c["prec"]).type)
    if "packed" in c:                                             # read when the plan is created
        models.release_plans()
        monkeypatch.setenv("SSF_C64_PACKED", str(c["packed"]))
    oa.set_engine(engine)
    try:
        out = {"ssfm": oa.ssfm, "manakovSSF": oa.manakovSSF, "manakovDBP": oa.manakovDBP}[c["func"]](
            E, make_param(oa.parameters, cfg), _trace=True)
        run = dict(models.last_run)
    finally:
        if "packed" in c:
            models.release_plans()
    if engine == "fused":
        assert run["engine"] == "fused" and run["pipeline"] == PIPELINE.get(c["N"], "fused-device")
    assert out.dtype == np.dtype(c["prec"]) and out.shape == E.shape
    return out, run


@pytest.mark.gpu
@pytest.mark.parametrize("c,engine", _with_engines(CLOSED_GPU), ids=_pair_id)
def test_closed_form_rotation_on_the_gpu(c, engine, monkeypatch):
    E, _, cfg, *_ = _cached(("closed", _case_id(c)), lambda: _closed_reference(c))
    out, run = _gpu_run(c, E, cfg, engine, monkeypatch)
    _check_closed(c, engine, out, run.get("iters", []), run.get("lims", []))


@pytest.mark.gpu
@pytest.mark.parametrize("c,engine", _with_engines(STRONG_GPU), ids=_pair_id)
def test_strong_field_with_dispersion_on_the_gpu(c, engine, monkeypatch):
    E, cfg, *_ = _cached(("strong", _case_id(c)), lambda: _strong_reference(c))
    out, run = _gpu_run(c, E, cfg, engine, monkeypatch)
    _check_strong(c, engine, out, run)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name,nsteps", REF_2W)
def test_reference_2w_setups_first_steps_on_the_gpu(name, nsteps, engine):
    import opticommpy_amd as oa
    from opticommpy_amd import models
    E, cfg, ref, gate = _cached(("2w", name, nsteps), lambda: _ref_2w(name, nsteps))
    oa.set_engine(engine)
    out = oa.ssfm(E, make_param(oa.parameters, cfg), _trace=True)
    d = rel_l2(out, ref)
    print(f"STRONG 2W {name} {nsteps} steps {engine}: gate {gate:.3e}, {engine}-to-oracle {d:.3e}")
    assert models.last_run["engine"] == engine and models.last_run["steps"] == nsteps and d <= gate
