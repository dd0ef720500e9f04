"""tests/clock_restatement.py held to the reference's fixtures (tests/golden/clock/*.npz): the converters' numpy statements give
the recorded results bit for bit; the clock recovery's definition gives the reference's shapes and gap pattern, lies within the
distances the generator recorded, and keeps its margin | |t_nco| - 1 | at 10 times the timing distance and more."""
import numpy as np
import pytest

import clock_cases as cc
import clock_restatement as rs

ISSUE_CASES = dict(
    interp=["adc_ratio_c128", "double_c64", "jitter_c128", "jitter_c64", "jitter_f32", "jitter_f64", "third_f32", "unity_f64"],
    quant=["b1", "b16", "b2", "b8"],
    conv=["adc_complex_filters", "adc_complex_nofilter", "adc_complex_nofilter_double", "adc_defaults", "adc_jitter_enob", "adc_real_filters",
          "adc_real_nofilter", "dac_complex_filters", "dac_complex_nofilter", "dac_real_filters", "dac_real_nofilter", "notebook_pair",
          "resample_down", "resample_up_1d"],
    gardner=["m300_nyq_c64_1d", "m300_ted_c128_1d", "p300_nyq_c128", "p300_ted_c64", "two_modes_c64", "zero_nyq_c128"])


def test_every_case_of_the_issue_has_a_fixture():
    assert dict(interp=cc.INTERP, quant=cc.QUANT, conv=cc.CONV, gardner=cc.GARDNER) == ISSUE_CASES
    for family, cases in ISSUE_CASES.items():
        for name in cases:
            cc.check_conditions(family, cc.load(family, name))
    assert set(cc.FILTERS) <= set(cc.CONV)


def test_fixtures_pin_what_the_issue_names():
    ratios = sorted(cc.load("interp", n)["cfg"]["ratio"] for n in cc.INTERP if not cc.load("interp", n)["cfg"]["jitter"])
    assert ratios == [1 / 3, 0.5 * (1 + 105e-6), 1.0, 2.0]
    assert {cc.load("interp", n)["x"].dtype.name for n in cc.INTERP if cc.load("interp", n)["cfg"]["jitter"]} == set(cc.clock._DTYPES)
    assert [cc.load("quant", n)["cfg"]["nBits"] for n in ("b1", "b2", "b8", "b16")] == [1, 2, 8, 16]
    g = {n: cc.load("gardner", n)["cfg"] for n in cc.GARDNER}
    assert {c["ppm"] for c in g.values()} == {300, -300, 0}
    assert {c["p"]["isNyquist"] for c in g.values()} == {True, False} and {c["p"]["lpad"] for c in g.values()} >= {0, 7}
    assert {c["p"]["maxPPM"] for c in g.values()} == {0, 500} and {c["one_d"] for c in g.values()} == {True, False}
    assert {cc.load("gardner", n)["x"].dtype.name for n in cc.GARDNER} == {"complex128", "complex64"}
    j = cc.load("conv", "adc_jitter_enob")["cfg"]["p"]
    assert j["jitter"] > 0 and j["ENOB"] < j["nBits"]
    # the recorded distances between the reference and the restatement (tests/clock_cases.py quotes the largest)
    assert max(float(cc.load("gardner", n)["dist_sig"]) for n in cc.GARDNER) <= 19
    assert max(float(cc.load("gardner", n)["dist_t"]) for n in cc.GARDNER) <= 2.7e-6


@pytest.mark.parametrize("name", cc.INTERP)
def test_interpolation_is_numpys(name):
    g = cc.load("interp", name)
    c = g["cfg"]
    np.random.seed(c["seed"])
    tout = rs.jittered(len(g["x"]), c["inFs"], c["outFs"], c["jitter_s"])
    assert np.array_equal(rs.clock_interp(g["x"], c["inFs"], c["outFs"], tout), g["y"])


@pytest.mark.parametrize("name", cc.QUANT)
def test_quantizer_is_numpys(name):
    g = cc.load("quant", name)
    c = g["cfg"]
    assert np.array_equal(rs.quantizer(g["x"], c["nBits"], c["maxV"], c["minV"]), g["y"])
    assert len(rs.quant_levels(c["nBits"], c["maxV"], c["minV"])) == c["levels"] == cc.clock.quant_table(c["nBits"], c["maxV"], c["minV"])[2]


@pytest.mark.parametrize("name", ["adc_complex_nofilter", "adc_complex_nofilter_double", "adc_real_nofilter", "adc_jitter_enob"])
def test_adc_without_filters_is_the_restated_chain(name):
    """Interpolate, clip (numpy's lexicographic clip of complex values), quantise; two jitter draws, the real parts' first; then
    the noise of ENOB < nBits from the same stream."""
    g = cc.load("conv", name)
    p, sig = g["cfg"]["written"], g["sigIn"]
    x = sig.reshape(len(sig), -1)
    np.random.seed(g["cfg"]["seed"])
    t_re = rs.jittered(len(x), p["inFs"], p["outFs"], p["jitter"])
    t_im = rs.jittered(len(x), p["inFs"], p["outFs"], p["jitter"]) if np.iscomplexobj(x) else None
    out = rs.adc_core(x, p["inFs"], p["outFs"], p["nBits"], p["Vmax"], p["Vmin"], t_re, t_im)
    if p["nBits"] > p["ENOB"]:
        out = out + cc.clock._extra_noise(out.shape, True, p["Vmax"] - p["Vmin"], p["nBits"], p["ENOB"])
    assert np.array_equal(out.flatten() if out.shape[1] == 1 else out, g["out"])
    if np.iscomplexobj(x) and name != "adc_jitter_enob":
        inside = np.abs(rs.clock_interp(np.real(x), p["inFs"], p["outFs"])) < min(abs(p["Vmin"]), abs(p["Vmax"]))
        assert np.any(inside)


@pytest.mark.parametrize("name", cc.GARDNER)
def test_clock_recovery_definition_against_the_reference(name):
    g = cc.load("gardner", name)
    want, tvw, info = cc.restated(g)
    assert want.shape == g["out"].shape and tvw.shape == g["tv"].shape and want.dtype == np.complex64
    assert cc.gap_indices(tvw) == g["cfg"]["gaps"] and info["last_n"] == g["cfg"]["last_n"]
    spacing = float(np.spacing(np.float32(np.max(np.abs(want)))))
    dist_sig = float(np.max(np.abs(want.astype(np.complex128) - g["out"].astype(np.complex128))) / spacing)
    dist_t = float(np.max(np.abs(tvw - g["tv"])))
    assert dist_sig == float(g["dist_sig"]) and dist_t == float(g["dist_t"])
    assert info["margin"] == float(g["margin"]) >= 10 * dist_t


def test_clock_drift_is_the_references():
    for name in cc.GARDNER:
        g = cc.load("gardner", name)
        assert [None if np.isnan(v) else float(v) for v in rs.clock_drift(g["tv"])] == g["cfg"]["drift"]
    assert any(v is not None for n in cc.GARDNER for v in cc.load("gardner", n)["cfg"]["drift"])


def test_local_maxima_is_scipys_rule():
    from scipy.signal import find_peaks
    rng = np.random.default_rng(3)
    for _ in range(20):
        d = np.round(rng.uniform(0, 1, size=60), 1)              # coarse values: plateaus are common
        assert rs.local_maxima(d, 0.5).tolist() == find_peaks(d, height=0.5)[0].tolist()
