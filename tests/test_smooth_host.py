"""Host-side checks of the sample-domain smoothers and of the energy and ZCR groups: afx_savgol_tables against
scipy.signal.savgol_coeffs, the three host executors (the kernels' operations in the kernels' order, on the CPU) against
scipy / numpy through the restatement tests/smooth_ref.py on the case lists of the GPU tests, the argument refusals, the
symbols, the stand-alone sanitizer program, and the Python dict builders.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.signal

from tests import smooth_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audio_feature_extraction_amd", "csrc")
NAMES_HOST = ("afx_smooth_geometry", "afx_savgol_tables", "afx_medfilt_host", "afx_savgol_host", "afx_energy_zcr_host")
NAMES_DEVICE = ("afx_medfilt_batch", "afx_savgol_batch", "afx_energy_zcr_batch")


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    return _native


def test_symbols_are_declared_bound_and_stubbed(N):
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    for name in NAMES_HOST + NAMES_DEVICE:
        assert name in N.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(N.lib(), name)
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)                  # found by their presence
    stubs = open(os.path.join(CSRC, "afx_host_stubs.cpp")).read()
    for name in NAMES_DEVICE:
        assert re.search(r"\bint\s+" + name + r"\s*\(", stubs), name
    for name in NAMES_HOST:                                                     # real in the host build
        assert not re.search(r"\bint\s+" + name + r"\s*\(", stubs), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    asan_srcs = re.search(r"^ASAN_SRCS := (.*)$", mk, re.M).group(1)
    assert "afx_smooth_host.cpp" in asan_srcs and "afx_smooth.hip" not in asan_srcs
    assert "afx_smooth.o" in mk and "afx_smooth_host.o" in mk and "smooth-check:" in mk
    for i, f in enumerate(N.EZ_FIELDS):                                         # the record's slots as the header names them
        enum = {"T": "T", "fl": "FL", "hop": "HOP", "zcr_local_stability": "ZCR_LOCAL"}.get(f, f.upper())
        assert re.search(r"\bAFX_EZ_%s = %d\b" % (enum, i), header), f
    assert re.search(r"\bAFX_EZ_N = %d\b" % N.EZ_N, header) and len(N.EZ_FIELDS) == N.EZ_N and N.EZ_FIELDS == S.REC_FIELDS
    assert (N.EZ_PREPROCESS, N.EZ_ENERGY, N.EZ_ZCR) == (1, 2, 4)
    assert re.search(r"AFX_EZ_PREPROCESS = 1, AFX_EZ_ENERGY = 2, AFX_EZ_ZCR = 4", header)


def test_geometry_and_case_lists(N):
    g = N.smooth_geometry()
    assert g["tile"] >= 64 and g["max_window"] == 31 and g["max_polyorder"] == 5 and g["max_deriv"] == 2
    assert max(S.MED_KERNELS) == g["max_window"] and max(w for w, _, _ in S.SAVGOL_CASES) == g["max_window"]
    for K in S.MED_KERNELS:
        ns = S.med_lengths(K, g["tile"])
        assert {1, 2, K, g["tile"] - 1, g["tile"], g["tile"] + 1, g["tile"] + K // 2, 2 * g["tile"] + 1, 3 * g["tile"] + 17} <= set(ns)
    for W, P, d in S.SAVGOL_CASES:
        ns = S.savgol_lengths(W, g["tile"])
        assert min(ns) == W and {W + 1, 2 * W - 1, g["tile"], 3 * g["tile"] + 17} <= set(ns)
    from audio_feature_extraction_amd import filters
    assert (filters.MAX_WINDOW, filters.MAX_POLYORDER, filters.MAX_DERIV) == (g["max_window"], g["max_polyorder"], g["max_deriv"])


def test_savgol_tables_match_scipy(N):
    """the interior taps against scipy.signal.savgol_coeffs to 1e-12 absolute at every window, order and derivative; the
    edge rows against the centred pseudo-inverse through numpy"""
    worst = worst_edge = 0.0
    for W in range(3, 32, 2):
        for P in range(0, min(6, W)):
            for d in range(3):
                t = N.savgol_tables(W, P, d)
                ref = scipy.signal.savgol_coeffs(W, P, deriv=d)
                worst = max(worst, float(np.max(np.abs(t["coeffs"] - ref))))
                h = W // 2
                worst_edge = max(worst_edge, float(np.max(np.abs(t["left"] - S._centred_rows(W, P, d, 1.0, range(h))))),
                                 float(np.max(np.abs(t["right"] - S._centred_rows(W, P, d, 1.0, range(h + 1, W))))))
    print(f"largest |coeffs - scipy| {worst:.2e}, largest |edge rows - numpy pinv| {worst_edge:.2e}")
    assert worst <= 1e-12 and worst_edge <= 1e-10
    t = N.savgol_tables(9, 2, 1, 0.25)
    np.testing.assert_allclose(t["coeffs"], scipy.signal.savgol_coeffs(9, 2, deriv=1, delta=0.25), rtol=0, atol=1e-11)
    assert not N.savgol_tables(5, 1, 2)["coeffs"].any()                        # deriv above the order: scipy's zeros


def test_refusals(N):
    x = np.ones(40, np.float32)
    for W, P, d, delta in ((33, 3, 0, 1.0), (10, 3, 0, 1.0), (1, 0, 0, 1.0), (11, 6, 0, 1.0), (11, 3, 3, 1.0)):
        with pytest.raises(NotImplementedError):
            N.savgol_tables(W, P, d, delta)
        with pytest.raises(NotImplementedError):
            N.savgol_host(x, W, P, d, delta)
    for W, P, d, delta in ((5, 5, 0, 1.0), (0, 0, 0, 1.0), (-3, 0, 0, 1.0), (11, -1, 0, 1.0), (11, 3, -1, 1.0), (11, 3, 0, 0.0),
                           (11, 3, 0, float("nan")), (11, 3, 0, float("inf"))):
        with pytest.raises(ValueError):
            N.savgol_tables(W, P, d, delta)
        with pytest.raises(ValueError):
            N.savgol_host(x, W, P, d, delta)
    for K in (0, -1, 2, 4):
        with pytest.raises(ValueError):
            N.medfilt_host(x, K)
    with pytest.raises(NotImplementedError):
        N.medfilt_host(x, 33)
    with pytest.raises(ValueError):
        N.medfilt_host(np.ones(4, np.float64), 3)
    for fl, hop, flags in ((1000, 512, 6), (32, 8, 6), (4096, 512, 6), (2048, 0, 6), (2048, 512, 8)):
        with pytest.raises(ValueError):
            N.energy_zcr_host(x, fl, hop, flags)


def test_python_argument_checks():
    """every refusal comes before a device is touched"""
    from audio_feature_extraction_amd import filters, AudioFeatureExtractor
    x = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="Each element of kernel_size should be odd"):
        filters.medfilt(x, 4)
    with pytest.raises(ValueError):
        filters.medfilt(x, 0)
    with pytest.raises(NotImplementedError):
        filters.medfilt(x, 33)
    with pytest.raises(ValueError, match="1-D"):
        filters.medfilt(np.zeros((2, 50), np.float32), 3)
    with pytest.raises(ValueError, match="1-D"):
        filters.medfilt_batch([x, np.zeros((2, 50), np.float32)], 3)
    with pytest.raises(ValueError, match="polyorder must be less than window_length"):
        filters.savgol_filter(x, 5, 5)
    with pytest.raises(ValueError, match="window_length must be less than or equal to the size of x"):
        filters.savgol_filter(x[:10], 11, 3)
    with pytest.raises(ValueError, match="mode must be"):
        filters.savgol_filter(x, 11, 3, mode="reflect")
    for mode in ("mirror", "constant", "nearest", "wrap"):
        with pytest.raises(NotImplementedError):
            filters.savgol_filter(x, 11, 3, mode=mode)
    for W, P, d in ((10, 3, 0), (33, 3, 0), (1, 0, 0), (11, 6, 0), (11, 3, 3)):
        with pytest.raises(NotImplementedError):
            filters.savgol_filter(x, W, P, deriv=d)
        with pytest.raises(NotImplementedError):
            filters.savgol_filter_batch([x], W, P, deriv=d)
    for kw in (dict(window_length=0, polyorder=0), dict(window_length=11, polyorder=-1), dict(window_length=11, polyorder=3, deriv=-1),
               dict(window_length=11, polyorder=3, delta=0.0), dict(window_length=11.5, polyorder=3)):
        with pytest.raises(ValueError):
            filters.savgol_filter(x, **kw)
    with pytest.raises(ValueError, match="1-D"):
        filters.savgol_filter(np.zeros((2, 50), np.float32), 11, 3)
    assert filters.medfilt_batch([], 3) == [] and filters.savgol_filter_batch([], 11, 3) == []
    assert filters.medfilt(np.zeros(0, np.float32), 3).size == 0
    ex = AudioFeatureExtractor(sr=22050, device=0)
    assert ex.extract_energy_zcr_features_batch([]) == []
    with pytest.raises(ValueError, match="1-D"):
        ex.extract_energy_zcr_features_batch([np.zeros((2, 50), np.float32)])
    with pytest.raises(ValueError, match="power of two"):
        ex.extract_energy_zcr_features_batch([x], frame_length=1000)
    with pytest.raises(ValueError):
        ex.extract_energy_zcr_features_batch([x], hop_length=0)
    assert callable(ex.extract_energy_features) and callable(ex.extract_zcr_features)


@pytest.mark.parametrize("K", S.MED_KERNELS + (7,))
def test_medfilt_host_equals_scipy(N, K):
    tile = N.smooth_geometry()["tile"]
    for k, n in enumerate(S.med_lengths(K, tile)):
        x = S.signal(n, 1000 * K + k)
        r = N.medfilt_host(x, K)
        assert r["status"] == N.CLIP_OK and r["out"].dtype == np.float32
        np.testing.assert_array_equal(r["out"], S.medfilt_ref(x, K), err_msg=f"K {K} n {n}")
        assert not np.signbit(r["out"][r["out"] == 0]).any()
        q = S.to_s16(x)
        np.testing.assert_array_equal(N.medfilt_host(q, K)["out"], N.medfilt_host(q.astype(np.float32) / np.float32(32768.0), K)["out"])


def test_medfilt_host_statuses_and_the_documented_values(N):
    np.testing.assert_array_equal(N.medfilt_host(np.array([3, 1, 2, 5, 4, -0., 0., 7], np.float32), 3)["out"],
                                  np.array([1, 2, 2, 4, 4, 0, 0, 0], np.float32))
    np.testing.assert_array_equal(N.medfilt_host(np.array([1, 2], np.float32), 5)["out"], np.zeros(2, np.float32))
    assert N.medfilt_host(np.zeros(0, np.float32), 3)["status"] == N.CLIP_TOO_SHORT
    bad = S.signal(300, 1)
    for v in (np.nan, np.inf, -np.inf):
        bad[299] = v
        r = N.medfilt_host(bad, 5)
        assert r["status"] == N.CLIP_NONFINITE and not r["out"].any()
    z = N.medfilt_host(np.zeros(100, np.float32), 25)
    assert z["status"] == N.CLIP_OK and not z["out"].any()


@pytest.mark.parametrize("W,P,d", S.SAVGOL_CASES)
def test_savgol_host_matches_scipy(N, W, P, d):
    """every length of the case, noise and the quadratic ramp; the largest ratio to the bound is printed"""
    tile = N.smooth_geometry()["tile"]
    worst = cond = 0.0
    for k, n in enumerate(S.savgol_lengths(W, tile)):
        for x in (S.signal(n, 5000 + 100 * W + k), S.quadratic(n)):
            r = N.savgol_host(x, W, P, d)
            assert r["status"] == N.CLIP_OK and r["out"].dtype == np.float32
            ratio, c = S.savgol_ratio(r["out"], x, W, P, d)
            assert ratio <= 1.0, (W, P, d, n, ratio, c)
            worst, cond = max(worst, ratio), max(cond, c)
    print(f"savgol ({W}, {P}, deriv {d}): largest ratio to the bound {worst:.3f}, largest conditioning {cond:.2e}")
    if P >= 2 and d == 0:                                   # the ramp comes back, edges included
        x = S.quadratic(3 * tile + 17)
        assert np.max(np.abs(N.savgol_host(x, W, P, 0)["out"].astype(np.float64) - x)) <= 2.0 ** -23 * np.max(np.abs(x))
    assert N.savgol_host(S.signal(W - 1, 3), W, P, d)["status"] == N.CLIP_TOO_SHORT
    bad = S.signal(2 * W, 4)
    bad[0] = np.nan
    assert N.savgol_host(bad, W, P, d)["status"] == N.CLIP_NONFINITE
    q = S.to_s16(S.signal(3 * W, 6))
    np.testing.assert_array_equal(N.savgol_host(q, W, P, d)["out"], N.savgol_host(q.astype(np.float32) / np.float32(32768.0), W, P, d)["out"])
    x = S.signal(4 * W, 8)
    ratio, _ = S.savgol_ratio(N.savgol_host(x, W, P, d, 0.25)["out"], x, W, P, d, 0.25)
    assert ratio <= 1.0


def _preprocessed(N, n, sr, seed):
    from tests import filt_ref as F
    r = N.sosfiltfilt_host(S.group_signal(n, sr, seed), N.butter_sos(5, 200 / (sr / 2), True), F.PADLEN, N.FILT_EXPERIMENT, F.COEF)
    assert r["status"] == N.CLIP_OK
    return r["out"]


@pytest.mark.parametrize("sr", S.GROUP_RATES)
def test_group_host_executor_matches_the_restatement(N, sr):
    from audio_feature_extraction_amd import AudioFeatureExtractor as A
    outside = {}
    cases = [(n, _preprocessed(N, n, sr, 300 + k)) for k, n in enumerate(S.GROUP_LENGTHS_PRE)]
    cases += [(n, S.group_signal(n, sr, 400 + k)) for k, n in enumerate(S.GROUP_LENGTHS_RAW)]
    for n, y in cases:
        ref = S.group_record(y)
        r = N.energy_zcr_host(y, S.FRAME_LENGTH, S.HOP_LENGTH)
        assert r["status"] == N.CLIP_OK
        S.check_record(r["rec"], ref, (sr, n))
        assert np.isnan(r["rec"][10:]).all()
        # a group alone equals its slice of the full record, the other group's fields NaN
        e = N.energy_zcr_host(y, S.FRAME_LENGTH, S.HOP_LENGTH, N.EZ_ENERGY)["rec"]
        z = N.energy_zcr_host(y, S.FRAME_LENGTH, S.HOP_LENGTH, N.EZ_ZCR)["rec"]
        np.testing.assert_array_equal(e[:6], r["rec"][:6])
        np.testing.assert_array_equal(z[[0, 1, 2, 6, 7, 8, 9]], r["rec"][[0, 1, 2, 6, 7, 8, 9]])
        assert np.isnan(e[6:]).all() and np.isnan(z[3:6]).all()
        # the dicts: flags and scores where the scalar behind them is clear of its threshold
        got = {**A._energy_dict(r["rec"]), **A._zcr_dict(r["rec"])}
        want = {**S.energy_dict(ref), **S.zcr_dict(ref)}
        assert list(got) == list(A._ENERGY_KEYS + A._ZCR_KEYS)
        for k, clear in S.flag_margins(want).items():
            outside[k] = outside.get(k, 0) + (0 if clear else 1)
            if clear:
                assert got[k] == want[k], (sr, n, k)
        for k in ("energy_cv", "energy_snr", "zcr_cv"):
            assert got[k] == pytest.approx(want[k], rel=1e-9, abs=1e-12), (sr, n, k)
    assert max(outside.values()) * 10 <= len(cases), outside


def test_group_framing_switches(N):
    """T = 9, 10, 11 around the window of the local stability; the n > 11 guard; the adjusted frame lengths"""
    f = N.EZ_FIELDS.index
    for n, (fl, hop, T) in ((5, (64, 16, 1)), (11, (64, 16, 1)), (12, (64, 16, 1)), (63, (64, 16, 4)), (64, (64, 16, 5)),
                            (65, (64, 16, 5)), (2047, (1024, 256, 8)), (2048, (2048, 512, 5)), (9 * 512 - 1, (2048, 512, 9)),
                            (9 * 512, (2048, 512, 10)), (10 * 512, (2048, 512, 11))):
        assert S.framing(n) == (fl, hop, T)
        r = N.energy_zcr_host(S.group_signal(n, 22050, n), S.FRAME_LENGTH, S.HOP_LENGTH)["rec"]
        assert (r[f("fl")], r[f("hop")], r[f("T")]) == (fl, hop, T)
    y = S.signal(12, 9)
    s11, s12 = S.smoothed(y[:11]), S.smoothed(y)
    np.testing.assert_array_equal(s11, S.medfilt_ref(y[:11], 3).astype(np.float32))          # the guard is strict
    assert not np.array_equal(s12, S.medfilt_ref(y, 3).astype(np.float32))
    assert N.energy_zcr_host(y[:11])["rec"][f("peak_smooth")] == np.max(np.abs(s11))
    assert N.energy_zcr_host(y)["rec"][f("peak_smooth")] == pytest.approx(np.max(np.abs(s12)), rel=2.0 ** -23)
    z = N.energy_zcr_host(np.zeros(5000, np.float32))
    assert z["status"] == N.CLIP_OK and not z["rec"][3:10].any()                            # a zero peak: the signal as it is
    assert N.energy_zcr_host(np.zeros(0, np.float32))["status"] == N.CLIP_TOO_SHORT
    bad = S.signal(300, 2)
    bad[17] = np.inf
    r = N.energy_zcr_host(bad)
    assert r["status"] == N.CLIP_NONFINITE and np.isnan(r["rec"]).all()


def test_dict_builders_on_hand_made_records(N):
    from audio_feature_extraction_amd import AudioFeatureExtractor as A
    rec = np.full(N.EZ_N, np.nan)
    f = N.EZ_FIELDS.index
    rec[f("energy_mean")], rec[f("energy_std")], rec[f("energy_p10")] = 0.1, 0.02, 0.005
    rec[f("zcr_mean")], rec[f("zcr_std")], rec[f("zcr_local_stability")] = 0.2, 0.1, 0.05
    e, z = A._energy_dict(rec), A._zcr_dict(rec)
    assert e == {"energy_mean": 0.1, "energy_std": 0.02, "energy_cv": pytest.approx(0.2), "energy_snr": pytest.approx(20 * np.log10(20.0)),
                 "energy_range_valid": True, "energy_stability": True, "energy_snr_valid": True, "energy_quality_score": 1.0}
    assert z == {"zcr_mean": 0.2, "zcr_std": 0.1, "zcr_cv": pytest.approx(0.5), "zcr_local_stability": 0.05, "zcr_range_valid": True,
                 "zcr_stability": False, "zcr_local_stable": True, "zcr_quality_score": pytest.approx(0.7)}
    assert all(type(v) in (float, bool, int) for v in list(e.values()) + list(z.values()))
    rec[f("energy_mean")], rec[f("energy_std")], rec[f("energy_p10")] = 0.0, 0.0, 0.0     # silence: cv inf, snr 0
    e = A._energy_dict(rec)
    assert e["energy_cv"] == float("inf") and e["energy_snr"] == 0 and e["energy_quality_score"] == pytest.approx(0.1)
    assert not (e["energy_range_valid"] or e["energy_stability"] or e["energy_snr_valid"])
    rec[f("zcr_mean")], rec[f("zcr_std")], rec[f("zcr_local_stability")] = 0.0, 0.0, 0.2
    z = A._zcr_dict(rec)
    assert z["zcr_cv"] == float("inf") and z["zcr_quality_score"] == 0.0
    recs = np.stack([rec, rec, rec])
    out = A._energy_zcr_dicts(N.EZ_ENERGY | N.EZ_ZCR, recs, np.array([N.CLIP_OK, N.CLIP_TOO_SHORT, N.CLIP_NONFINITE]))
    assert out[1] is None and out[2] is None and list(out[0]) == list(A._ENERGY_KEYS + A._ZCR_KEYS)
    assert list(A._energy_zcr_dicts(N.EZ_ZCR, recs[:1], np.array([N.CLIP_OK]))[0]) == list(A._ZCR_KEYS)


def test_smooth_check_program_is_clean():
    """the host executors and the tables under AddressSanitizer + UBSan: a stand-alone program, nothing preloaded"""
    r = subprocess.run(["make", "-C", CSRC, "smooth-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "smooth_check: ok" in r.stdout
