"""The host side of afx_specdist_batch / afx_clip_fft_batch: their symbols, the cost record and a hand-computed cut, the
refusals, the host executors against the long-double truth of tests/spectrum_ref.py at every test length, and quality.*
through the host fallback.  CPU only."""
import os
import re

import numpy as np
import pytest

from tests import spectrum_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afx_specdist_batch", "afx_clip_fft_batch", "afx_specdist_host", "afx_clip_fft_host", "afx_specdist_cost")


def check_bins(got, p, what):
    """bins 0 .. n / 2 of a clip's DFT within bound(n) of the truth, relative L2"""
    n = p["n"]
    assert got.dtype == np.complex128 and got.shape == (n // 2 + 1,), what
    err = S.rel_l2(got, p["R"][:n // 2 + 1])
    print(f"{what:24s} n {n:7d}  rfft error {err:.2e}  bound {p['bound']:.2e}")
    assert err <= p["bound"], (what, n, err, p["bound"])


def check_record(rec, p, what):
    """one AFX_SPECDIST_N record: n exactly, the distance within the pair's tolerance, Parseval both ways to 1e-12"""
    n = p["n"]
    assert rec[0] == n, what
    err = abs(rec[1] / n - p["spec_dist"])
    print(f"{what:24s} n {n:7d}  spec_dist error {err:.2e}  allowed {p['tol']:.2e}")
    assert err <= p["tol"], (what, n, err, p["tol"])
    for k, y in ((2, p["r"]), (3, p["d"])):
        want = n * float(np.sum(y.astype(np.float64) ** 2))
        assert abs(rec[k] - want) <= 1e-12 * want, (what, n, k, rec[k], want)


def test_symbols_are_declared_bound_and_stubbed():
    from audio_feature_extraction_amd import _native as N
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    stubs = open(os.path.join(ROOT, "audio_feature_extraction_amd", "csrc", "afx_host_stubs.cpp")).read()
    for name in NEW:
        assert name in N.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(N.lib(), name)
        assert bool(re.search(r"\bint\s+" + name + r"\s*\(", stubs)) == name.endswith("_batch"), name         # the host executors and the cost are real in the host build
    assert re.search(r"#define\s+AFX_VERSION\s+107\b", header)           # found by their presence
    assert re.search(r"AFX_SPECDIST_N\s*=\s*%d\b" % N.SPECDIST_N, header) and len(N.SPECDIST_FIELDS) == N.SPECDIST_N
    assert re.search(r"#define\s+AFX_CFFT_MAX_N\s+\(1\s*<<\s*21\)", header) and N.CFFT_MAX_N == 1 << 21
    mk = open(os.path.join(ROOT, "audio_feature_extraction_amd", "csrc", "Makefile")).read()
    assert re.search(r"^ASAN_SRCS :=.*afx_cfft_host\.cpp", mk, re.M) and "spectrum-check:" in mk


def test_the_cost_record_and_one_cut_written_out():
    """128 bytes a sample for the work and the filter spectrum (16 M each, M < 4 n) plus both float32 uploads, 256 a pair:
         97: 136 x 97 + 256 = 13448      2048: 278784      2049: 278920      5: 936      4097: 557448
    At 300000 bytes: (97, 2048) = 292232 since 2049 would pass; (2049, 5) = 279856; (4097)."""
    from audio_feature_extraction_amd import _native as N
    c = N.specdist_cost()
    assert c.tolist() == [0, 0, 128 + 8, 256, 64, 2 ** 30 - 1]
    assert N.specdist_cost(N.FMT_S16)[2] == 128 + 4 and N.specdist_cost(N.FMT_F32, N.MEM_DEVICE)[2] == 128
    lengths = (97, 2048, 2049, 5, 4097)
    per = [136 * n + 256 for n in lengths]
    assert per == [13448, 278784, 278920, 936, 557448]
    assert N.stft_chunks(lengths, c, 300000).tolist() == [0, 0, 1, 1, 2]
    assert N.stft_chunks(lengths, c, 292231).tolist() == [0, 1, 2, 2, 3]        # one byte less than (97, 2048)
    assert N.stft_chunks(lengths, c, sum(per)).tolist() == [0] * 5 and N.stft_chunks(lengths, c, sum(per) - 1).tolist() == [0] * 4 + [1]
    assert N.stft_chunks((0, 97, 0), c, 1).tolist() == [-1, 0, -1]
    # the real workspace of a pair stays under the linear bound at every test length: M points of work and of filter
    # spectrum at 16 bytes, the job record (56), the record (32), two flag words (8), the staging's rounding (2 x 7 x 4)
    for n in S.LENGTHS + (6, 1025, 1 << 21):
        logm = 0
        while (1 << logm) < 2 * n - 1:
            logm += 1
        assert (1 << logm) >= 2 * n - 1 and (1 << logm) < 4 * n
        assert 2 * 16 * (1 << logm) + 2 * 56 + 32 + 8 + 56 <= 128 * n + 256, n
    with pytest.raises(ValueError):
        N.specdist_cost(7)
    with pytest.raises(ValueError):
        N.specdist_cost(N.FMT_F32, 9)


def test_refusals_need_no_device():
    from audio_feature_extraction_amd import _native as N
    from audio_feature_extraction_amd import quality as Q
    y = S.pairs()[4]["r"]
    with pytest.raises(ValueError):
        N.specdist_host(y, S.as_s16(y))                                  # mixed sample types
    with pytest.raises(ValueError):
        N.specdist_host(y.astype(np.float64), y.astype(np.float64))
    with pytest.raises(ValueError):
        N.clip_fft_host(np.zeros((2, 8), np.float32))
    L = N.lib()
    rec, st = np.zeros(N.SPECDIST_N), np.zeros(1, np.int32)
    assert L.afx_specdist_host(y.ctypes.data, y.ctypes.data, N.FMT_F32, -1, 5, rec.ctypes.data, st.ctypes.data) == -1      # negative length
    assert L.afx_clip_fft_host(y.ctypes.data, N.FMT_F32, -1, rec.ctypes.data, st.ctypes.data) == -1
    assert L.afx_specdist_host(y.ctypes.data, y.ctypes.data, N.FMT_F32, 1 << 28, 1 << 28, rec.ctypes.data, st.ctypes.data) == -5   # over the limit: nothing is read
    assert L.afx_clip_fft_host(y.ctypes.data, N.FMT_F32, 1 << 28, rec.ctypes.data, st.ctypes.data) == -5
    assert L.afx_specdist_host(y.ctypes.data, y.ctypes.data, 5, 5, 5, rec.ctypes.data, st.ctypes.data) == -1
    for f in (Q.spec_dist, Q.pesq_like):
        with pytest.raises(ValueError, match="1-D"):
            f(np.zeros((2, 100), np.float32), np.zeros((2, 100), np.float32))
        with pytest.raises(ValueError, match="mixes"):
            f(y, S.as_s16(y))
        with pytest.raises(ValueError, match="empty"):
            f(y, np.zeros(0, np.float32))
        with pytest.raises(ValueError, match="finite"):
            f(y, np.full(y.size, np.nan, np.float32))
    with pytest.raises(ValueError, match="1-D"):
        Q.clip_rfft(np.zeros((2, 100), np.float32))
    with pytest.raises(ValueError, match="finite"):
        Q.clip_rfft(np.array([0.5, np.inf, 0.25], np.float32))
    assert Q.spec_dist_batch([]) == [] and Q.pesq_like_batch([]) == [] and Q.clip_rfft_batch([]) == []


def test_host_executors_match_the_truth():
    from audio_feature_extraction_amd import _native as N
    for p in S.pairs():
        r = N.clip_fft_host(p["r"])
        assert r["status"] == N.CLIP_OK
        check_bins(r["bins"], p, "clip_fft_host")
        s = N.specdist_host(p["r"], p["d"])
        assert s["status"] == N.CLIP_OK
        check_record(s["rec"], p, "specdist_host")
        same = N.specdist_host(p["r"], p["r"].copy())["rec"]
        assert same[1] == 0 and same[2] == same[3], p["n"]              # equal sample for sample: exactly no distance
    p = S.pairs()[5]
    q = S.as_s16(p["r"])
    f = (q.astype(np.float32) / np.float32(32768.0))
    np.testing.assert_array_equal(N.clip_fft_host(q)["bins"], N.clip_fft_host(f)["bins"])      # int16 is value / 32768
    np.testing.assert_array_equal(N.specdist_host(q, S.as_s16(p["d"]))["rec"],
                                  N.specdist_host(f, S.as_s16(p["d"]).astype(np.float32) / np.float32(32768.0))["rec"])
    # lengths that differ: the shorter one counts
    short = N.specdist_host(p["r"], p["d"][:97])["rec"]
    np.testing.assert_array_equal(short, N.specdist_host(p["r"][:97], p["d"][:97])["rec"])
    e = N.specdist_host(p["r"], np.zeros(0, np.float32))
    assert e["status"] == N.CLIP_TOO_SHORT and np.isnan(e["rec"]).all()
    e = N.clip_fft_host(np.zeros(0, np.float32))
    assert e["status"] == N.CLIP_TOO_SHORT and e["bins"].size == 0
    bad = p["d"].copy()
    bad[1000] = np.inf
    e = N.specdist_host(p["r"], bad)
    assert e["status"] == N.CLIP_NONFINITE and np.isnan(e["rec"]).all()
    e = N.clip_fft_host(bad)
    assert e["status"] == N.CLIP_NONFINITE and np.isnan(e["bins"]).all()


def test_quality_through_the_host_fallback(monkeypatch):
    from audio_feature_extraction_amd import quality as Q
    from tests import assess_clips as K
    monkeypatch.setattr(Q, "_on_gpu", lambda: False)              # the host executors, whether or not a GPU is visible
    P = [p for p in S.pairs() if 2 < p["n"] <= 22050]
    got = Q.pesq_like_batch([(p["r"], p["d"]) for p in P])
    dist = Q.spec_dist_batch([(p["r"], p["d"]) for p in P])
    for p, g, d in zip(P, got, dist):
        assert list(g) == ["snr", "correlation", "spec_dist", "pesq"]
        want = S.pesq_exact(p["r"], p["d"], p["spec_dist"])
        assert g["spec_dist"] == d and abs(d - p["spec_dist"]) <= p["tol"]
        assert abs(g["pesq"] - want) <= 0.7 * p["tol"] + 1e-11, (p["n"], g["pesq"], want)    # d pesq / d spec_dist = 3.5 x 0.2
        assert abs(want - S.pesq_like(p["r"], p["d"])["pesq"]) <= 1e-5                         # numpy's float32 means
        assert 1.0 <= g["pesq"] <= 4.5
        check_bins(Q.clip_rfft(p["r"]), p, "quality.clip_rfft")
    p = P[-1]
    assert Q.pesq_like(p["r"], p["d"]) == got[-1]["pesq"] and Q.spec_dist(p["r"], p["d"]) == dist[-1]
    # lengths that differ within a pair; int16
    a = Q.pesq_like_batch([(p["r"], p["d"][:5000]), (S.as_s16(p["r"]), S.as_s16(p["d"]))])
    assert a[0] == Q.pesq_like_batch([(p["r"][:5000], p["d"][:5000])])[0]
    rf, df = S.as_s16(p["r"]) / np.float32(32768), S.as_s16(p["d"]) / np.float32(32768)
    assert abs(a[1]["pesq"] - S.pesq_exact(rf, df, S.spec_dist(rf, df))) <= 1e-9
    # the NaN cases: Python's min and max keep them
    const = np.full(3000, 0.25, np.float32)
    g = Q.pesq_like_batch([(const, p["r"][:3000])])[0]
    assert np.isnan(g["correlation"]) and np.isnan(g["pesq"]) and np.isfinite(g["spec_dist"])
    assert np.isnan(Q._pesq_from(0.5, 20.0, float("nan"))) and Q._pesq_from(1.0, 100, 0.0) == 4.5
    same = Q.pesq_like_batch([(p["r"], p["r"].copy())])[0]
    assert same == {"snr": 100, "correlation": 1.0, "spec_dist": 0.0, "pesq": 4.5}
    # evaluate_noise_reduction: the default is what it was, pesq=True adds the key in the reference's order
    sr = 22050
    n = sr
    y = (0.02 * np.random.default_rng(11).standard_normal(n)).astype(np.float32)
    y[int(0.4 * sr):] += K.tone(sr, n - int(0.4 * sr))
    outs = {"original": y, "spectral_subtraction": (y * np.float32(0.9)), "wiener_filter": np.roll(y, 1) * np.float32(0.8)}
    from audio_feature_extraction_amd import effects
    monkeypatch.setattr(effects, "spectral_subtraction", lambda x, sr, device=0: outs["spectral_subtraction"])
    monkeypatch.setattr(effects, "wiener_filter", lambda x, sr, device=0: outs["wiener_filter"])
    two = Q.evaluate_noise_reduction(y, sr)
    three = Q.evaluate_noise_reduction(y, sr, pesq=True)
    assert list(two) == list(three) == ["original", "spectral_subtraction", "wiener_filter"]
    for k in two:
        assert list(two[k]) == ["snr", "stoi"] and list(three[k]) == ["snr", "pesq", "stoi"]
        assert three[k]["snr"] == two[k]["snr"] and three[k]["stoi"] == two[k]["stoi"]
        want = S.pesq_exact(y, outs[k], S.spec_dist(y, outs[k]))
        assert abs(three[k]["pesq"] - want) <= 1e-9, (k, three[k]["pesq"], want)
    assert three["original"]["pesq"] == 4.5
