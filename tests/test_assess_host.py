"""The host side of afx_assess_batch / afx_compare_batch: their symbols, the cost record and a hand-computed cut, the
argument refusals, the host executors against tests/assess_ref.py on the clips of the GPU test, and quality.* through the
host fallback.  CPU only."""
import os
import re

import numpy as np
import pytest

from tests import assess_clips as K
from tests import assess_ref as R
from tests import wavfiles as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("afx_assess_batch", "afx_compare_batch", "afx_assess_host", "afx_compare_host", "afx_assess_cost")
RTOL = 1e-5                                       # the project's RMS tolerance (tests/parity.py)
FILE_KEYS = ["file_path", "file_name", "sample_rate", "bit_depth", "channels", "duration", "silence_ratio", "max_silence_duration",
             "rms_dbfs", "peak_dbfs", "rms_cv", "snr", "format_ok", "silence_ok", "volume_ok", "stability_ok", "snr_ok", "assessment_ok"]


def check_record(got, y, fs, fl, what, threshold_db=-40.0):
    """One AFX_ASSESS_N record against the float64 truth: counts and the peak exactly, the mean squares and RMS values within
    RTOL, the deviation within RTOL of the mean RMS."""
    ref = R.record(y, fs, fl, threshold_db)
    for k in (0, 1, 2, 5, 7):
        assert got[k] == ref[k], (what, R.RECORD[k], got[k], ref[k])
    for k in (3, 4, 8):
        assert abs(got[k] - ref[k]) <= RTOL * abs(ref[k]), (what, R.RECORD[k], got[k], ref[k])
    assert (np.isnan(got[6]) and np.isnan(ref[6])) or abs(got[6] - ref[6]) <= RTOL * abs(ref[6]), (what, got[6], ref[6])
    assert abs(got[9] - ref[9]) <= RTOL * ref[8], (what, got[9], ref[9])


def check_keys(got, y, sr, what, threshold_db=-40.0):
    """quality.assess's dict against the restatement: the reference's keys in its order, decisions and counts exactly, the
    derived dB / ratio values at the relative level of the sums they come from; ``snr`` where it is well conditioned."""
    ref = R.assess(y, sr, threshold_db)
    assert list(got) == list(ref) == ["silence_ratio", "max_silence_duration", "silence_ok", "rms_dbfs", "peak_dbfs", "volume_ok",
                                      "rms_std", "rms_cv", "stability_ok", "snr", "snr_ok"], what
    for k in ("silence_ratio", "max_silence_duration", "silence_ok", "peak_dbfs", "volume_ok", "stability_ok"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ("rms_dbfs", "rms_cv"):
        assert abs(got[k] - ref[k]) <= RTOL * abs(ref[k]), (what, k, got[k], ref[k])
    mean = ref["rms_std"] / ref["rms_cv"] if ref["rms_cv"] else 0.0
    assert abs(got["rms_std"] - ref["rms_std"]) <= RTOL * mean, (what, got["rms_std"], ref["rms_std"])
    if R.snr_is_robust(y):
        assert abs(got["snr"] - ref["snr"]) <= RTOL * abs(ref["snr"]) and got["snr_ok"] == ref["snr_ok"], (what, got["snr"], ref["snr"])


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
    assert re.search(r"AFX_ASSESS_N\s*=\s*%d\b" % N.ASSESS_N, header) and re.search(r"AFX_COMPARE_N\s*=\s*%d\b" % N.COMPARE_N, header)
    assert len(N.ASSESS_FIELDS) == N.ASSESS_N and tuple(N.ASSESS_FIELDS) == R.RECORD and len(N.COMPARE_FIELDS) == N.COMPARE_N
    mk = open(os.path.join(ROOT, "audio_feature_extraction_amd", "csrc", "Makefile")).read()
    assert re.search(r"^ASAN_SRCS :=.*afx_assess_host\.cpp", mk, re.M) and "assess-check:" in mk
    import audio_feature_extraction_amd as pkg
    import audio_feature_extraction_toolkit as alias
    assert alias.quality is pkg.quality and "quality" not in pkg.__all__


def test_the_cost_record_and_one_cut_written_out():
    """17 bytes a sample for the pieces and span records at frame length 1 plus the float32 upload, 256 a clip:
         5000: 21 x 5000 + 256 = 105256      12345: 259501      700: 14956      9000: 189256      3000: 63256      7000: 147256
    At 280000 bytes: (5000) since 105256 + 259501 is over; (12345, 700) = 274457; (9000, 3000) = 252512; (7000)."""
    from audio_feature_extraction_amd import _native as N
    c = N.assess_cost()
    assert c.tolist() == [0, 0, 17 + 4, 256, 64, 2 ** 30 - 1]
    assert N.assess_cost(N.COST_ASSESS, N.FMT_S16)[2] == 17 + 2 and N.assess_cost(N.COST_ASSESS, N.FMT_F32, N.MEM_DEVICE)[2] == 17
    assert N.assess_cost(N.COST_COMPARE).tolist() == [0, 0, 1 + 8, 256, 64, 2 ** 30 - 1]
    assert N.assess_cost(N.COST_COMPARE, N.FMT_S16, N.MEM_DEVICE)[2] == 1
    lengths = (5000, 12345, 700, 9000, 3000, 7000)
    per = [21 * n + 256 for n in lengths]
    assert per == [105256, 259501, 14956, 189256, 63256, 147256]
    assert N.stft_chunks(lengths, c, 280000).tolist() == [0, 1, 1, 2, 2, 3]
    assert N.stft_chunks(lengths, c, 274456).tolist() == [0, 1, 2, 2, 2, 3]      # one byte less than (12345, 700)
    assert N.stft_chunks(lengths, c, sum(per)).tolist() == [0] * 6 and N.stft_chunks(lengths, c, sum(per) - 1).tolist() == [0] * 5 + [1]
    assert N.stft_chunks((0, 5000, 0), c, 1).tolist() == [-1, 0, -1]
    # the bound holds for every frame length: the slots of both framings and the span records of a clip
    for n in (1, 4095, 4096, 4097, 40000):
        for fl in (1, 2, 3, 80, 441):
            frames = 1 + (n + 2 * (fl // 2) - fl) // fl
            spans = -(-n // 4096)
            assert 2 * 8 * (frames + 1 + spans) + 16 * spans + 56 + 80 + 4 <= 17 * n + 256
    with pytest.raises(ValueError):
        N.assess_cost(2)
    with pytest.raises(ValueError):
        N.assess_cost(0, 7)


def test_refusals_need_no_device():
    from audio_feature_extraction_amd import _native as N
    from audio_feature_extraction_amd import quality as Q
    y = K.tone(16000, 2000)
    N.assess_host(y, 1, 1)
    for fs, fl in ((0, 10), (10, 0), (-3, 10)):
        with pytest.raises(ValueError, match="frame lengths"):
            N.assess_host(y, fs, fl)
    for thr in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="threshold_db"):
            N.assess_host(y, 160, 1600, thr)
    with pytest.raises(ValueError, match="noise_cap"):
        N.assess_host(y, 160, 1600, -40.0, -1)
    with pytest.raises(ValueError):
        N.assess_host(y.astype(np.float64), 160, 1600)
    with pytest.raises(ValueError):
        N.compare_host(y, K.as_s16(y))
    with pytest.raises(ValueError, match="100 Hz"):
        Q.assess(y, 50)
    with pytest.raises(ValueError, match="threshold_db"):
        Q.assess(y, 16000, threshold_db=float("nan"))
    with pytest.raises(ValueError, match="1-D"):
        Q.assess(np.zeros((2, 100), np.float32), 16000)
    with pytest.raises(ValueError, match="empty"):
        Q.assess(np.zeros(0, np.float32), 16000)
    with pytest.raises(ValueError, match="finite"):
        Q.assess(np.array([0.1, np.nan, 0.2] * 10, np.float32), 16000)
    with pytest.raises(ValueError, match="one per signal"):
        Q.assess_batch([y, y], [16000, 8000, 8000])
    assert Q.assess_batch([], 16000) == [] and Q.compare_batch([]) == []


def test_host_executor_matches_the_restatement():
    from audio_feature_extraction_amd import _native as N
    for name, y, sr in K.every_clip():
        fs, fl = R.frame_lengths(sr)
        for v in (y, K.as_s16(y)):
            r = N.assess_host(v, fs, fl)
            if v.size == 0:
                assert r["status"] == N.CLIP_TOO_SHORT and np.isnan(r["rec"]).all()
                continue
            assert r["status"] == N.CLIP_OK, name
            check_record(r["rec"], v, fs, fl, f"{name} {v.dtype}")
    for (name, sr), y in K.SEGMENTED.items():
        fs, fl = R.frame_lengths(sr)
        assert tuple(N.assess_host(y, fs, fl)["rec"][:3]) == K.SEG_COUNTS[name]
    # other thresholds and caps; the clamp at -80 dB
    y = K.SEGMENTED[("a", 16000)]
    check_record(N.assess_host(y, 160, 1600, -70.0)["rec"], y, 160, 1600, "-70", -70.0)
    assert N.assess_host(y, 160, 1600, -85.0)["rec"][1] == 0 == R.record(y, 160, 1600, -85.0)[1]
    assert N.assess_host(y, 160, 1600, -40.0, 100)["rec"][6] == pytest.approx(np.mean(y[:100].astype(np.float64) ** 2), rel=1e-12)
    bad = y.copy()
    bad[777] = np.inf
    r = N.assess_host(bad, 160, 1600)
    assert r["status"] == N.CLIP_NONFINITE and np.isnan(r["rec"]).all()


def test_compare_host_matches_the_restatement():
    from audio_feature_extraction_amd import _native as N
    from audio_feature_extraction_amd import quality as Q
    y = K.lead_in(16000, 20000)
    dc = (0.5 + 1e-3 * np.sin(np.arange(20000) * 0.05)).astype(np.float32)
    dc2 = (0.5 + 1e-3 * np.sin(np.arange(20000) * 0.05 + 0.3)).astype(np.float32)
    for r, d in ((y, y), (y, -y), (y, y[:7000] * np.float32(0.5)), (dc, dc2), (K.as_s16(y), K.as_s16(y * np.float32(0.7)))):
        rec = N.compare_host(r, d)["rec"]
        n = min(r.size, d.size)
        rf = R._signal(r, False)[:n]
        df = R._signal(d, False)[:n]
        ef = (R._signal(d, True)[:n] - R._signal(r, True)[:n]).astype(np.float64)
        want = [n, rf.sum(), df.sum(), (rf * rf).sum(), (df * df).sum(), (rf * df).sum(), (ef * ef).sum(),
                ((rf - rf.mean()) ** 2).sum(), ((df - df.mean()) ** 2).sum(), ((rf - rf.mean()) * (df - df.mean())).sum()]
        np.testing.assert_allclose(rec, want, rtol=1e-10, atol=1e-9)
        got, ex = Q.compare_batch([(r, d)])[0], R.pair_exact(r, d)
        for k in ("correlation", "mse", "snr"):
            assert abs(got[k] - ex[k]) <= 1e-12 * abs(ex[k]) + (1e-12 if k == "snr" else 0), (k, got[k], ex[k])
        assert abs(got["stoi"] - R.stoi_like(r, d)) <= 1e-12
    const = np.full(3000, 0.25, np.float32)
    got = Q.compare_batch([(const, y)])[0]
    assert np.isnan(got["correlation"]) and np.isnan(got["stoi"]) and np.isnan(Q.stoi_like(const, y))
    assert Q.stoi_like(y, y) == 1.0 and Q.compare_batch([(y, y)])[0]["snr"] == 100
    r = N.compare_host(y, np.zeros(0, np.float32))
    assert r["status"] == N.CLIP_TOO_SHORT and np.isnan(r["rec"]).all()


def test_quality_through_the_host_fallback(tmp_path, monkeypatch):
    from audio_feature_extraction_amd import quality as Q
    from audio_feature_extraction_amd import wavio
    monkeypatch.setattr(Q, "_on_gpu", lambda: False)              # the host executors, whether or not a GPU is visible
    clips = [(n, y, sr) for n, y, sr in K.every_clip() if y.size]
    got = Q.assess_batch([y for _, y, _ in clips], [sr for _, _, sr in clips])
    for (name, y, sr), g in zip(clips, got):
        check_keys(g, y, sr, name)
    y = K.SEGMENTED[("a", 16000)]
    a = Q.assess(y, 16000)
    assert a["silence_ratio"] == 200 / 290 and a["max_silence_duration"] == 1.2 and not a["silence_ok"]
    check_keys(Q.assess(y, 16000, threshold_db=-70), y, 16000, "threshold", -70.0)
    check_keys(Q.assess(K.as_s16(y), 16000), K.as_s16(y), 16000, "s16")
    z = Q.assess(np.zeros(8000, np.float32), 16000)
    assert (z["silence_ratio"], z["rms_dbfs"], z["peak_dbfs"], z["snr"], z["rms_cv"]) == (0, -100, -100, 0, 0)
    full = K.as_s16(K.tone(16000, 4000))
    full[100] = -32768
    assert Q.assess(full, 16000)["peak_dbfs"] == 0 and not Q.assess(full, 16000)["volume_ok"]
    lead = K.lead_in(16000, 32000)
    assert Q.estimate_snr(lead) == pytest.approx(R.estimate_snr(lead)["snr"], rel=1e-9)
    # files: the reference's record, its error record for a missing file and for one that is not RIFF/WAVE
    good, other, webm = str(tmp_path / "t.wav"), str(tmp_path / "o.wav"), str(tmp_path / "s.webm")
    W.write_wav(good, W.quantize(lead, "s32"), 16000, "s32")
    W.write_wav(other, W.quantize(K.lead_in(22050, 30000), "s16", 2), 22050, "s16")
    open(webm, "wb").write(b"\x1a\x45\xdf\xa3" + bytes(200))
    missing = str(tmp_path / "none.wav")
    res = Q.assess_files([good, missing, other, webm])
    assert [list(r) for r in res] == [FILE_KEYS, ["file_path", "file_name", "assessment_ok", "error"], FILE_KEYS,
                                      ["file_path", "file_name", "assessment_ok", "error"]]
    for r, p in zip(res, (good, missing, other, webm)):
        assert r["file_path"] == p and r["file_name"] == os.path.basename(p)
    assert res[1]["assessment_ok"] is False and res[3]["assessment_ok"] is False and res[1]["error"] and res[3]["error"]
    assert (res[0]["sample_rate"], res[0]["bit_depth"], res[0]["channels"], res[0]["duration"], res[0]["format_ok"]) == (16000, "32-bit", 1, 2.0, True)
    assert (res[2]["sample_rate"], res[2]["bit_depth"], res[2]["channels"], res[2]["format_ok"]) == (22050, "PCM_16", 2, False)
    assert not res[2]["assessment_ok"]
    for r, p in ((res[0], good), (res[2], other)):
        a = Q.assess(*wavio.load(p, None))
        for k in a:
            if k != "rms_std":
                assert r[k] == a[k], k
    assert res[0]["assessment_ok"] == all(res[0][k] for k in ("format_ok", "silence_ok", "volume_ok", "stability_ok", "snr_ok"))
    assert Q.assess_files([other], expected={"sample_rate": 22050, "subtype": "PCM_16", "channels": 2})[0]["format_ok"] is True
