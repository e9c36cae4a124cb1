"""Known answers for tests/assess_ref.py, the numpy restatement of the reference's recording screen and denoising scores:
answers that follow from the reference's expressions alone.  CPU only."""
import numpy as np
import pytest

from tests import assess_clips as K
from tests import assess_ref as R


@pytest.mark.parametrize("f32", [False, True])
def test_a_steady_tone_has_no_silence(f32):
    y = K.tone(16000, 16000)
    d = R.detect_silence(y, 16000, f32=f32)
    assert (d["n_short"], d["silent"], d["longest_run"]) == (101, 0, 0)
    assert d["silence_ratio"] == 0 and d["max_silence_duration"] == 0 and d["silence_ok"]
    v = R.check_volume_levels(y, f32)
    assert abs(v["rms_dbfs"] - 20 * np.log10(0.3 / np.sqrt(2))) < 0.01 and abs(v["peak_dbfs"] - 20 * np.log10(0.3)) < 0.01 and v["volume_ok"]
    s = R.check_amplitude_stability(y, 16000, f32)
    assert s["stability_ok"] and abs(s["rms_cv"] - 0.1193) < 1e-3     # 9 full frames, two half ones at 1 / sqrt(2) of their RMS
    assert not R.snr_is_robust(y)                                # the leading window has the clip's own power


@pytest.mark.parametrize("f32", [False, True])
def test_segments_give_the_exact_ratio_and_the_longest_run(f32):
    y = K.SEGMENTED[("a", 16000)]
    d = R.detect_silence(y, 16000, f32=f32)
    assert (d["n_short"], d["silent"], d["longest_run"]) == K.SEG_COUNTS["a"] == (290, 200, 120)
    assert d["silence_ratio"] == 200 / 290 and d["max_silence_duration"] == 1.2 and not d["silence_ok"]
    flags = R.silence_frames(y, 16000, f32=f32)
    assert flags.tolist() == [False] * 30 + [True] * 120 + [False] * 30 + [True] * 30 + [False] * 30 + [True] * 50
    # every rate: the same counts (the run lasts 120 frames of int(0.01 sr) samples)
    for sr in K.RATES:
        d = R.detect_silence(K.SEGMENTED[("a", sr)], sr, f32=f32)
        assert (d["n_short"], d["silent"], d["longest_run"]) == (290, 200, 120)
        assert d["max_silence_duration"] == 120 * int(sr * 0.01) / sr


def test_a_clip_that_starts_and_ends_in_silence():
    for sr in K.RATES:
        d = R.detect_silence(K.SEGMENTED[("b", sr)], sr)
        assert (d["n_short"], d["silent"], d["longest_run"]) == K.SEG_COUNTS["b"] == (100, 70, 50)   # the run to the last frame counts
    d = R.detect_silence(K.SEGMENTED[("b", 16000)], 16000)
    assert d["max_silence_duration"] == 0.5 and d["silence_ratio"] == 0.7 and not d["silence_ok"]


@pytest.mark.parametrize("f32", [False, True])
def test_an_all_zero_clip(f32):
    y = np.zeros(8000, np.float32)
    a = R.assess(y, 16000, f32=f32)
    assert a["silence_ratio"] == 0 and a["max_silence_duration"] == 0      # every frame equals the reference level
    assert a["rms_dbfs"] == -100 and a["peak_dbfs"] == -100 and not a["volume_ok"]
    assert a["snr"] == 0 and not a["snr_ok"] and a["rms_cv"] == 0 and a["stability_ok"]
    assert R.silence_is_robust(y, 16000) and R.snr_is_robust(y)


def test_a_clip_below_amin_has_no_silence():
    y = K.tone(16000, 8000, amp=5e-6)
    y[3000:6000] *= np.float32(1e-3)
    assert R.frame_rms(y, 160).max() < R.AMIN
    d = R.detect_silence(y, 16000)
    assert d["silent"] == 0 and d["silence_ratio"] == 0           # amin floors every frame and the reference alike
    assert R.silence_is_robust(y, 16000)


def test_full_scale_s16_peaks_at_zero_dbfs():
    q = K.as_s16(K.tone(16000, 4000))
    q[1234] = -32768
    v = R.check_volume_levels(q)
    assert v["peak_dbfs"] == 0 and not v["volume_ok"] and v["rms_dbfs"] > -30
    assert R.check_volume_levels(q, f32=True)["peak_dbfs"] == 0


def test_the_snr_branches():
    rng = np.random.default_rng(5)
    loud_first = np.concatenate([0.3 * rng.standard_normal(2000), 0.01 * rng.standard_normal(18000)]).astype(np.float32)
    noise, signal = R.snr_powers(loud_first)
    assert signal <= noise and R.estimate_snr(loud_first)["snr"] == 0 and R.snr_is_robust(loud_first)
    y = K.lead_in(16000, 32000)
    noise, signal = R.snr_powers(y)
    s = R.estimate_snr(y)
    assert R.snr_is_robust(y) and abs(s["snr"] - 10 * np.log10((signal - noise) / noise)) < 1e-12 and s["snr"] > 40 and s["snr_ok"]
    assert np.isnan(R.snr_powers(np.ones(9, np.float32))[0]) and R.estimate_snr(np.ones(9, np.float32))["snr"] == 0   # an empty window
    assert R.snr_powers(np.ones(10, np.float32))[0] == 1.0
    # the window is capped at 2000 samples
    z = np.concatenate([np.zeros(2000), np.ones(98000)]).astype(np.float32)
    assert R.snr_powers(z) == (0.0, 0.98)


@pytest.mark.parametrize("fl", [80, 160, 220, 441])
def test_frame_counts(fl):
    # librosa pads fl // 2 on either side and takes whole frames: 1 + len // fl for an even frame, and for an odd one
    # (441 at 44100 Hz) 1 + (len - 1) // fl -- a clip of exactly 441 samples has one frame
    for n in (1, fl - 1, fl, fl + 1, 5 * fl + 3):
        assert R.frame_rms(np.ones(n, np.float32), fl).size == 1 + (n + 2 * (fl // 2) - fl) // fl == 1 + (n - fl % 2) // fl
        if fl % 2 == 0:
            assert R.frame_rms(np.ones(n, np.float32), fl).size == 1 + n // fl
    # frame t covers [t fl - fl // 2, t fl - fl // 2 + fl) cut to the clip: the mean is over fl samples, zeros included
    y = np.arange(1, 2 * fl + 2, dtype=np.float64)
    r = R.frame_rms(y, fl)
    h = fl // 2
    assert r.size == 3
    np.testing.assert_allclose(r[0] ** 2, np.sum(y[:fl - h] ** 2) / fl, rtol=1e-13)
    np.testing.assert_allclose(r[1] ** 2, np.sum(y[fl - h:2 * fl - h] ** 2) / fl, rtol=1e-13)
    np.testing.assert_allclose(r[2] ** 2, np.sum(y[2 * fl - h:] ** 2) / fl, rtol=1e-13)


def test_record_matches_the_checks():
    y = K.MIXED[5][1]                                             # 8000 Hz, 2.3 s
    rec = dict(zip(R.RECORD, R.record(y, 80, 800)))
    d = R.detect_silence(y, 8000)
    assert (rec["n_short"], rec["silent"], rec["longest_run"]) == (d["n_short"], d["silent"], d["longest_run"])
    assert rec["n_long"] == 1 + y.size // 800 == R.frame_rms(y, 800).size and rec["peak"] == np.abs(y).max()
    noise, signal = R.snr_powers(y)
    assert rec["noise_mean_square"] == noise and rec["mean_square"] == signal
    assert rec["rms_long_std"] == R.check_amplitude_stability(y, 8000)["rms_std"]


def test_pair_scores():
    y = K.lead_in(16000, 20000)
    same = R.pair_stats(y, y)
    assert same["snr"] == 100 and same["mse"] == 0 and abs(same["correlation"] - 1) < 1e-12
    assert abs(R.stoi_like(y, y) - 1.0) < 1e-12                   # 0.5 + 0.3 + 0.2
    neg = R.pair_stats(y, -y)
    assert abs(neg["correlation"] + 1) < 1e-12 and abs(neg["snr"] - 10 * np.log10(0.25)) < 1e-9
    assert R.stoi_like(y, -y) == pytest.approx(0.3 * max(1 - 10 * neg["mse"], 0))
    const = np.full(5000, 0.25, np.float32)
    assert np.isnan(R.pair_stats(const, y)["correlation"]) and np.isnan(R.stoi_like(const, y))    # Python's max(nan, 0)
    # the shorter side decides the length
    assert R.pair_stats(y, y[:7000] * np.float32(0.5)) == R.pair_stats(y[:7000], y[:7000] * np.float32(0.5))
    ex, st = R.pair_exact(y, y * np.float32(0.9)), R.pair_stats(y, y * np.float32(0.9))
    for k in ("correlation", "mse", "snr"):
        assert abs(ex[k] - st[k]) <= 1e-12 * abs(ex[k])


def test_the_robustness_predicate_refuses_borderline_clips():
    y = K.tone(16000, 16000)
    y[4000:8000] *= np.float32(10 ** (-40.004 / 20))               # frames 0.004 dB below the threshold
    assert not R.silence_is_robust(y, 16000) and R.silence_is_robust(y, 16000, threshold_db=-30.0)
    z = np.full(4000, R.AMIN * (1 + 1e-4), np.float32)              # the loudest frame sits on amin
    assert not R.silence_is_robust(z, 16000)
