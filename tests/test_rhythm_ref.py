"""Known answers of the restatement tests/rhythm_ref.py (the spec of afx_rhythm_batch), and the robustness of every input the
GPU test pins a tempo on.  CPU only."""
import functools

import numpy as np
import pytest

from tests import rhythm_ref as R

# (rate, click period in bpm, the restatement's tempo): bpm[lag] of the lag nearest the true period; 200 bpm folds to
# half its rate under the prior round 120
CLICKS = ((22050, 60, 60.093), (22050, 90, 89.103), (22050, 120, 117.454), (22050, 150, 151.999), (16000, 60, 60.484),
          (16000, 120, 117.188), (44100, 120, 120.185), (22050, 200, 99.384))


@functools.lru_cache(maxsize=None)
def pinned_inputs():
    """(name, sr, signal) of every input tests/test_gpu_rhythm.py pins the tempo on"""
    out = [(f"clicks{bpm}_{sr}", sr, R.clicks(sr, bpm)) for sr, bpm, _ in CLICKS]
    out.append(("silence22050", 22050, np.zeros(30000, np.float32)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def unpinned_inputs():
    sr = 22050
    t = np.arange(3 * sr) / float(sr)
    gate = (np.floor(t / 0.37) % 2 == 0).astype(np.float64)
    return (("noise22050", sr, (0.3 * np.random.default_rng(1).standard_normal(5 * sr)).astype(np.float32)),
            ("gated440", sr, (0.4 * gate * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)),
            ("clicks_gap22050", sr, R.clicks(sr, 100, seconds=6.0, silent=(2.0, 3.5))))


def test_envelope_starts_with_three_zeros_and_short_clips_are_zero():
    y = (0.3 * np.random.default_rng(3).standard_normal(20000)).astype(np.float32)
    for dtype in ("f64", "f32", "fft32"):
        e = R.onset_strength(y, 22050, dtype)
        assert e.shape == (1 + y.size // 512,) and not e[:3].any() and (e[3:] > 0).all()
        assert e.dtype == (np.float64 if dtype == "f64" else np.float32)
        for n, T in ((300, 1), (700, 2), (1500, 3)):
            e = R.onset_strength(y[:n], 22050, dtype)
            assert e.shape == (T,) and not e.any()
            assert R.tempo(y[:n], 22050, dtype) == 0.0
        e = R.onset_strength(y[:1600], 22050, dtype)          # T = 4: exactly one value behind the three zeros
        assert e.shape == (4,) and np.count_nonzero(e) == 1 and e[3] > 0


def test_silence_has_tempo_zero():
    y = np.zeros(30000, np.float32)
    assert not R.onset_strength(y, 22050).any()
    assert R.tempo(y, 22050) == 0.0 and R.tempo(y, 22050, "f32") == 0.0
    d = R.rhythm_features(y, 22050)
    assert list(d) == list(R.KEYS) and all(v == 0.0 for v in d.values())


@pytest.mark.parametrize("sr,win,kmin", [(22050, 344, 9), (16000, 250, 6), (44100, 689, 17)])
def test_tempo_table(sr, win, kmin):
    w, k, bpm, logprior = R.tempo_table(sr)
    assert (w, k) == (win, kmin) and bpm.shape == logprior.shape == (win,)
    assert bpm[0] == np.inf and bpm[k] < 320.0 <= bpm[k - 1]
    assert np.all(np.isneginf(logprior[:k])) and np.all(np.isfinite(logprior[k:]))
    assert bpm[1] == 60.0 * sr / 512.0
    j = int(np.argmax(logprior))                                     # the prior peaks at the lag nearest 120 bpm in octaves
    assert j == k + int(np.argmin(np.abs(np.log2(bpm[k:] / 120.0))))


def test_fft_route_equals_the_direct_sum():
    y = (0.3 * np.random.default_rng(5).standard_normal(12000)).astype(np.float32)
    e = R.onset_strength(y, 22050)
    a, b = R.tempogram(e, 22050), R.tempogram_direct(e, 22050)
    assert a.shape == (344, e.size)
    assert np.max(np.abs(a - b)) < 1e-13
    assert np.all(a[0, np.abs(b).max(axis=0) > 0] == 1.0)          # lag 0 is the maximum
    e32 = e.astype(np.float32)
    assert np.max(np.abs(R.tempogram(e32, 22050, f32=True) - R.tempogram(e32, 22050))) < 1e-5


@pytest.mark.parametrize("sr,bpm,want", CLICKS)
def test_click_tracks(sr, bpm, want):
    y = R.clicks(sr, bpm)
    tempo, lag, _, _ = R.tempo_from(R.onset_strength(y, sr), sr)
    assert tempo == pytest.approx(want, abs=5.01e-4)          # the table is rounded to three decimals
    period = 60.0 * sr / (512.0 * bpm)                               # the true period in frames (twice it where 200 bpm folds)
    assert min(abs(lag - period), abs(lag - 2 * period)) <= 1.0
    assert R.tempo(y, sr, "f32") == tempo


def test_pinned_inputs_are_robust_and_the_others_are_not():
    for name, sr, y in pinned_inputs():
        lags, lead = R.tempo_lead(y, sr)
        print(f"{name}: lag {lags[0]} lead {lead:.4f}")
        assert R.tempo_is_robust(y, sr), (name, lags, lead)
    for i, (name, sr, y) in enumerate(unpinned_inputs()):
        lags, lead = R.tempo_lead(y, sr)
        print(f"{name}: lags {sorted(set(lags))} lead {lead:.4f}")
        if i == 0:                                                    # white noise: one lag, but a lead of a few 1e-3
            assert not R.tempo_is_robust(y, sr), (name, lags, lead)


def test_rhythm_features_keys():
    d = R.rhythm_features(R.clicks(22050, 90, seconds=4.0), 22050)
    assert list(d) == ["tempo", "rhythm_regularity", "onset_strength_mean", "onset_strength_std"]
    assert all(type(v) is float and np.isfinite(v) for v in d.values())
    assert d["rhythm_regularity"] == d["onset_strength_std"] / (d["onset_strength_mean"] + 1e-8)
