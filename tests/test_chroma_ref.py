"""Known answers of the restatement tests/chroma_ref.py (the spec of afx_chroma_batch), and the robustness of every input the
GPU test pins a tuning on.  CPU only."""
import numpy as np
import pytest

from tests import chroma_ref as R


def pinned_inputs():
    """(name, sr, signal) of every input tests/test_gpu_chroma.py pins the estimated tuning on"""
    from audio_feature_extraction_amd.synth import make_clip
    out = [("clip16000", 16000, make_clip(16000, 16000, 2.0)), ("clip22050", 22050, make_clip(22050, 22050, 2.0)),
           ("speech16000", 16000, make_clip(16001, 16000, 1.7, speechy=True)),
           ("nopeak22050", 22050, make_clip(22051, 22050, 1.7, speechy=True))]
    for sr in (16000, 22050, 44100):
        out.append((f"octave{sr}", sr, R.tones(sr, 2 * sr, (452.0, 904.0))))
    for sr in (16000, 44100):
        out.append((f"chord{sr}", sr, R.tones(sr, 2 * sr, [1.01 * f for f in (261.63, 329.63, 392.0, 523.25)], noise=0.01)))
    return out


def unpinned_inputs():
    rng = np.random.default_rng(11)
    return [("noise22050", 22050, (0.3 * rng.standard_normal(2 * 22050)).astype(np.float32)),
            ("chord22050", 22050, R.tones(22050, 2 * 22050, [1.01 * f for f in (261.63, 329.63, 392.0, 523.25)], noise=0.01)),
            ("tone440", 22050, R.tones(22050, 2 * 22050, (440.0,)))]


@pytest.mark.parametrize("sr,want", [(22050, 0.46), (44100, 0.46), (16000, 0.48)])
def test_tuning_of_a_452_hz_tone(sr, want):
    y = R.tones(sr, 2 * sr, (452.0, 904.0))
    for f32 in (False, True):
        assert R.estimate_tuning(R.power_spectrogram(y, f32), sr) == pytest.approx(want, abs=1e-12)


def test_tuning_grid():
    assert R.EDGES[50] == 0.0 and R.EDGES.shape == (101,)
    np.testing.assert_array_equal(R.EDGES[:100], np.arange(100) * 0.01 + -0.5)


@pytest.mark.parametrize("sr", [16000, 22050, 44100])
def test_filters(sr):
    w = R.chroma_filters(sr, 0.0)
    assert w.shape == (12, 1025) and w.dtype == np.float32
    assert w.min() >= 0.0 and w.max() <= 1.0
    k = int(round(440.0 * 2048 / sr))
    assert int(np.argmax(w[:, k])) == 9                      # A, counted from C (base_c)
    assert np.all(w[:, 0] < 1e-3)                            # the DC column sits 1.5 octaves below bin 1, far down the octave weight


def test_chroma_frames_peak_at_one_or_are_zero():
    from audio_feature_extraction_amd.synth import make_clip
    y = np.concatenate([make_clip(3, 22050, 0.5), np.zeros(4096, np.float32)])
    for f32 in (False, True):
        c = R.chroma_stft(y, 22050, f32=f32)
        assert c.shape == (12, 1 + y.size // 512)
        mx = c.max(axis=0)
        assert np.all((mx == 1.0) | (np.abs(c).max(axis=0) == 0.0))
        assert (mx == 1.0).any() and (mx == 0.0).any() and c.min() >= 0.0


def test_silence():
    y = np.zeros(3000, np.float32)
    assert R.estimate_tuning(R.power_spectrogram(y), 22050) == 0.0
    assert not R.chroma_stft(y, 22050).any()
    assert not R.melspectrogram(y, 22050).any()


def test_peak_rules_on_a_hand_made_spectrum():
    sr = 22050
    S = np.zeros((1025, 1))
    S[99:102, 0] = (2.0, 8.0, 4.0)        # a peak at 100: b = 1, a = -10, shift = 0.1, mag = 8 + 0.5 * 1 * 0.1
    S[200:202, 0] = (3.0, 3.0)            # a plateau: only 200 is a peak (> left, >= right); b = 1.5, a = -3, shift 0.5
    S[300, 0] = 0.7                       # below a tenth of the frame maximum: masked
    S[5, 0] = 6.0                         # 53.8 Hz: under fmin
    S[400, 0] = 7.0                       # 4306 Hz: over fmax
    S[13, 0] = 5.0                        # 139.97 Hz: just under fmin
    S[14, 0] = 1.0                        # 150.7 Hz, > its masked left neighbour?  no: S[13] = 5 is unmasked and larger
    peak, pitch, mag = R.piptrack(S, sr)
    assert np.flatnonzero(peak[:, 0]).tolist() == [100, 200]
    assert pitch[100, 0] == pytest.approx(100.1 * sr / 2048) and mag[100, 0] == pytest.approx(8.05)
    assert pitch[200, 0] == pytest.approx(200.5 * sr / 2048) and mag[200, 0] == pytest.approx(3.0 + 0.5 * 1.5 * 0.5)
    # |b| >= |a|: no shift
    S2 = np.zeros((1025, 1))
    S2[149:152, 0] = (0.0, 1.0, 1.0)      # b = 0.5, a = -1 -> shift 0.5; then a flat pair where |b| = |a|
    S2[50:53, 0] = (1.0, 2.0, 0.0)        # b = -0.5, a = -3
    S2[60:63, 0] = (0.0, 3.0, 3.0)
    S2[61, 0] = 2.0                       # (0, 2, 3): not a peak at 61; 62: (2, 3, 0): b = -1, a = -4
    peaks, kept, counts = R.tuning_histogram(S2, sr)
    assert peaks == 3 and kept == 2 and counts.sum() == 2     # magnitudes 1.125, 2.04, 3.125: the median 2.04 keeps two
    # the median of an even count is the mean of the two middle values
    S3 = np.zeros((1025, 1))
    for k, v in ((50, 1.0), (60, 2.0), (70, 3.0), (80, 4.0)):
        S3[k, 0] = v                      # isolated bins: b = 0, mag = v; median 2.5 keeps 3 and 4
    assert R.tuning_histogram(S3, sr)[:2] == (4, 2)


def test_pinned_inputs_are_robust_and_the_others_are_not():
    for name, sr, y in pinned_inputs():
        assert R.tuning_is_robust(y, sr), name
    for name, sr, y in unpinned_inputs()[:1]:
        assert not R.tuning_is_robust(y, sr), name
    name, sr, y = pinned_inputs()[3]
    assert R.tuning_histogram(R.power_spectrogram(y), sr)[0] == 0, name       # the no-peak case


def test_timbre_features_keys():
    from audio_feature_extraction_amd.synth import make_clip
    d = R.timbre_features(make_clip(1, 22050, 0.5), 22050)
    assert list(d) == ["mel_energy_mean", "mel_energy_std", "chroma_mean", "chroma_std", "mfcc_mean", "mfcc_std"]
    assert all(type(v) is float and np.isfinite(v) for v in d.values())
