"""Known answers of the restatement tests/filt_ref.py of the experiment extractor's preprocess_audio.  CPU only."""
import numpy as np
import pytest
import scipy.signal

from tests import filt_ref as F


def _amp_phase(y, f, sr):
    """amplitude and phase (against sin) of the f Hz component of the middle half of y, by least squares"""
    n = y.size
    t = np.arange(n) / sr
    sl = slice(n // 4, 3 * n // 4)
    A = np.stack([np.sin(2 * np.pi * f * t[sl]), np.cos(2 * np.pi * f * t[sl])], axis=1)
    (s, c), *_ = np.linalg.lstsq(A, y[sl], rcond=None)
    return float(np.hypot(s, c)), float(np.arctan2(c, s))


@pytest.mark.parametrize("sr", F.RATES)
def test_stop_band_tone_is_attenuated_by_the_squared_response(sr):
    """forward and backward: the magnitude response applies twice, the phase cancels"""
    t = np.arange(2 * sr) / sr
    y = F.highpass(np.sin(2 * np.pi * 50.0 * t).astype(np.float32), sr)
    b, a = F.butter_ba(sr)
    _, h = scipy.signal.freqz(b, a, worN=[50.0], fs=sr)
    amp, ph = _amp_phase(y, 50.0, sr)
    assert amp == pytest.approx(abs(h[0]) ** 2, rel=1e-4)
    assert abs(h[0]) ** 2 < 2e-6                                   # (50 / 200)^10, about 1e-6
    assert abs(ph) < 1e-3


@pytest.mark.parametrize("sr", F.RATES)
def test_pass_band_tone_passes_with_unit_gain_and_zero_phase(sr):
    t = np.arange(sr) / sr
    x = np.sin(2 * np.pi * 2000.0 * t).astype(np.float32)
    y = F.highpass(x, sr)
    amp, ph = _amp_phase(y, 2000.0, sr)
    assert amp == pytest.approx(1.0, abs=1e-6) and abs(ph) < 1e-6
    assert np.max(np.abs(y[sr // 4:3 * sr // 4] - x[sr // 4:3 * sr // 4])) < 1e-6


@pytest.mark.parametrize("sr", F.RATES)
def test_output_peak_is_one_and_the_stages_are_the_documented_ones(sr):
    y = F.signal(5000, sr, 1)
    out = F.preprocess_experiment(y, sr)
    assert out.dtype == np.float64 and out.shape == y.shape and np.max(np.abs(out)) == 1.0
    u = F.filter_input(y)
    yn = y / np.max(np.abs(y))
    assert u.dtype == np.float32 and yn.dtype == np.float32
    assert u[0] == yn[0] + (2 * yn[0] - yn[1])                      # librosa's initial state
    np.testing.assert_array_equal(u[1:], yn[1:] + np.float32(-0.98) * yn[:-1])
    # scaling the input does not change the result: the first normalisation removes it (a power of two scales exactly)
    np.testing.assert_array_equal(F.preprocess_experiment(4.0 * y, sr), out)


def test_failures_are_none_and_silence_is_zeros():
    assert F.preprocess_experiment(np.ones(F.PADLEN, np.float32), 22050) is None          # filtfilt raises: n <= padlen
    assert F.preprocess_experiment(np.ones(F.PADLEN + 1, np.float32), 22050) is not None
    bad = F.signal(100, 22050, 0)
    bad[50] = np.nan
    assert F.preprocess_experiment(bad, 22050) is None
    z = F.preprocess_experiment(np.zeros(100, np.float32), 22050)
    assert z.shape == (100,) and not z.any()


def test_conditioning_of_noise_stays_below_the_cap():
    for sr in F.RATES:
        c = F.conditioning(F.filter_input(F.signal(12305, sr, 3)), sr)
        print(sr, c)
        assert 0 < c <= F.MAX_CONDITIONING
