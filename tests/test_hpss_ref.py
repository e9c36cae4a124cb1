"""CPU checks of the harmonic-percussive oracle (tests/hpss_ref.py) and of effects' argument checks (no device needed)."""
import numpy as np
import pytest
from scipy import ndimage

from tests import hpss_ref as R


@pytest.mark.parametrize("T", [1] + list(range(3, 41)))
def test_median_rule_equals_scipy(T):
    S = np.random.default_rng(T).random((40, T)).astype(np.float32)
    np.testing.assert_array_equal(R.median_time(S), ndimage.median_filter(S, size=(1, 31), mode="reflect"))
    np.testing.assert_array_equal(R.median_freq(S), ndimage.median_filter(S, size=(31, 1), mode="reflect"))


def test_median_rule_differs_from_scipy_at_two_frames():
    # the periodic mirror of [a, b] is a b b a a b b a ...: every 31-wide window holds 15 or 16 of each value.  scipy's
    # extended row at T = 2 holds a 0.0 that is not in the data; the GPU and the oracle follow the mirror.
    S = np.array([[0.82, 0.33]], np.float32)
    ours = R.median_time(S)
    assert set(ours.ravel()) <= {np.float32(0.82), np.float32(0.33)}
    assert not np.array_equal(ours, ndimage.median_filter(S, size=(1, 31), mode="reflect"))


@pytest.mark.parametrize("n", [300, 700, 5000, 22050])
def test_harmonic_plus_percussive_is_the_signal(n):
    y = np.random.default_rng(n).standard_normal(n)
    h, p = R.hpss(y)[:2]
    assert np.max(np.abs(h + p - y)) <= 1e-12 * max(1.0, np.max(np.abs(y)))


def test_steady_tone_is_harmonic():
    sr = 22050
    y = np.sin(2 * np.pi * 440.0 * np.arange(int(1.5 * sr)) / sr)
    f = R.harmonic_features(y, sr)
    assert f["harmonic_ratio"] > 0.99


@pytest.mark.parametrize("n", [7000, 100000])
def test_click_train_has_no_harmonic_energy(n):
    y = R.click_train(n)
    h = R.hpss(y)[0]
    assert np.all(h == 0.0)
    assert R.harmonic_features(y, 22050, h)["harmonic_energy"] == 0.0


def test_float32_variant_is_close():
    y = np.random.default_rng(3).standard_normal(9000).astype(np.float32)
    h64, h32 = R.hpss(y)[0], R.hpss(y, f32=True)[0]
    assert h32.dtype == np.float32
    assert np.max(np.abs(h32 - h64)) <= 1e-5 * np.max(np.abs(y))


@pytest.mark.parametrize("kw", [{"kernel_size": 17}, {"kernel_size": (31, 31)}, {"power": 1.0}, {"margin": 2.0}])
def test_effects_reject_non_default_arguments(kw):
    from audio_feature_extraction_amd import effects
    y = np.zeros(1000, np.float32)
    for f in (effects.hpss, effects.harmonic, effects.percussive):
        with pytest.raises(ValueError):
            f(y, **kw)
    with pytest.raises(ValueError):
        effects.hpss_batch([y], **kw)


@pytest.mark.parametrize("y", [np.zeros((2, 100), np.float32), np.zeros(0, np.float32),
                               np.array([0.0, np.nan, 1.0], np.float32), np.array([np.inf] * 10, np.float32)])
def test_effects_reject_bad_signals(y):
    from audio_feature_extraction_amd import effects
    for f in (effects.hpss, effects.harmonic, effects.percussive):
        with pytest.raises(ValueError):
            f(y)
    with pytest.raises(ValueError):
        effects.hpss_batch([np.ones(10, np.float32), y])
