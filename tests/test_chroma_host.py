"""CPU-only checks of the chroma feature's host side: the filterbank builder of libafx.so against the restatement, and the
argument checks of audio_feature_extraction_amd.feature (which fail before any device is touched)."""
import numpy as np
import pytest

from audio_feature_extraction_amd import _native as N
from tests import chroma_ref as R


@pytest.mark.parametrize("sr", [16000, 22050, 44100])
@pytest.mark.parametrize("tuning", [-0.5, -0.07, 0.0, 0.46])
def test_filter_table_matches_the_restatement(sr, tuning):
    # both are float64 formulas rounded once; libm and numpy may differ in the last double bit before that rounding
    got, ref = N.chroma_filters(sr, tuning), R.chroma_filters(sr, tuning)
    assert got.shape == ref.shape == (12, 1025) and got.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(ref), np.finfo(np.float32).tiny))
    assert np.all(np.abs(got.astype(np.float64) - ref) <= ulp), float(np.max(np.abs(got.astype(np.float64) - ref) / ulp))


def test_filter_builder_rejects_bad_arguments():
    with pytest.raises(ValueError):
        N.chroma_filters(0, 0.0)
    with pytest.raises(ValueError):
        N.chroma_filters(22050, float("nan"))


@pytest.mark.parametrize("kw", [{"n_fft": 1024}, {"hop_length": 256}, {"norm": 2}, {"n_chroma": 24}, {"window": "hamming"},
                                {"center": False}, {"win_length": 1024}])
def test_non_default_keywords_raise(kw):
    from audio_feature_extraction_amd import feature
    y = np.zeros(4096, np.float32)
    with pytest.raises(ValueError):
        feature.chroma_stft(y, 22050, **kw)
    with pytest.raises(ValueError):
        feature.chroma_stft_batch([y], 22050, **kw)


@pytest.mark.parametrize("kw", [{"n_mels": 64}, {"power": 1.0}, {"fmax": 8000.0}, {"htk": True}])
def test_non_default_mel_keywords_raise(kw):
    from audio_feature_extraction_amd import feature
    with pytest.raises(ValueError):
        feature.melspectrogram(np.zeros(4096, np.float32), 22050, **kw)
    with pytest.raises(ValueError):
        feature.estimate_tuning(np.zeros(4096, np.float32), 22050, resolution=0.02)


def test_bad_signals_raise():
    from audio_feature_extraction_amd import feature
    with pytest.raises(ValueError):
        feature.chroma_stft(np.zeros((2, 4096), np.float32))
    with pytest.raises(ValueError):
        feature.melspectrogram(np.zeros((2, 4096), np.float32))
    with pytest.raises(ValueError):
        feature.chroma_stft(np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        feature.estimate_tuning(np.array([0.0, np.nan], np.float32))
    with pytest.raises(ValueError):
        feature.chroma_stft(np.zeros(4096, np.float32), tuning=float("inf"))
