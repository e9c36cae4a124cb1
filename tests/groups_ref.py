"""Restatement of what the experiment extractor's ``extract_all_features`` computes from one signal
(04_feature_extraction_experiment/feature_extractor.py:624-687): ``preprocess_audio`` once, then the spectral, harmonic,
timbre and rhythm groups on the same ``(y, sr)``, merged into one dict in that order.  It only composes the restatements
the groups already have -- tests/filt_ref.py, oracle/cpu_ref.py, tests/hpss_ref.py, tests/chroma_ref.py,
tests/rhythm_ref.py -- and is the spec of afx_groups_batch and ``extract_signal_features_batch``."""
import numpy as np
import scipy.fft

from oracle import cpu_ref
from tests import chroma_ref, filt_ref, hpss_ref, rhythm_ref

GROUPS = ("spectral", "harmonic", "timbre", "rhythm")
SPECTRAL_KEYS = tuple(f"spectral_{k}_{s}" for k in ("centroid", "bandwidth", "rolloff", "contrast") for s in ("mean", "std"))
HARMONIC_KEYS = ("harmonic_energy", "harmonic_ratio", "harmonic_freq_mean", "harmonic_freq_std")
KEYS = {"spectral": SPECTRAL_KEYS, "harmonic": HARMONIC_KEYS, "timbre": chroma_ref.KEYS, "rhythm": rhythm_ref.KEYS}


def preprocess(y, sr):
    """the signal every group sees: float32 (the reference's float64 result rounded once), or None where the reference's
    preprocess_audio returns None"""
    out = filt_ref.preprocess_experiment(np.asarray(y, np.float32), sr)
    return None if out is None else out.astype(np.float32)


def group_features(y, sr, group) -> dict:
    if group == "spectral":
        return {k: float(v) for k, v in cpu_ref.extract_spectral_features(y, sr).items()}
    if group == "harmonic":
        return hpss_ref.harmonic_features(y, sr)
    if group == "timbre":
        return chroma_ref.timbre_features(y, sr)
    if group == "rhythm":
        return rhythm_ref.rhythm_features(y, sr)
    raise ValueError(f"unknown feature group {group!r}")


def signal_features(y, sr, preprocess_first=True, groups=GROUPS):
    """the merged dict of the asked groups in the reference's order, or None where its preprocess fails"""
    for g in groups:
        if g not in GROUPS:
            raise ValueError(f"unknown feature group {g!r}")
    y = np.asarray(y, np.float32)
    if preprocess_first:
        y = preprocess(y, sr)
        if y is None:
            return None
    elif y.size == 0 or not np.isfinite(y).all():
        return None
    out = {}
    for g in GROUPS:
        if g in groups:
            out.update(group_features(y, sr, g))
    return out


def _magnitude_f32(y, n_fft=2048, hop_length=512, window="hann"):
    """the magnitude spectrogram in librosa's dtypes for float32 audio: float32 frames, a complex64 FFT"""
    yp = np.pad(np.asarray(y, np.float32), n_fft // 2)
    T = 1 + (yp.size - n_fft) // hop_length
    idx = np.arange(n_fft)[:, None] + hop_length * np.arange(T)[None, :]
    w = cpu_ref.get_window(window, n_fft).astype(np.float32)
    return np.abs(scipy.fft.rfft(yp[idx] * w[:, None], axis=0)).astype(np.float32)


def contrast_is_well_conditioned(y, sr) -> bool:
    """True when spectral_contrast's mean and std may be held to 1e-4 of their size in float32 at all: the restatement
    evaluated on a float32 STFT -- what librosa itself computes for float32 audio -- stays within a quarter of that bound
    of the float64 one.  Behind the experiment's preprocess most signals fail this: filtfilt squares the high-pass's response,
    the lowest bins of the 0 - 200 Hz band are left at rounding level, and that band's valley (the smallest of its bins)
    is whatever the FFT's own error makes of them."""
    c64 = cpu_ref.spectral_contrast(y, sr)
    keep = cpu_ref._magnitude_spectrogram
    cpu_ref._magnitude_spectrogram = _magnitude_f32
    try:
        c32 = cpu_ref.spectral_contrast(y, sr)
    finally:
        cpu_ref._magnitude_spectrogram = keep
    return all(abs(float(f(c32)) - float(f(c64))) <= 0.25e-4 * max(abs(float(f(c64))), 1.0) for f in (np.mean, np.std))
