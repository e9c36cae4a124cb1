"""Restatement, with scipy, of the experiment extractor's preprocess_audio
(04_feature_extraction_experiment/feature_extractor.py:133-154) and of its filter stage alone; the cases and the tolerance
the filter tests share.  float32 in, as the reference's loader hands it over; the filter stage returns scipy's float64.

    y = librosa.util.normalize(y)                       float32: y / max|y|, unchanged below tiny(float32)
    y = librosa.effects.preemphasis(y, coef=0.98)       float32, oracle.cpu_ref.preemphasis
    b, a = scipy.signal.butter(5, 200 / (sr / 2), btype='high')
    y = scipy.signal.filtfilt(b, a, y)                  float64 (the odd extension in the input's float32)
    y = librosa.util.normalize(y, norm=np.inf, axis=0)  float64

Tolerance (outputs scaled so that the reference's peak is 1):  |got - ref| <= 2^-23 + 4 conditioning(case).  The first term
is the one float32 rounding of the result, <= 2^-25 for |v| <= 1, with a factor four for float64 noise in the peak
division.  The second is the reference's own indeterminacy: the distance between scipy's sosfiltfilt and filtfilt on the
case's filter input, i.e. between two float64 evaluations of the same filter.  It is computed from scipy alone, and every
case must keep it below 2^-20 (asserted where the bound is used)."""
import functools

import numpy as np
import scipy.signal

from oracle import cpu_ref as R

RATES = (8000, 16000, 22050, 48000)
PADLEN = 18                    # scipy.signal.filtfilt's default for a 5th-order (b, a): 3 * max(len(a), len(b))
COEF = 0.98
EPS32 = 2.0 ** -23
MAX_CONDITIONING = 2.0 ** -20


def normalize(y: np.ndarray) -> np.ndarray:
    """librosa.util.normalize(y, norm=np.inf, axis=0) of a 1-D array: the quotient is formed in float64 and stored in y's
    dtype; a peak below tiny(y.dtype) divides by 1; a NaN / inf raises."""
    if not np.isfinite(y).all():
        raise ValueError("Input must be finite")
    length = np.max(np.abs(y).astype(np.float64))
    if length < np.finfo(y.dtype).tiny:
        length = 1.0
    return (y.astype(np.float64) / length).astype(y.dtype)


@functools.lru_cache(maxsize=None)
def butter_ba(sr: int):
    return scipy.signal.butter(5, 200 / (sr / 2), btype="high")


def filter_input(y: np.ndarray) -> np.ndarray:
    """what preprocess_audio hands to filtfilt: float32"""
    u = R.preemphasis(normalize(y), COEF)
    assert u.dtype == y.dtype
    return u


def highpass(u: np.ndarray, sr: int) -> np.ndarray:
    """the filter stage alone: scipy.signal.filtfilt with the experiment's filter (ValueError for len(u) <= 18)"""
    b, a = butter_ba(sr)
    return scipy.signal.filtfilt(b, a, u)


def preprocess_experiment(y: np.ndarray, sr: int):
    """the reference's preprocess_audio: float64, or None where the reference catches an exception"""
    try:
        return normalize(highpass(filter_input(y), sr))
    except Exception:
        return None


def conditioning(u: np.ndarray, sr: int) -> float:
    """max|sosfiltfilt(tf2sos(b, a), u, padlen=18) - filtfilt(b, a, u)| / max|filtfilt| on the filter input u"""
    b, a = butter_ba(sr)
    ref = scipy.signal.filtfilt(b, a, u)
    peak = float(np.max(np.abs(ref)))
    if peak == 0.0:
        return 0.0
    return float(np.max(np.abs(scipy.signal.sosfiltfilt(scipy.signal.tf2sos(b, a), u, padlen=PADLEN) - ref))) / peak


def bound(u: np.ndarray, sr: int) -> float:
    c = conditioning(u, sr)
    assert c <= MAX_CONDITIONING, (sr, u.size, c)
    return EPS32 + 4.0 * c


def shape_lengths(block: int, tile: int, p: int = PADLEN):
    """the lengths at which the block decomposition changes path: the shortest clips, either side of one block, of two
    blocks, of one tile (extended length = n + 2 p), and more than three tiles"""
    return (p + 1, p + 2, block - 2 * p - 1, block - 2 * p, block - 2 * p + 1, 2 * block - 2 * p + 1, tile - 2 * p,
            tile - 2 * p + 1, 3 * tile + 17)


def signal(n: int, sr: int, seed: int) -> np.ndarray:
    """white noise + 0.5 DC + a 50 Hz tone: a wrong carry leaks the DC the high-pass otherwise removes entirely"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    return (0.3 * rng.standard_normal(n) + 0.5 + 0.4 * np.sin(2 * np.pi * 50.0 * t)).astype(np.float32)


def to_s16(y: np.ndarray) -> np.ndarray:
    return np.clip(np.round(y * 8192.0), -32768, 32767).astype(np.int16)


def error_ratio(got: np.ndarray, ref: np.ndarray, u: np.ndarray, sr: int) -> float:
    """max|got - ref| over the reference's peak, as a fraction of the bound of the case"""
    peak = float(np.max(np.abs(ref)))
    assert peak > 0
    return float(np.max(np.abs(got.astype(np.float64) - ref))) / peak / bound(u, sr)
