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
import collections.abc
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


# ---- any sections, any padlen: the cases the filter tests share beyond the experiment's 5th-order high-pass ---------------
# The reference is scipy.signal.sosfiltfilt itself.  Sections in general have no well-conditioned (b, a) form, so the
# reference's indeterminacy is measured between two float64 evaluations of the same linear filter that scipy offers for any
# sections: the cascade in its given order and in the reverse order.  The bound keeps the formula of the module docstring.

SHAPE_SR = 22050                                        # only names the tone of signal(): the filters are given by Wn
SHAPE_PADLENS = (0, 1, 18, 63, 64, 65, 2048, 4095, 4096)
SHAPE_FILTER_SECTIONS = {                               # name -> section count (the kernels' template argument)
    "hp1_200hz_22k": 1, "lp2_0.1": 1,
    "lp3_0.1": 2, "hp4_80hz_48k": 2, "ellip4_0.2": 2, "band2_0.1_0.3": 2,
    "lp6_0.25": 3, "cheby2_5_hp_0.05": 3, "gain_lp4_0.1": 3,
    "hp7_0.02": 4, "lp8_0.05": 4, "lp8_0.01": 4, "hp8_200hz_48k": 4, "scipy_lp8_0.05": 4, "gain2_lp4_0.1": 4,
}
EXPERIMENT_PAIRS = (("hp1_200hz_22k", 2048), ("lp8_0.05", 4096))   # experiment mode on other filters: S = 1 and S = 4


def _gain(g: float) -> np.ndarray:
    return np.array([[g, 0.0, 0.0, 1.0, 0.0, 0.0]])


@functools.lru_cache(maxsize=None)
def _shape_filter(name: str) -> np.ndarray:
    from audio_feature_extraction_amd import _native as N
    own = {"hp1_200hz_22k": (1, 200 / 11025, True), "lp2_0.1": (2, 0.1, False), "lp3_0.1": (3, 0.1, False),
           "hp4_80hz_48k": (4, 80 / 24000, True), "lp6_0.25": (6, 0.25, False), "hp7_0.02": (7, 0.02, True),
           "lp8_0.05": (8, 0.05, False), "lp8_0.01": (8, 0.01, False), "hp8_200hz_48k": (8, 200 / 24000, True)}
    if name in own:
        sos = N.butter_sos(*own[name])
    elif name == "ellip4_0.2":                          # zeros on the unit circle: b2 != 0 with b1 != -2 b0
        sos = scipy.signal.ellip(4, 0.5, 60, 0.2, output="sos")
    elif name == "band2_0.1_0.3":
        sos = scipy.signal.butter(2, [0.1, 0.3], "band", output="sos")
    elif name == "cheby2_5_hp_0.05":
        sos = scipy.signal.cheby2(5, 40, 0.05, "high", output="sos")
    elif name == "scipy_lp8_0.05":                      # the whole gain in the first section, scipy's order
        sos = scipy.signal.butter(8, 0.05, output="sos")
    elif name == "gain_lp4_0.1":                        # a gain-only section [g, 0, 0, 1, 0, 0] in front
        sos = np.concatenate([_gain(0.75), N.butter_sos(4, 0.1, False)])
    elif name == "gain2_lp4_0.1":
        sos = np.concatenate([_gain(1.5), _gain(0.5), N.butter_sos(4, 0.1, False)])
    else:
        raise KeyError(name)
    sos = np.ascontiguousarray(sos, np.float64)
    assert sos.shape == (SHAPE_FILTER_SECTIONS[name], 6), (name, sos.shape)
    sos.setflags(write=False)
    return sos


class _ShapeFilters(collections.abc.Mapping):
    """name -> sections, built when first asked for (the project's own come from the built library)"""

    def __getitem__(self, name):
        return _shape_filter(name)

    def __iter__(self):
        return iter(SHAPE_FILTER_SECTIONS)

    def __len__(self):
        return len(SHAPE_FILTER_SECTIONS)


SHAPE_FILTERS = _ShapeFilters()


def shape_lengths_general(block: int, tile: int, p: int):
    """shape_lengths at padlen p, and the lengths either side of one and of two tiles that it leaves out; only clips the
    filter takes (n > p) of at least two samples.  With p = tile the first tile of every clip is extension only."""
    ns = shape_lengths(block, tile, p) + (tile - 2 * p - 1, 2 * tile - 2 * p, 2 * tile - 2 * p + 1)
    return tuple(dict.fromkeys(n for n in ns if n > max(p, 1)))


@functools.lru_cache(maxsize=None)
def shape_clip(name: str, p: int, n: int) -> np.ndarray:
    """the clip of one case: signal() with a seed of the case's own"""
    seed = 1000 * list(SHAPE_FILTER_SECTIONS).index(name) + 37 * SHAPE_PADLENS.index(p) + n % 997
    y = signal(n, SHAPE_SR, seed)
    y.setflags(write=False)
    return y


def sos_reference(sos: np.ndarray, u: np.ndarray, padlen: int) -> np.ndarray:
    """scipy.signal.sosfiltfilt on the float32 u: the odd extension in float32, the passes in float64 (what filt_e restates)"""
    assert u.dtype == np.float32
    return scipy.signal.sosfiltfilt(np.array(sos, np.float64), u, padlen=padlen)     # a writable copy: scipy refuses others


def sos_conditioning(sos: np.ndarray, u: np.ndarray, padlen: int) -> float:
    """max|sosfiltfilt(sos) - sosfiltfilt(sos[::-1])| / max|sosfiltfilt(sos)|: exactly 0 for one section"""
    ref = sos_reference(sos, u, padlen)
    peak = float(np.max(np.abs(ref)))
    assert peak > 0
    return float(np.max(np.abs(sos_reference(np.ascontiguousarray(sos[::-1]), u, padlen) - ref))) / peak


def sos_bound(sos: np.ndarray, u: np.ndarray, padlen: int) -> float:
    c = sos_conditioning(sos, u, padlen)
    assert c <= MAX_CONDITIONING, (u.size, padlen, c)
    return EPS32 + 4.0 * c


@functools.lru_cache(maxsize=None)
def shape_case(name: str, p: int, n: int):
    """(reference, bound) of one case: computed once, shared, never modified"""
    sos, u = SHAPE_FILTERS[name], shape_clip(name, p, n)
    ref = sos_reference(sos, u, p)
    ref.setflags(write=False)
    return ref, sos_bound(sos, u, p)


def sos_error_ratio(got: np.ndarray, ref: np.ndarray, bnd: float) -> float:
    """max|got - ref| over the reference's peak, as a fraction of the bound"""
    peak = float(np.max(np.abs(ref)))
    assert peak > 0
    return float(np.max(np.abs(got.astype(np.float64) - ref))) / peak / bnd
