"""``librosa.feature.chroma_stft`` / ``melspectrogram`` and ``librosa.estimate_tuning`` on the GPU, at librosa's defaults:
the 2048 / 512 periodic-Hann power spectrogram, piptrack's peaks (150 .. 4000 Hz, threshold 0.1) and the 0.01-semitone tuning
histogram, the 12-class filterbank (ctroct 5, octwidth 2, base C) with max-normalised frames, and the 128-band Slaney mel
power -- the matrices the reference's timbre group starts from
(04_feature_extraction_experiment/feature_extractor.py:558-590).

``tempogram`` / ``tempo`` are ``librosa.feature.tempogram`` and ``librosa.feature.tempo`` as ``librosa.beat.beat_track`` calls
them on ``librosa.onset.onset_strength(y, sr)``: an autocorrelation window of ``int(8 sr) // 512`` frames (344 at 22050 Hz, not
``tempogram``'s own default of 384), the log-normal prior round 120 bpm, no tempo above 320 bpm -- what the reference's rhythm
group reads (04_feature_extraction_experiment/feature_extractor.py:592-622).

Everything runs in ``libafx.so`` (``afx_chroma_batch``, ``afx_rhythm_batch``); there is no CPU fallback.
``tests/chroma_ref.py`` and ``tests/rhythm_ref.py`` restate what is computed.  Signals work from one sample up
(T = 1 + len // 512 frames).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import _native
from .effects import _as_signal

_plans: dict = {}

_DEFAULTS = {"n_fft": 2048, "hop_length": 512, "win_length": None, "window": "hann", "center": True, "pad_mode": "constant",
             "S": None, "norm": np.inf, "n_chroma": 12, "power": 2.0, "n_mels": 128, "fmin": 0.0, "fmax": None,
             "htk": False, "resolution": 0.01, "bins_per_octave": 12, "ctroct": 5.0, "octwidth": 2, "base_c": True}


def _plan(device: int, sr) -> _native.Plan:
    if not (np.isscalar(sr) and float(sr) == int(sr) and int(sr) > 0):
        raise ValueError(f"sr={sr!r} must be a positive integer")
    key = (device, int(sr))
    pl = _plans.get(key)
    if pl is None:
        pl = _plans[key] = _native.Plan(_native.Context(device), _native.make_params(int(sr), 2048, 512, 13, 128, "hann"))
    return pl


def _same(v, d) -> bool:
    if d is None or isinstance(d, (str, bool)):
        return type(v) is type(d) and v == d
    return bool(np.isscalar(v)) and not isinstance(v, (str, bool)) and v == d


def _check_args(kwargs: dict) -> None:
    """Every librosa keyword must be at its default: nothing else is implemented."""
    for k, v in kwargs.items():
        if k not in _DEFAULTS:
            raise TypeError(f"unexpected keyword argument {k!r}")
        if not _same(v, _DEFAULTS[k]):
            raise ValueError(f"{k}={v!r} is not supported (only the default {_DEFAULTS[k]!r})")


def _tunings(tuning, n: int) -> Optional[np.ndarray]:
    if tuning is None:
        return None
    t = np.asarray(tuning, np.float64)
    if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != n) or not np.isfinite(t).all():
        raise ValueError("tuning must be None, a finite scalar or one finite value per signal")
    return np.broadcast_to(t, (n,))


def _run(signals: Sequence[np.ndarray], sr, device: int, **want) -> dict:
    lengths = np.array([s.size for s in signals], np.int64)
    out = _plan(device, sr).chroma_batch(np.concatenate(signals), _native.packed_offsets(lengths), lengths, want_stats=False, **want)
    bad = np.flatnonzero(out["status"] != _native.CLIP_OK)
    if bad.size:
        raise ValueError(f"clip {int(bad[0])} status {int(out['status'][bad[0]])}")
    return out


def chroma_stft_batch(signals: Sequence[np.ndarray], sr=22050, *, tuning=None, device: int = 0, **kwargs) -> List[np.ndarray]:
    """``librosa.feature.chroma_stft`` of many mono signals in one device pass: a list of [12, T] float32 matrices.
    ``tuning``: None (estimated per signal, as librosa does), a scalar, or one value per signal."""
    _check_args(kwargs)
    sig = [_as_signal(s, i) for i, s in enumerate(signals)]
    if not sig:
        return []
    return [c.copy() for c in _run(sig, sr, device, tuning=_tunings(tuning, len(sig)))["chroma"]]


def chroma_stft(y, sr=22050, *, tuning=None, device: int = 0, **kwargs) -> np.ndarray:
    """``librosa.feature.chroma_stft(y=y, sr=sr, tuning=tuning)``: [12, T] float32, every frame scaled to maximum 1."""
    return chroma_stft_batch([y], sr, tuning=tuning, device=device, **kwargs)[0]


def melspectrogram_batch(signals: Sequence[np.ndarray], sr=22050, *, device: int = 0, **kwargs) -> List[np.ndarray]:
    """``librosa.feature.melspectrogram`` of many mono signals in one device pass: a list of [128, T] float32 matrices."""
    _check_args(kwargs)
    sig = [_as_signal(s, i) for i, s in enumerate(signals)]
    if not sig:
        return []
    return [m.copy() for m in _run(sig, sr, device, tuning=0.0, want_chroma=False, want_mel=True)["mel"]]


def melspectrogram(y, sr=22050, *, device: int = 0, **kwargs) -> np.ndarray:
    """``librosa.feature.melspectrogram(y=y, sr=sr)``: [128, T] float32 mel power."""
    return melspectrogram_batch([y], sr, device=device, **kwargs)[0]


def estimate_tuning(y, sr=22050, *, device: int = 0, **kwargs) -> float:
    """``librosa.estimate_tuning(y=y, sr=sr)``: the deviation from A440 in fractions of a semitone, one of -0.5 + 0.01 k."""
    _check_args(kwargs)
    return float(_run([_as_signal(y)], sr, device, want_chroma=False)["tuning"][0])


# ---- tempogram / tempo (afx_rhythm_batch) ---------------------------------------------------------------------------
_RHYTHM_DEFAULTS = {"onset_envelope": None, "hop_length": 512, "win_length": None, "center": True, "window": "hann",
                    "norm": np.inf, "tg": None, "start_bpm": 120, "std_bpm": 1.0, "ac_size": 8.0, "max_tempo": 320.0,
                    "prior": None}


def _check_rhythm_args(kwargs: dict) -> None:
    """Every librosa keyword must be at the value beat_track gives it: nothing else is implemented (``win_length`` None
    stands for int(8 sr) // 512; a caller-supplied ``onset_envelope`` / ``tg`` is not supported)."""
    for k, v in kwargs.items():
        if k not in _RHYTHM_DEFAULTS:
            raise TypeError(f"unexpected keyword argument {k!r}")
        if not _same(v, _RHYTHM_DEFAULTS[k]):
            raise ValueError(f"{k}={v!r} is not supported (only the default {_RHYTHM_DEFAULTS[k]!r})")


def _run_rhythm(signals, sr, device: int, **want) -> dict:
    sig = [_as_signal(s, i) for i, s in enumerate(signals)]
    lengths = np.array([s.size for s in sig], np.int64)
    out = _plan(device, sr).rhythm_batch(np.concatenate(sig), _native.packed_offsets(lengths), lengths, want_stats=False, **want)
    bad = np.flatnonzero(out["status"] != _native.CLIP_OK)
    if bad.size:
        raise ValueError(f"clip {int(bad[0])} status {int(out['status'][bad[0]])}")
    return out


def tempogram_batch(signals: Sequence[np.ndarray], sr=22050, *, device: int = 0, **kwargs) -> List[np.ndarray]:
    """The autocorrelation tempogram of many mono signals in one device pass: a list of [int(8 sr) // 512, T] float32."""
    _check_rhythm_args(kwargs)
    if not len(signals):
        return []
    return [t.copy() for t in _run_rhythm(signals, sr, device, want_env=False, want_tempogram=True)["tempogram"]]


def tempogram(y=None, sr=22050, onset_envelope=None, *, device: int = 0, **kwargs) -> np.ndarray:
    """``librosa.feature.tempogram(onset_envelope=librosa.onset.onset_strength(y=y, sr=sr), sr=sr, win_length=int(8 sr) //
    512)``: [win, T] float32, every frame divided by its largest magnitude (lag 0 of a non-zero frame is 1)."""
    if onset_envelope is not None or y is None:
        raise ValueError("onset_envelope= is not supported (only y: the envelope is computed on the device)")
    return tempogram_batch([y], sr, device=device, **kwargs)[0]


def tempo_batch(signals: Sequence[np.ndarray], sr=22050, *, device: int = 0, **kwargs) -> np.ndarray:
    """The tempo of many mono signals in one device pass: float64 [n] (0.0 for a signal whose onset envelope is all zero)."""
    _check_rhythm_args(kwargs)
    if not len(signals):
        return np.zeros(0, np.float64)
    return _run_rhythm(signals, sr, device, want_env=False)["tempo"].copy()


def tempo(y=None, sr=22050, onset_envelope=None, *, device: int = 0, **kwargs) -> np.ndarray:
    """The tempo ``librosa.beat.beat_track(onset_envelope=librosa.onset.onset_strength(y=y, sr=sr), sr=sr)`` returns --
    ``librosa.feature.tempo(..., ac_size=8.0, max_tempo=320)``, 0.0 for an all-zero envelope -- as a float64 array of shape
    (1,), as librosa >= 0.10 does.  One arg-max decides it: see DESIGN.md 6."""
    if onset_envelope is not None or y is None:
        raise ValueError("onset_envelope= is not supported (only y: the envelope is computed on the device)")
    return tempo_batch([y], sr, device=device, **kwargs)
