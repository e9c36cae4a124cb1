"""``librosa.beat.beat_track`` on the GPU, as the reference's rhythm group calls it
(04_feature_extraction_experiment/feature_extractor.py:604-607): ``beat_track(onset_envelope=onset_env, sr=sr)`` at librosa's
defaults -- hop 512, tightness 100, trim -- with the tempo ``feature.tempo`` decides unless one is given.  The tracker is
Ellis's dynamic programme; ``tests/beat_ref.py`` restates what is computed, including the decisions where librosa is
undefined (one frame, or a cumulative score without a local maximum: no beats) and the beat-indexed trim.

Everything runs in ``libafx.so`` (``afx_beat_batch``); there is no CPU fallback.

``y=`` computes the envelope the reference feeds the tracker, ``onset.onset_strength(y, sr)`` (mean aggregate).  librosa's own
``beat_track(y=y)`` aggregates its envelope with the median instead; ours is ``beat_track(onset_envelope=onset_strength(y))``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import _native
from .effects import _as_signal
from .feature import _plan, _same

_DEFAULTS = {"hop_length": 512, "start_bpm": 120.0, "prior": None, "sparse": True}
_UNITS = ("frames", "samples", "time")


def _check_args(kwargs: dict, tightness, units) -> None:
    """Every librosa keyword other than tightness, trim, bpm and units must be at its default: nothing else is implemented."""
    for k, v in kwargs.items():
        if k not in _DEFAULTS:
            raise TypeError(f"unexpected keyword argument {k!r}")
        if not _same(v, _DEFAULTS[k]):
            raise ValueError(f"{k}={v!r} is not supported (only the default {_DEFAULTS[k]!r})")
    if units not in _UNITS:
        raise ValueError(f"units={units!r} must be one of {_UNITS}")
    if not (np.isscalar(tightness) and np.isfinite(tightness) and tightness > 0):
        raise ValueError(f"tightness={tightness!r} must be a positive number")


def _as_envelope(e, i: int) -> np.ndarray:
    e = np.asarray(e)
    if e.ndim != 1 or e.dtype.kind not in "fiu":
        raise ValueError(f"onset envelope {i} must be a one-dimensional real array")
    return np.ascontiguousarray(e, np.float32)


def _bpm_array(bpm, n: int):
    if bpm is None:
        return None
    b = np.asarray(bpm, np.float64)
    if b.ndim == 0:
        b = np.full(n, float(b))
    if b.shape != (n,):
        raise ValueError("bpm must be a scalar or one tempo per clip (time-varying tempo is not supported)")
    if not np.all(np.isfinite(b) & (b > 0)):
        raise ValueError("bpm must be finite and > 0")
    return b


def beat_track_batch(signals: Sequence[np.ndarray] = None, sr=22050, *, onset_envelopes: Sequence[np.ndarray] = None,
                     tightness=100, trim: bool = True, bpm=None, units: str = "frames", device: int = 0,
                     **kwargs) -> List[Tuple[np.ndarray, np.ndarray]]:
    """``beat_track`` of many mono signals, or of many onset envelopes, in one device pass: a list of (tempo, beats).
    ``bpm``: None (the tempo is decided per clip), a scalar, or one tempo per clip."""
    _check_args(kwargs, tightness, units)
    if (signals is None) == (onset_envelopes is None):
        raise ValueError("give either signals or onset_envelopes")
    env_mode = onset_envelopes is not None
    clips = [_as_envelope(e, i) for i, e in enumerate(onset_envelopes)] if env_mode else [_as_signal(s, i) for i, s in enumerate(signals)]
    if not clips:
        return []
    bpm = _bpm_array(bpm, len(clips))
    lengths = np.array([c.size for c in clips], np.int64)
    out = _plan(device, sr).beat_batch(np.concatenate(clips), _native.packed_offsets(lengths), lengths, envelopes=env_mode,
                                       bpm=bpm, tightness=float(tightness), trim=bool(trim))
    bad = np.flatnonzero(out["status"] != _native.CLIP_OK)
    if bad.size:
        raise ValueError(f"clip {int(bad[0])} status {int(out['status'][bad[0]])}")
    res = []
    for i, frames in enumerate(out["beats"]):
        if units == "samples":
            beats = frames * 512
        elif units == "time":
            beats = frames.astype(np.float64) * 512.0 / float(sr)
        else:
            beats = frames
        res.append((out["tempo"][i:i + 1].copy(), beats))
    return res


def beat_track(*, y=None, sr=22050, onset_envelope=None, hop_length=512, start_bpm=120.0, tightness=100, trim=True,
               bpm=None, prior=None, units="frames", sparse=True, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """``librosa.beat.beat_track(onset_envelope=onset_envelope, sr=sr)``, or with ``y=`` the same on
    ``onset.onset_strength(y, sr)`` -- NOT librosa's own ``y=`` path, which aggregates the envelope with the median; ours is
    ``beat_track(onset_envelope=onset_strength(y))``, what the reference extractor calls.  Returns ``(tempo, beats)``: tempo as
    ``feature.tempo`` returns it (float64, shape (1,); 0.0 for an all-zero envelope), beats as int64 frame or sample indices or
    float64 seconds (``units``).  ``hop_length``, ``start_bpm``, ``prior`` and ``sparse=False`` are refused off their defaults
    (ValueError); ``bpm`` is a scalar."""
    if (y is None) == (onset_envelope is None):
        raise ValueError("give either y or onset_envelope")
    if bpm is not None and not np.isscalar(bpm):
        raise ValueError("bpm must be a scalar (time-varying tempo is not supported)")
    kw = dict(hop_length=hop_length, start_bpm=start_bpm, prior=prior, sparse=sparse)
    if y is not None:
        return beat_track_batch([y], sr, tightness=tightness, trim=trim, bpm=bpm, units=units, device=device, **kw)[0]
    return beat_track_batch(None, sr, onset_envelopes=[onset_envelope], tightness=tightness, trim=trim, bpm=bpm, units=units,
                            device=device, **kw)[0]
