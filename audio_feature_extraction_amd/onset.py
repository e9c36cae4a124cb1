"""``librosa.onset.onset_strength`` on the GPU, at librosa's defaults: the 128-band Slaney mel power of the 2048 / 512
periodic-Hann spectrogram in dB (``power_to_db`` with ref 1, top_db 80 over the clip), the rectified difference at lag 1, the
mean over the bands, three zeros in front (lag + n_fft // (2 hop)) and a cut to T = 1 + len // 512 frames -- the envelope the
reference's rhythm group starts from (04_feature_extraction_experiment/feature_extractor.py:592-622).

Everything runs in ``libafx.so`` (``afx_rhythm_batch``); there is no CPU fallback.  ``tests/rhythm_ref.py`` restates what is
computed.  Signals work from one sample up; the first three values are 0, so a signal of three frames or fewer gives zeros.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from . import _native
from .effects import _as_signal
from .feature import _plan, _same

_DEFAULTS = {"S": None, "lag": 1, "max_size": 1, "ref": None, "detrend": False, "center": True, "feature": None,
             "aggregate": None, "n_fft": 2048, "hop_length": 512, "n_mels": 128, "fmin": 0.0, "fmax": None,
             "htk": False, "window": "hann", "win_length": None, "pad_mode": "constant", "power": 2.0}


def _check_args(kwargs: dict) -> None:
    """Every librosa keyword must be at its default: nothing else is implemented."""
    for k, v in kwargs.items():
        if k not in _DEFAULTS:
            raise TypeError(f"unexpected keyword argument {k!r}")
        if not _same(v, _DEFAULTS[k]):
            raise ValueError(f"{k}={v!r} is not supported (only the default {_DEFAULTS[k]!r})")


def onset_strength_batch(signals: Sequence[np.ndarray], sr=22050, *, device: int = 0, **kwargs) -> List[np.ndarray]:
    """``librosa.onset.onset_strength`` of many mono signals in one device pass: a list of (T,) float32 envelopes."""
    _check_args(kwargs)
    sig = [_as_signal(s, i) for i, s in enumerate(signals)]
    if not sig:
        return []
    lengths = np.array([s.size for s in sig], np.int64)
    out = _plan(device, sr).rhythm_batch(np.concatenate(sig), _native.packed_offsets(lengths), lengths, want_stats=False)
    bad = np.flatnonzero(out["status"] != _native.CLIP_OK)
    if bad.size:
        raise ValueError(f"clip {int(bad[0])} status {int(out['status'][bad[0]])}")
    return [e.copy() for e in out["env"]]


def onset_strength(y, sr=22050, *, device: int = 0, **kwargs) -> np.ndarray:
    """``librosa.onset.onset_strength(y=y, sr=sr)``: (T,) float32."""
    return onset_strength_batch([y], sr, device=device, **kwargs)[0]
