"""``librosa.effects.hpss / harmonic / percussive`` on the GPU: harmonic-percussive separation at librosa 0.11's defaults
(kernel_size 31, power 2, margin 1) on the 2048 / 512 periodic-Hann STFT, the separation the reference's harmonic features
start from (04_feature_extraction_experiment/feature_extractor.py:525-556).

The STFT, both 31-tap median filters, the soft masks and the inverse STFT run in ``libafx.so`` (``afx_hpss_batch``); there
is no CPU fallback.  The time-axis median follows scipy's 'reflect' mirror repeated with period 2T for every clip of T
frames (scipy itself departs from it at T = 2, i.e. 512 .. 1023 samples).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import _native

_plans: dict = {}


def _plan(device: int) -> _native.Plan:
    pl = _plans.get(device)
    if pl is None:
        # sr does not enter the separation; the plan is librosa's 2048 / 512 Hann STFT
        pl = _plans[device] = _native.Plan(_native.Context(device), _native.make_params(22050, 2048, 512, 13, 128, "hann"))
    return pl


def _check_args(kernel_size, power, margin) -> None:
    if not (np.isscalar(kernel_size) and kernel_size == 31):
        raise ValueError(f"kernel_size={kernel_size!r} is not supported (only the default 31)")
    if not (np.isscalar(power) and power == 2.0):
        raise ValueError(f"power={power!r} is not supported (only the default 2.0)")
    if not (np.isscalar(margin) and margin == 1.0):
        raise ValueError(f"margin={margin!r} is not supported (only the default 1.0)")


def _as_signal(y, i=None) -> np.ndarray:
    what = "y" if i is None else f"signal {i}"
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError(f"{what} must be 1-D (mono), got shape {y.shape}")
    if y.size == 0:
        raise ValueError(f"{what} is empty")
    y = np.ascontiguousarray(y, np.float32)
    if not np.isfinite(y).all():
        raise ValueError(f"{what}: audio buffer is not finite everywhere")
    return y


def _run(signals: Sequence[np.ndarray], want_perc: bool, device: int) -> dict:
    lengths = np.array([s.size for s in signals], np.int64)
    out = _plan(device).hpss_batch(np.concatenate(signals), _native.packed_offsets(lengths), lengths, want_perc=want_perc, want_stats=False)
    bad = np.flatnonzero(out["status"] != _native.CLIP_OK)
    if bad.size:
        raise ValueError(f"hpss: clip {int(bad[0])} status {int(out['status'][bad[0]])}")
    return out


def hpss_batch(signals: Sequence[np.ndarray], *, kernel_size=31, power=2.0, margin=1.0,
               device: int = 0) -> List[Tuple[np.ndarray, np.ndarray]]:
    """``librosa.effects.hpss`` of many mono signals in one device pass: a list of (harmonic, percussive) float32 pairs,
    each of its input's length."""
    _check_args(kernel_size, power, margin)
    sig = [_as_signal(s, i) for i, s in enumerate(signals)]
    if not sig:
        return []
    out = _run(sig, True, device)
    return [(h.copy(), p.copy()) for h, p in zip(out["harm"], out["perc"])]


def hpss(y, *, kernel_size=31, power=2.0, margin=1.0, device: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """``librosa.effects.hpss(y)``: (harmonic, percussive), float32, of ``y``'s length."""
    return hpss_batch([y], kernel_size=kernel_size, power=power, margin=margin, device=device)[0]


def harmonic(y, *, kernel_size=31, power=2.0, margin=1.0, device: int = 0) -> np.ndarray:
    """``librosa.effects.harmonic(y)``: the harmonic part, float32, of ``y``'s length."""
    _check_args(kernel_size, power, margin)
    return _run([_as_signal(y)], False, device)["harm"][0].copy()


def percussive(y, *, kernel_size=31, power=2.0, margin=1.0, device: int = 0) -> np.ndarray:
    """``librosa.effects.percussive(y)``: the percussive part, float32, of ``y``'s length."""
    return hpss(y, kernel_size=kernel_size, power=power, margin=margin, device=device)[1]
