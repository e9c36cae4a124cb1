"""ITU-R BS.1770-4 integrated loudness and loudness / peak normalisation on the GPU, with the semantics of ``pyloudnorm``
0.1.x at the experiment's call sites (04_feature_extraction_experiment/process_audio.py:36-37, 57-61, 134-147;
feature_extraction.py:185-189): ``Meter(rate).integrated_loudness`` with K-weighting and 0.4 s blocks on mono audio,
``normalize.loudness`` and ``normalize.peak``.

The measure runs in ``libafx.so`` (``afx_loudness_batch``): the two K-weighting sections as a causal cascade in float64,
the gating blocks' sums of squares in float64, both gates in the linear domain; the final ``log10`` and the gain are host
double arithmetic.  There is no CPU fallback.  Signals are taken as float32 (what the extractors hold); normalised audio is
float32, one rounded product per sample (what numpy 1.24 gives for a float32 array times a Python float).

Deviations.  pyloudnorm rounds each filter stage to the array's dtype (float32 for a ``librosa.load`` array); the engine
does not, and differs from it by that rounding noise.  A clip without a level -- silence reads ``-inf`` -- comes
back unchanged from ``normalize_batch`` and ``normalize_volume`` (pyloudnorm multiplies by ``inf``).  Arrays of shape
``(n, channels)`` raise ``NotImplementedError``; rates from 4000 to 192000 Hz.
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native

_ctxs: dict = {}
REFERENCE_LEVEL = -23.0          # config/experiment_config.yaml:26


def _ctx(device: int) -> _native.Context:
    c = _ctxs.get(device)
    if c is None:
        c = _ctxs[device] = _native.Context(device)
    return c


def _as_clip(x, what: str) -> np.ndarray:
    x = np.asarray(x)
    if x.ndim == 2:
        raise NotImplementedError(f"{what}: only mono audio is supported, got shape {x.shape}")
    if x.ndim != 1:
        raise ValueError(f"{what} must be 1-D (mono), got shape {x.shape}")
    if not np.issubdtype(x.dtype, np.floating):
        raise ValueError("Data must be floating point.")
    return np.ascontiguousarray(x, np.float32)


def _check_meter(rate, block_size) -> Tuple[int, float]:
    if int(rate) != rate or rate < 1:
        raise ValueError("rate must be a positive integer")
    block_size = float(block_size)
    if not np.isfinite(block_size) or block_size <= 0.0:
        raise ValueError("block_size must be positive and finite")
    _native.loudness_blocks(0, int(rate), block_size)              # NotImplementedError outside the supported range
    return int(rate), block_size


def _pack(clips: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    lengths = np.array([c.size for c in clips], np.int64)
    offsets = _native.packed_offsets(lengths, 4)
    buf = np.zeros(int((offsets + lengths).max()) if len(clips) else 0, np.float32)
    for o, c in zip(offsets, clips):
        buf[o:o + c.size] = c
    return buf, offsets, lengths


def _batch(clips, rates, block_size, mode, target, want_blocks, device) -> dict:
    cl = [_as_clip(c, f"clip {i}") for i, c in enumerate(clips)]
    rates = np.broadcast_to(np.asarray(rates), (len(cl),))
    for r in np.unique(rates):
        _check_meter(r, block_size)
    buf, offsets, lengths = _pack(cl)
    out = _ctx(device).loudness_batch(buf, offsets, lengths, rates.astype(np.int32), block_size, mode, target,
                                      want_blocks=want_blocks)
    out["lengths"], out["in"] = lengths, cl
    return out


def _warn_clipped(peak_out: float) -> None:
    if peak_out >= 1.0:
        warnings.warn("Possible clipped samples in output.")


class Meter:
    """``pyloudnorm.Meter(rate, filter_class="K-weighting", block_size=0.400)`` for mono audio."""

    def __init__(self, rate: int, filter_class: str = "K-weighting", block_size: float = 0.400, *, device: int = 0):
        if filter_class != "K-weighting":
            raise NotImplementedError(f"filter_class={filter_class!r} is not supported (only 'K-weighting')")
        self.rate, self.block_size = _check_meter(rate, block_size)
        self.filter_class, self.device = filter_class, int(device)

    def integrated_loudness(self, data) -> float:
        """The gated loudness of ``data`` in LUFS (``-inf`` when no block passes the gates).  ``ValueError`` for audio
        shorter than a block, as pyloudnorm's, and for a NaN / inf sample."""
        return integrated_loudness(data, self.rate, self.block_size, device=self.device)


def integrated_loudness_batch(clips: Sequence[np.ndarray], rates, block_size: float = 0.400, *, device: int = 0) -> List[Optional[float]]:
    """``Meter(rate, block_size=block_size).integrated_loudness(clip)`` of many mono clips in one device pass; ``rates``: one
    rate for all, or one per clip.  ``None`` where pyloudnorm would raise (shorter than a block) and for a clip that is not
    finite."""
    if len(clips) == 0:
        return []
    out = _batch(clips, rates, block_size, _native.LOUD_MEASURE, 0.0, False, device)
    return [float(r[0]) if st == _native.CLIP_OK else None for r, st in zip(out["rec"], out["status"])]


def integrated_loudness(y, rate: int, block_size: float = 0.400, *, device: int = 0) -> float:
    """``pyloudnorm.Meter(rate, block_size=block_size).integrated_loudness(y)`` of one mono signal."""
    y = _as_clip(y, "data")
    rate, block_size = _check_meter(rate, block_size)
    if y.size < block_size * rate:
        raise ValueError("Audio must have length greater than the block size.")
    v = integrated_loudness_batch([y], rate, block_size, device=device)[0]
    if v is None:
        raise ValueError("array must not contain infs or NaNs")
    return v


def block_loudness(y, rate: int, block_size: float = 0.400, *, device: int = 0) -> np.ndarray:
    """The loudness of every gating block, ``l_j = -0.691 + 10 log10 z_j`` (float64; ``-inf`` for a silent block)."""
    y = _as_clip(y, "data")
    rate, block_size = _check_meter(rate, block_size)
    if y.size < block_size * rate:
        raise ValueError("Audio must have length greater than the block size.")
    out = _batch([y], rate, block_size, _native.LOUD_MEASURE, 0.0, True, device)
    if out["status"][0] != _native.CLIP_OK:
        raise ValueError("array must not contain infs or NaNs")
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(out["z"])


def normalize_loudness(y, input_loudness: float, target_loudness: float) -> np.ndarray:
    """``pyloudnorm.normalize.loudness(y, input_loudness, target_loudness)``: ``y`` times 10^((target - input) / 20).  An
    elementwise product of the caller's array in its own dtype -- host arithmetic, as there is nothing to measure; use
    :func:`normalize_batch` to measure and scale on the device in one call."""
    y = np.asarray(y)
    gain = np.power(10.0, (float(target_loudness) - float(input_loudness)) / 20.0)
    out = (y * y.dtype.type(gain)) if np.issubdtype(y.dtype, np.floating) else gain * y
    if out.size:
        _warn_clipped(float(np.max(np.abs(out))))
    return out


def normalize_peak(y, target_db: float, *, device: int = 0) -> np.ndarray:
    """``pyloudnorm.normalize.peak(y, target_db)`` of one mono signal on the device: float32, peak at ``target_db`` dB.
    A signal of zeros comes back unchanged."""
    y = _as_clip(y, "data")
    if y.size == 0:
        return y.copy()
    out = _batch([y], 48000, 0.400, _native.LOUD_NORM_PEAK, float(target_db), False, device)
    if out["status"][0] != _native.CLIP_OK:
        raise ValueError("array must not contain infs or NaNs")
    _warn_clipped(float(out["rec"][0][_native.LOUD_FIELDS.index("peak_out")]))
    return out["out"][out["offsets"][0]:out["offsets"][0] + y.size].copy()


def normalize_batch(clips: Sequence[np.ndarray], rates, target: float = REFERENCE_LEVEL, block_size: float = 0.400, *,
                    device: int = 0) -> Tuple[List[np.ndarray], List[Optional[float]]]:
    """Measures every mono clip and scales it to ``target`` LUFS in one call: ``(clips, loudness)``.  A clip pyloudnorm's
    meter would refuse (shorter than a block) or that is not finite comes back as a float32 copy of the input with loudness
    ``None`` -- the reference's ``normalize_volume`` keeps such audio as it is --, and so does, with loudness ``-inf``, a clip
    without a level."""
    if len(clips) == 0:
        return [], []
    out = _batch(clips, rates, block_size, _native.LOUD_NORM_LOUDNESS, float(target), False, device)
    ys, ls = [], []
    k_out = _native.LOUD_FIELDS.index("peak_out")
    for x, o, n, r, st in zip(out["in"], out["offsets"], out["lengths"], out["rec"], out["status"]):
        if st != _native.CLIP_OK:
            ys.append(x.copy()); ls.append(None)
            continue
        ys.append(out["out"][o:o + n].copy()); ls.append(float(r[0]))
        _warn_clipped(float(r[k_out]))
    return ys, ls
