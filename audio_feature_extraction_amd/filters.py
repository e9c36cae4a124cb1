"""Zero-phase IIR filtering on the GPU with ``scipy.signal.filtfilt`` semantics (odd extension, both passes started from
the step steady state), and the experiment extractor's ``preprocess_audio`` built on it
(04_feature_extraction_experiment/feature_extractor.py:133-154).

The passes run in ``libafx.so`` (``afx_sosfiltfilt_batch``) on cascaded second-order sections in float64; there is no CPU
fallback.  Signals are taken as float32 (what the extractors hold); results are float32.

Sections.  ``sosfiltfilt``, ``sosfiltfilt_batch`` and ``filtfilt`` accept any ``(n, 6)`` section array with ``n <= 4`` and
``a0 == 1`` -- scipy's own sections of any design (Butterworth, elliptic, Chebyshev), band-pass sections, gain-only and
first-order sections included -- and any ``padlen`` from 0 to 4096.  Only the designer ``butter_sos`` is
limited to low- and high-pass.

Smoothers.  ``medfilt`` and ``savgol_filter`` (and their ``_batch`` forms) are ``scipy.signal.medfilt`` (zero padding, odd
kernels up to 31; value-exact) and ``scipy.signal.savgol_filter(mode='interp')`` (odd windows 3 .. 31, order up to 5,
derivative up to 2; float64 chains of fused multiply-adds, one rounding to float32) on samples, in ``afx_medfilt_batch`` /
``afx_savgol_batch``.

Conditioning.  ``filtfilt(b, a, x)`` goes through ``scipy.signal.tf2sos``: the engine never runs the (b, a) recursion.  For
the high-pass filters of the extractors (200 Hz, order 5) the poles cluster near z = 1 and the float64 (b, a) recursion of
scipy is itself only defined to 3e-10 of the peak at 22.05 kHz and 7e-9 at 48 kHz (its distance from the same recursion in
long double); ``sosfiltfilt`` and ``filtfilt`` of scipy differ by up to 6e-10 at 16 / 22.05 kHz and 1e-7 at 48 kHz.  Results
here agree with scipy's ``sosfiltfilt`` to float64 rounding and with ``filtfilt`` to that distance.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from . import _native

_ctxs: dict = {}
_BTYPES = {"low": False, "lowpass": False, "lp": False, "high": True, "highpass": True, "hp": True}


def _ctx(device: int) -> _native.Context:
    c = _ctxs.get(device)
    if c is None:
        c = _ctxs[device] = _native.Context(device)
    return c


def butter_sos(order: int, wn: float, btype: str = "low") -> np.ndarray:
    """``scipy.signal.butter(order, wn, btype, output='sos')`` for ``btype`` 'low' / 'high' and orders 1 .. 8: the same
    filter as (order + 1) // 2 sections of unit pass-band gain each (scipy puts the whole gain into its first section and
    orders the sections differently; the cascade's response is the same).  Host only."""
    if not isinstance(btype, str) or btype.lower() not in _BTYPES:
        if isinstance(btype, str) and btype.lower() in ("band", "bandpass", "bp", "bs", "bandstop", "stop"):
            raise ValueError(f"btype={btype!r} is not supported (only 'low' and 'high')")
        raise ValueError("'%s' is an invalid bandtype for filter." % (btype,))
    if int(order) != order or order < 1:
        raise ValueError("Filter order must be a nonnegative integer")
    wn = float(np.asarray(wn, np.float64).reshape(()))
    if not 0.0 < wn < 1.0:
        raise ValueError("Digital filter critical frequencies must be 0 < Wn < 1")
    return _native.butter_sos(int(order), wn, _BTYPES[btype.lower()])


def _check_sos(sos) -> np.ndarray:
    sos = np.atleast_2d(np.asarray(sos, np.float64))
    if sos.ndim != 2 or sos.shape[1] != 6:
        raise ValueError("sos array must be shape (n_sections, 6)")
    if not (sos[:, 3] == 1).all():
        raise ValueError("sos[:, 3] should be all ones")
    if sos.shape[0] > 4:
        raise NotImplementedError("more than 4 sections (order 8) is not supported")
    return np.ascontiguousarray(sos)


def _default_padlen(sos: np.ndarray) -> int:
    # scipy.signal.sosfiltfilt: 3 * ntaps, ntaps less the trailing zeros both polynomials share
    ntaps = 2 * sos.shape[0] + 1
    ntaps -= min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum()))
    return 3 * ntaps


def _as_clip(x, what: str) -> np.ndarray:
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError(f"{what} must be 1-D (mono), got shape {x.shape}")
    return np.ascontiguousarray(x, np.float32)


def _run(clips: Sequence[np.ndarray], sos: np.ndarray, padlen: int, mode: int, preemph: float, device: int) -> dict:
    lengths = np.array([c.size for c in clips], np.int64)
    out = _ctx(device).sosfiltfilt_batch(np.concatenate(clips) if len(clips) else np.zeros(0, np.float32),
                                         _native.packed_offsets(lengths), lengths, sos, padlen, mode=mode, preemph=preemph)
    out["clips"] = [out["out"][o:o + n].copy() if st == _native.CLIP_OK else None
                    for o, n, st in zip(out["offsets"], lengths, out["status"])]
    return out


def sosfiltfilt_batch(sos, clips: Sequence[np.ndarray], padlen: Optional[int] = None, *, device: int = 0) -> List[Optional[np.ndarray]]:
    """``scipy.signal.sosfiltfilt(sos, x, padlen=padlen)`` of many mono clips in one device pass: a list of float32 arrays
    of their inputs' lengths, ``None`` for a clip scipy would refuse (no longer than ``padlen``, or not finite)."""
    sos = _check_sos(sos)
    padlen = _default_padlen(sos) if padlen is None else int(padlen)
    if padlen < 0:
        raise ValueError("padlen must be >= 0")
    cl = [_as_clip(c, f"clip {i}") for i, c in enumerate(clips)]
    if not cl:
        return []
    return _run(cl, sos, padlen, _native.FILT_PLAIN, 0.0, device)["clips"]


def sosfiltfilt(sos, x, padlen: Optional[int] = None, *, device: int = 0) -> np.ndarray:
    """``scipy.signal.sosfiltfilt(sos, x, padlen=padlen)`` (padtype 'odd') of one mono signal, float32."""
    sos = _check_sos(sos)
    padlen = _default_padlen(sos) if padlen is None else int(padlen)
    if padlen < 0:
        raise ValueError("padlen must be >= 0")
    x = _as_clip(x, "x")
    if x.size <= padlen:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
    y = _run([x], sos, padlen, _native.FILT_PLAIN, 0.0, device)["clips"][0]
    if y is None:
        raise ValueError("array must not contain infs or NaNs")
    return y


def filtfilt(b, a, x, padlen: Optional[int] = None, *, device: int = 0) -> np.ndarray:
    """``scipy.signal.filtfilt(b, a, x, padlen=padlen)`` (padtype 'odd') of one mono signal, float32.  The filter is
    converted by ``scipy.signal.tf2sos`` and run as a cascade: see the conditioning note of this module."""
    import scipy.signal
    b, a = np.atleast_1d(np.asarray(b, np.float64)), np.atleast_1d(np.asarray(a, np.float64))
    if b.ndim != 1 or a.ndim != 1 or a.size == 0 or a[0] == 0:
        raise ValueError("b and a must be 1-D and a[0] nonzero")
    if padlen is None:
        padlen = 3 * max(a.size, b.size)
    return sosfiltfilt(scipy.signal.tf2sos(b, a), x, padlen=padlen, device=device)


MAX_WINDOW, MAX_POLYORDER, MAX_DERIV = 31, 5, 2          # what afx_medfilt_batch / afx_savgol_batch compile in


def _check_kernel_size(kernel_size) -> int:
    k = np.asarray(kernel_size)
    if k.ndim > 1 or k.size != 1:
        raise ValueError("kernel_size must be a scalar (clips are one-dimensional)")
    k = int(k.reshape(()))
    if k < 1:
        raise ValueError("kernel_size must be positive")
    if k % 2 != 1:
        raise ValueError("Each element of kernel_size should be odd.")
    if k > MAX_WINDOW:
        raise NotImplementedError(f"kernel sizes above {MAX_WINDOW} are not supported")
    return k


def _smooth_clips(out: dict, lengths) -> List[Optional[np.ndarray]]:
    return [out["out"][o:o + n].copy() if st == _native.CLIP_OK else None
            for o, n, st in zip(out["offsets"], lengths, out["status"])]


def medfilt_batch(clips: Sequence[np.ndarray], kernel_size: int = 3, *, device: int = 0) -> List[Optional[np.ndarray]]:
    """``scipy.signal.medfilt(x, kernel_size)`` of many mono clips in one device pass: float32 arrays of their inputs'
    lengths (value-exact: every output is one of the inputs or the zero padding), ``None`` for an empty clip or one that is
    not finite."""
    k = _check_kernel_size(kernel_size)
    cl = [_as_clip(c, f"clip {i}") for i, c in enumerate(clips)]
    if not cl:
        return []
    lengths = np.array([c.size for c in cl], np.int64)
    return _smooth_clips(_ctx(device).medfilt_batch(np.concatenate(cl), _native.packed_offsets(lengths), lengths, k), lengths)


def medfilt(x, kernel_size: int = 3, *, device: int = 0) -> np.ndarray:
    """``scipy.signal.medfilt(x, kernel_size)`` of one mono signal (zero padding; odd ``kernel_size`` up to 31), float32."""
    k = _check_kernel_size(kernel_size)
    x = _as_clip(x, "x")
    if x.size == 0:
        return x.copy()
    y = medfilt_batch([x], k, device=device)[0]
    if y is None:
        raise ValueError("array must not contain infs or NaNs")
    return y


def _check_savgol(window_length, polyorder, deriv, delta, mode) -> tuple:
    if mode not in ("mirror", "constant", "nearest", "interp", "wrap"):
        raise ValueError("mode must be 'mirror', 'constant', 'nearest' 'wrap' or 'interp'.")
    if mode != "interp":
        raise NotImplementedError(f"mode={mode!r} is not supported (only 'interp')")
    w, p, d = int(window_length), int(polyorder), int(deriv)
    if w != window_length or p != polyorder or d != deriv:
        raise ValueError("window_length, polyorder and deriv must be integers")
    if w < 1:
        raise ValueError("window_length must be a positive integer")
    if p < 0 or d < 0:
        raise ValueError("polyorder and deriv must be nonnegative integers")
    if p >= w:
        raise ValueError("polyorder must be less than window_length.")
    delta = float(delta)
    if not np.isfinite(delta) or delta == 0.0:
        raise ValueError("delta must be finite and not 0")
    if w % 2 == 0 or w < 3 or w > MAX_WINDOW:
        raise NotImplementedError(f"window_length must be odd and in 3 .. {MAX_WINDOW}")
    if p > MAX_POLYORDER or d > MAX_DERIV:
        raise NotImplementedError(f"polyorder above {MAX_POLYORDER} or deriv above {MAX_DERIV} is not supported")
    return w, p, d, delta


def savgol_filter_batch(clips: Sequence[np.ndarray], window_length: int, polyorder: int, deriv: int = 0, delta: float = 1.0,
                        mode: str = "interp", *, device: int = 0) -> List[Optional[np.ndarray]]:
    """``scipy.signal.savgol_filter(x, window_length, polyorder, deriv, delta, mode='interp')`` of many mono clips in one
    device pass: the float32 samples widened to float64, results rounded once to float32; ``None`` for a clip scipy would
    refuse (shorter than the window) or one that is not finite."""
    w, p, d, delta = _check_savgol(window_length, polyorder, deriv, delta, mode)
    cl = [_as_clip(c, f"clip {i}") for i, c in enumerate(clips)]
    if not cl:
        return []
    lengths = np.array([c.size for c in cl], np.int64)
    return _smooth_clips(_ctx(device).savgol_batch(np.concatenate(cl), _native.packed_offsets(lengths), lengths, w, p, d, delta),
                         lengths)


def savgol_filter(x, window_length: int, polyorder: int, deriv: int = 0, delta: float = 1.0, mode: str = "interp", *,
                  device: int = 0) -> np.ndarray:
    """``scipy.signal.savgol_filter(x, window_length, polyorder, deriv=deriv, delta=delta, mode='interp')`` of one mono signal,
    float32 (odd ``window_length`` 3 .. 31, ``polyorder`` up to 5, ``deriv`` up to 2)."""
    w, p, d, delta = _check_savgol(window_length, polyorder, deriv, delta, mode)
    x = _as_clip(x, "x")
    if x.size < w:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    y = savgol_filter_batch([x], w, p, d, delta, device=device)[0]
    if y is None:
        raise ValueError("array must not contain infs or NaNs")
    return y


EXPERIMENT_COEF, EXPERIMENT_CUTOFF_HZ, EXPERIMENT_ORDER, EXPERIMENT_PADLEN = 0.98, 200.0, 5, 18


def _preprocess_experiment(signals: Sequence[np.ndarray], sr: int, device: int) -> dict:
    cl = [_as_clip(c, f"signal {i}") for i, c in enumerate(signals)]
    sos = butter_sos(EXPERIMENT_ORDER, EXPERIMENT_CUTOFF_HZ / (sr / 2), "high")
    return _run(cl, sos, EXPERIMENT_PADLEN, _native.FILT_EXPERIMENT, EXPERIMENT_COEF, device)


def preprocess_experiment_batch(signals: Sequence[np.ndarray], sr: int, *, device: int = 0) -> List[Optional[np.ndarray]]:
    """The experiment extractor's ``preprocess_audio`` of many mono signals at rate ``sr`` in one device pass: peak
    normalisation, pre-emphasis 0.98, the zero-phase 5th-order Butterworth high-pass at 200 Hz, peak normalisation;
    float32.  ``None`` for a clip the reference returns None for (18 samples or fewer, or not finite)."""
    if len(signals) == 0:
        return []
    return _preprocess_experiment(signals, sr, device)["clips"]
