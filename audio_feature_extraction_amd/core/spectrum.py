"""``librosa.stft`` / ``librosa.istft`` on the GPU at n_fft 1024 and 2048, with any hop in [1, n_fft], any window and both
of the padding modes the reference's own calls use (00_audio_data_collection_experiment/noise_reduction.py:31-84,
05_dtw_alignment_experiment/process_audio.py:21-33, visualization.py:194-208), in ``afx_stft_batch`` / ``afx_istft_batch``;
there is no CPU fallback.  DESIGN.md section 26 is the definition.

The spectrum comes back in librosa's own shape, dtype and memory order ([1 + n_fft / 2, T] complex64, every frame's bins
contiguous) without a transpose pass: the device writes frame after frame and the result is a view of that buffer.
``magphase``, ``amplitude_to_db`` and ``power_to_db`` are librosa's numpy helpers, here for the calls that follow a
transform.

``phase_vocoder`` is ``librosa.phase_vocoder`` on such a spectrum, in ``afx_pvoc_batch``: float32
magnitudes, float64 phases as a prefix sum in a fixed order.  ``effects.time_stretch`` is the whole stretch in one call.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import scipy.signal

from .. import _native

_ctxs: dict = {}


def _ctx(device: int) -> _native.Context:
    c = _ctxs.get(device)
    if c is None:
        c = _ctxs[device] = _native.Context(device)
    return c


def _window(window, win_length, n_fft: int) -> np.ndarray:
    """The float32 window of n_fft values: scipy's periodic window of win_length, or the caller's array, zero-padded centred
    as librosa.util.pad_center does."""
    win_length = n_fft if win_length is None else int(win_length)
    if not 1 <= win_length <= n_fft:
        raise NotImplementedError(f"win_length={win_length} is not supported (1 .. n_fft)")
    if isinstance(window, (str, tuple, float)):
        w = scipy.signal.get_window(window, win_length, fftbins=True)
    elif callable(window):
        w = np.asarray(window(win_length), np.float64)
    else:
        w = np.asarray(window, np.float64)
    if w.shape != (win_length,):
        raise ValueError(f"window must hold win_length = {win_length} values, got shape {w.shape}")
    lpad = (n_fft - win_length) // 2
    return np.pad(w, (lpad, n_fft - win_length - lpad)).astype(np.float32)


def _opts(n_fft, hop_length, win_length, center, pad_mode, out_kind=_native.STFT_COMPLEX) -> _native.StftOpts:
    n_fft = int(n_fft)
    if n_fft not in (1024, 2048):
        raise NotImplementedError(f"n_fft={n_fft} is not supported (1024, 2048)")
    win_length = n_fft if win_length is None else int(win_length)
    hop = win_length // 4 if hop_length is None else int(hop_length)
    if not 1 <= hop <= n_fft:
        raise NotImplementedError(f"hop_length={hop} is not supported (1 .. n_fft)")
    return _native.stft_opts(n_fft, hop, center, pad_mode, out_kind)


def _signal(y, i=None) -> np.ndarray:
    what = "y" if i is None else f"signal {i}"
    y = np.asarray(y)
    if y.ndim != 1:
        raise NotImplementedError(f"{what} must be 1-D (mono), got shape {y.shape}")
    return np.ascontiguousarray(y, np.int16 if y.dtype == np.int16 else np.float32)


_WHY = {_native.CLIP_TOO_SHORT: "is too short for this framing", _native.CLIP_NONFINITE: "is not finite everywhere"}


def _forward(signals, opts, window, device) -> list:
    sig = [_signal(s, i) for i, s in enumerate(signals)]
    if not sig:
        return []
    if len({s.dtype for s in sig}) > 1:
        sig = [s if s.dtype == np.float32 else s.astype(np.float32) / np.float32(32768.0) for s in sig]
    lengths = np.array([s.size for s in sig], np.int64)
    offsets = _native.packed_offsets(lengths, 4)
    buf = np.zeros(int((offsets + lengths).max()), sig[0].dtype)
    for o, s in zip(offsets, sig):
        buf[o:o + s.size] = s
    r = _ctx(device).stft_batch(buf, offsets, lengths, opts, window)
    return list(zip(r["spec"], r["status"]))


def stft_batch(signals: Sequence[np.ndarray], n_fft: int = 2048, hop_length: Optional[int] = None,
               win_length: Optional[int] = None, window="hann", center: bool = True, pad_mode: str = "constant",
               device: int = 0) -> List[Optional[np.ndarray]]:
    """``librosa.stft`` of many mono signals (float32, or int16 taken as value / 32768) in one device pass: per signal the
    complex64 [1 + n_fft / 2, T] spectrum, or None where the single call would raise (too short, not finite)."""
    opts = _opts(n_fft, hop_length, win_length, center, pad_mode)
    return [d if st == _native.CLIP_OK else None for d, st in _forward(signals, opts, _window(window, win_length, opts.n_fft), device)]


def stft(y, n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None, window="hann",
         center: bool = True, pad_mode: str = "constant", device: int = 0) -> np.ndarray:
    """``librosa.stft(y, ...)``: complex64 [1 + n_fft / 2, T] in librosa's memory order.  ValueError for a clip that is empty,
    too short for the framing (shorter than n_fft without ``center``, at most n_fft / 2 samples under reflect padding) or
    not finite, and for a ``pad_mode`` other than "constant" / "reflect"; NotImplementedError for any other n_fft, a hop or
    a win_length outside 1 .. n_fft."""
    opts = _opts(n_fft, hop_length, win_length, center, pad_mode)
    (d, st), = _forward([y], opts, _window(window, win_length, opts.n_fft), device)
    if st != _native.CLIP_OK:
        raise ValueError(f"stft: y {_WHY.get(int(st), 'failed')}")
    return d


def spectrogram(y, n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None, window="hann",
                center: bool = True, pad_mode: str = "constant", power: float = 1, device: int = 0) -> np.ndarray:
    """``abs(stft(y)) ** power`` for power 1 or 2, float32 [1 + n_fft / 2, T], taken on the device: half the bytes of the
    complex spectrum ever leave it."""
    if power not in (1, 2):
        raise NotImplementedError(f"power={power!r} is not supported (1, 2)")
    opts = _opts(n_fft, hop_length, win_length, center, pad_mode, _native.STFT_MAG if power == 1 else _native.STFT_POWER)
    (d, st), = _forward([y], opts, _window(window, win_length, opts.n_fft), device)
    if st != _native.CLIP_OK:
        raise ValueError(f"spectrogram: y {_WHY.get(int(st), 'failed')}")
    return d


def istft_batch(spectra: Sequence[np.ndarray], hop_length: Optional[int] = None, win_length: Optional[int] = None,
                n_fft: Optional[int] = None, window="hann", center: bool = True, length=None,
                device: int = 0) -> List[Optional[np.ndarray]]:
    """``librosa.istft`` of many spectra of one framing in one device pass (``length``: None, one value, or one per
    spectrum with None for none): float32 signals, None for a spectrum without frames."""
    specs = [np.asarray(D) for D in spectra]
    if not specs:
        return []
    for D in specs:
        if D.ndim != 2:
            raise NotImplementedError(f"a spectrum must be 2-D (mono), got shape {D.shape}")
    n_fft = 2 * (specs[0].shape[0] - 1) if n_fft is None else int(n_fft)
    opts = _opts(n_fft, hop_length, win_length, center, "constant")
    bins = n_fft // 2 + 1
    if any(D.shape[0] != bins for D in specs):
        raise ValueError(f"every spectrum must have 1 + n_fft / 2 = {bins} rows")
    if length is None or np.isscalar(length):
        length = [length] * len(specs)
    if len(length) != len(specs):
        raise ValueError("length must have one entry per spectrum")
    want = np.array([-1 if l is None else int(l) for l in length], np.int64)
    if np.any((want < 0) & np.array([l is not None for l in length])):
        raise ValueError("length must not be negative")
    frames = np.array([D.shape[1] for D in specs], np.int64)
    offsets = _native.packed_offsets(frames * bins)
    buf = np.zeros(int(frames.sum()) * bins, np.complex64)
    for o, D in zip(offsets, specs):
        # Fortran order is the device's layout: frame after frame.  librosa's own arrays are copied once, flat
        buf[o:o + D.size] = np.asfortranarray(D, np.complex64).ravel(order="F")
    r = _ctx(device).istft_batch(buf, offsets, frames, opts, _window(window, win_length, n_fft), lengths=want)
    return [r["out"][o:o + n].copy() if st == _native.CLIP_OK else None
            for o, n, st in zip(r["offsets"], r["samples"], r["status"])]


def istft(D, hop_length: Optional[int] = None, win_length: Optional[int] = None, n_fft: Optional[int] = None,
          window="hann", center: bool = True, length: Optional[int] = None, device: int = 0) -> np.ndarray:
    """``librosa.istft(D, ...)``: float32.  ``D`` may have any memory layout.  ValueError for a spectrum without frames."""
    y, = istft_batch([D], hop_length, win_length, n_fft, window, center, length, device)
    if y is None:
        raise ValueError("istft: D has no frames")
    return y


def _rate(rate, i=None) -> float:
    what = "rate" if i is None else f"rate {i}"
    rate = float(rate)
    if not (np.isfinite(rate) and rate > 0):
        raise ValueError(f"{what} must be finite and > 0, got {rate!r}")
    return rate


def _pvoc_framing(bins: int, hop_length, n_fft):
    n_fft = 2 * (bins - 1) if n_fft is None else int(n_fft)
    if n_fft < 2 or n_fft > 4096 or n_fft % 2:
        raise NotImplementedError(f"n_fft={n_fft} is not supported (even, 2 .. 4096)")
    hop = n_fft // 4 if hop_length is None else int(hop_length)
    if not 1 <= hop <= n_fft:
        raise NotImplementedError(f"hop_length={hop} is not supported (1 .. n_fft)")
    return n_fft, hop


def phase_vocoder_batch(spectra: Sequence[np.ndarray], rates, hop_length: Optional[int] = None, n_fft: Optional[int] = None,
                        device: int = 0) -> List[Optional[np.ndarray]]:
    """``librosa.phase_vocoder`` of many spectra of one framing in one device pass, spectrum i by ``rates[i]`` (or one rate
    for all): per spectrum the complex64 [1 + n_fft / 2, ceil(T / rate)] result, or None where the single call would raise
    (no frames, a NaN / inf bin)."""
    specs = [np.asarray(D) for D in spectra]
    rates = [rates] * len(specs) if np.isscalar(rates) else list(rates)
    if len(rates) != len(specs):
        raise ValueError("rates must have one entry per spectrum")
    rates = [_rate(r, i) for i, r in enumerate(rates)]
    if not specs:
        return []
    for D in specs:
        if D.ndim != 2:
            raise NotImplementedError(f"a spectrum must be 2-D (mono), got shape {D.shape}")
    n_fft, hop = _pvoc_framing(specs[0].shape[0], hop_length, n_fft)
    bins = n_fft // 2 + 1
    if any(D.shape[0] != bins for D in specs):
        raise ValueError(f"every spectrum must have 1 + n_fft / 2 = {bins} rows")
    frames = np.array([D.shape[1] for D in specs], np.int64)
    offsets = _native.packed_offsets(frames * bins)
    buf = np.zeros(max(int(frames.sum()) * bins, 1), np.complex64)
    for o, D in zip(offsets, specs):
        buf[o:o + D.size] = np.asfortranarray(D, np.complex64).ravel(order="F")
    r = _ctx(device).pvoc_batch(buf, offsets, frames, rates, n_fft, hop)
    return list(r["spec"])


def phase_vocoder(D, *, rate, hop_length: Optional[int] = None, n_fft: Optional[int] = None, device: int = 0) -> np.ndarray:
    """``librosa.phase_vocoder(D, rate=rate, hop_length=hop_length, n_fft=n_fft)``: complex64 [1 + n_fft / 2, ceil(T / rate)]
    in librosa's memory order.  ValueError for a rate that is not finite and > 0, a spectrum without frames, and -- where
    librosa lets the bin poison its row -- a NaN / inf bin; NotImplementedError for an odd n_fft, an n_fft beyond 4096 or a
    hop outside 1 .. n_fft."""
    rate = _rate(rate)
    P, = phase_vocoder_batch([D], [rate], hop_length, n_fft, device)
    if P is None:
        raise ValueError("phase_vocoder: D has no frames" if np.asarray(D).shape[1] == 0 else "phase_vocoder: D is not finite everywhere")
    return P


# ---- librosa's numpy helpers around a transform ---------------------------------------------------------------------------
def magphase(D, power: float = 1):
    """``librosa.magphase``: (abs(D) ** power, D / abs(D)) with a phase of 1 where D is 0."""
    D = np.asarray(D)
    mag = np.abs(D)
    zeros = mag == 0
    phase = np.exp(1.0j * np.angle(D + zeros.astype(mag.dtype))).astype(D.dtype if np.iscomplexobj(D) else np.complex64)
    return mag ** power, phase


def power_to_db(S, ref=1.0, amin: float = 1e-10, top_db: Optional[float] = 80.0) -> np.ndarray:
    """``librosa.power_to_db``: 10 log10(max(amin, S)) - 10 log10(max(amin, ref)), then floored at its maximum - top_db.
    ``ref`` is a number or a callable of the (magnitude of the) input, such as ``np.max``."""
    S = np.asarray(S)
    if amin <= 0:
        raise ValueError("amin must be strictly positive")
    magnitude = np.abs(S) if np.iscomplexobj(S) else S
    ref_value = ref(magnitude) if callable(ref) else np.abs(ref)
    log_spec = 10.0 * np.log10(np.maximum(amin, magnitude))
    log_spec = log_spec - 10.0 * np.log10(np.maximum(amin, ref_value))
    if top_db is not None:
        if top_db < 0:
            raise ValueError("top_db must be non-negative")
        log_spec = np.maximum(log_spec, log_spec.max() - top_db)
    return log_spec


def amplitude_to_db(S, ref=1.0, amin: float = 1e-5, top_db: Optional[float] = 80.0) -> np.ndarray:
    """``librosa.amplitude_to_db``: ``power_to_db(abs(S) ** 2, ref ** 2, amin ** 2, top_db)``."""
    magnitude = np.abs(np.asarray(S))
    ref_value = ref(magnitude) if callable(ref) else np.abs(ref)
    out_arr = magnitude if magnitude.dtype.kind == "f" else magnitude.astype(np.float64)
    return power_to_db(np.square(out_arr), ref=ref_value ** 2, amin=amin ** 2, top_db=top_db)
