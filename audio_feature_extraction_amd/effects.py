"""``librosa.effects.hpss / harmonic / percussive`` on the GPU: harmonic-percussive separation at librosa 0.11's defaults
(kernel_size 31, power 2, margin 1) on the 2048 / 512 periodic-Hann STFT, the separation the reference's harmonic features
start from (04_feature_extraction_experiment/feature_extractor.py:525-556).

The STFT, both 31-tap median filters, the soft masks and the inverse STFT run in ``libafx.so`` (``afx_hpss_batch``); there
is no CPU fallback.  The time-axis median follows scipy's 'reflect' mirror repeated with period 2T for every clip of T
frames (scipy itself departs from it at T = 2, i.e. 512 .. 1023 samples).

On the same STFT, the reference's STFT-domain noise reducers (00_audio_data_collection_experiment/noise_reduction.py:15-92:
``spectral_subtraction``, ``wiener_filter``) and the signal conditioning in front of its DTW aligner
(05_dtw_alignment_experiment/process_audio.py:9-54: ``preprocess_alignment``), all in ``afx_denoise_batch``.

On scipy's STFT at 1024 / 256 or 2048 / 512, ``noisereduce.reduce_noise`` as the experiment's audio processor calls it
(04_feature_extraction_experiment/process_audio.py:82-98): ``reduce_noise``, in ``afx_gate_batch``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

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


# ---- STFT-domain noise reduction (afx_denoise_batch) ------------------------------------------------------------------
def _sr_plan(device: int, sr: int) -> _native.Plan:
    """the 2048 / 512 Hann plan at ``sr`` (the energy VAD frames the signal by the sample rate)"""
    if int(sr) == 22050:
        return _plan(device)
    pl = _plans.get((device, int(sr)))
    if pl is None:
        pl = _plans[(device, int(sr))] = _native.Plan(_native.Context(device), _native.make_params(int(sr), 2048, 512, 13, 128, "hann"))
    return pl


def _check_framing(frame_length, hop_length) -> None:
    if frame_length != 2048 or hop_length != 512:
        raise NotImplementedError(f"frame_length={frame_length!r}, hop_length={hop_length!r} is not supported (only 2048 / 512)")


def _mono_f32(signals) -> List[np.ndarray]:
    sig = [np.ascontiguousarray(s, np.float32) for s in signals]
    for i, y in enumerate(sig):
        if y.ndim != 1:
            raise ValueError(f"signal {i} must be 1-D (mono), got shape {y.shape}")
    return sig


def _denoise(sig: List[np.ndarray], sr: int, device: int, **kw) -> dict:
    lengths = np.array([s.size for s in sig], np.int64)
    y = np.concatenate(sig) if sig else np.zeros(0, np.float32)
    return _sr_plan(device, sr).denoise_batch(y, _native.packed_offsets(lengths), lengths, **kw)


def _reduce(who: str, signals, sr, frame_length, hop_length, device, mode, beta, noise_frames) -> List[np.ndarray]:
    _check_framing(frame_length, hop_length)
    pr = _native.make_params(int(sr), 2048, 512, 13, 128, "hann")
    _native.denoise_check(pr, 0, mode, beta, noise_frames)           # before any device is touched
    sig = _mono_f32(signals)
    if not sig:
        return []
    out = _denoise(sig, sr, device, mode=mode, beta=beta, noise_frames=noise_frames)
    bad = np.flatnonzero(out["status"] != _native.CLIP_OK)
    if bad.size:
        what = "is empty" if out["status"][bad[0]] == _native.CLIP_TOO_SHORT else "is not finite everywhere"
        raise ValueError(f"{who}: signal {int(bad[0])} {what}")
    return [o.copy() for o in out["out"]]


def spectral_subtraction_batch(signals: Sequence[np.ndarray], sr: int = 22050, *, frame_length: int = 2048, hop_length: int = 512,
                               beta: float = 0.01, noise_frames: int = 10, device: int = 0) -> List[np.ndarray]:
    """``spectral_subtraction`` of many mono signals in one device pass."""
    return _reduce("spectral_subtraction", signals, sr, frame_length, hop_length, device, _native.DENOISE_SPECSUB, beta, noise_frames)


def spectral_subtraction(y, sr: int = 22050, *, frame_length: int = 2048, hop_length: int = 512, beta: float = 0.01,
                         noise_frames: int = 10, device: int = 0) -> np.ndarray:
    """The reference's ``NoiseReducer.spectral_subtraction``: |X| - beta N clamped at zero with X's phase, N the mean
    magnitude of the first ``noise_frames`` frames; float32 of ``y``'s length (zero from 512 (len // 512) on)."""
    return spectral_subtraction_batch([y], sr, frame_length=frame_length, hop_length=hop_length, beta=beta,
                                      noise_frames=noise_frames, device=device)[0]


def wiener_filter_batch(signals: Sequence[np.ndarray], sr: int = 22050, *, frame_length: int = 2048, hop_length: int = 512,
                        noise_frames: int = 10, device: int = 0) -> List[np.ndarray]:
    """``wiener_filter`` of many mono signals in one device pass."""
    return _reduce("wiener_filter", signals, sr, frame_length, hop_length, device, _native.DENOISE_WIENER, 0.0, noise_frames)


def wiener_filter(y, sr: int = 22050, *, frame_length: int = 2048, hop_length: int = 512, noise_frames: int = 10,
                  device: int = 0) -> np.ndarray:
    """The reference's ``NoiseReducer.wiener_filter``: X P / (P + Np + eps), Np the mean power of the first
    ``noise_frames`` frames; float32 of ``y``'s length (zero from 512 (len // 512) on)."""
    return wiener_filter_batch([y], sr, frame_length=frame_length, hop_length=hop_length, noise_frames=noise_frames,
                               device=device)[0]


def _preprocess_alignment(signals, sr: int, device: int) -> dict:
    pr = _native.make_params(int(sr), 2048, 512, 13, 128, "hann")
    _native.denoise_check(pr, _native.DENOISE_RMS_GAIN | _native.DENOISE_VAD, _native.DENOISE_SPECSUB, 1.0, 10)
    return _denoise(_mono_f32(signals), sr, device, mode=_native.DENOISE_SPECSUB, beta=1.0, noise_frames=10, rms_gain=True, vad=True)


def preprocess_alignment_batch(signals: Sequence[np.ndarray], sr: int, *, device: int = 0) -> List[Optional[np.ndarray]]:
    """``preprocess_alignment`` of many signals in one device pass; ``None`` for a clip that cannot be processed (fewer than
    512 samples, or a NaN / inf sample)."""
    if not len(signals):
        return []
    out = _preprocess_alignment(signals, sr, device)
    return [o[:512 * (o.size // 512)].copy() if st == _native.CLIP_OK else None for o, st in zip(out["out"], out["status"])]


def preprocess_alignment(y, sr: int, *, device: int = 0) -> np.ndarray:
    """The conditioning the reference's DTW aligner gives every recording (process_audio.py:13-51): gain to RMS 0.1,
    spectral subtraction of the whole noise profile (beta 1, 10 frames), then an energy VAD at 25 ms / 10 ms that zeroes
    everything outside its speech frames.  float32 of 512 (len // 512) samples, what the reference writes to disk.  Raises
    ``ValueError`` where the batch form gives ``None``."""
    out = _preprocess_alignment([y], sr, device)
    st = int(out["status"][0])
    if st != _native.CLIP_OK:
        raise ValueError("preprocess_alignment: " + ("fewer than 512 samples" if st == _native.CLIP_TOO_SHORT else "audio buffer is not finite everywhere"))
    o = out["out"][0]
    return o[:512 * (o.size // 512)].copy()


# ---- spectral gating (afx_gate_batch): noisereduce.reduce_noise ----------------------------------------------------------
_ctxs: dict = {}
_GATE_KEYS = ("stationary", "prop_decrease", "time_constant_s", "freq_mask_smooth_hz", "time_mask_smooth_ms",
              "thresh_n_mult_nonstationary", "sigmoid_slope_nonstationary", "n_std_thresh_stationary", "chunk_size", "padding",
              "n_fft", "win_length", "hop_length", "clip_noise_stationary")


def _ctx(device: int) -> _native.Context:
    c = _ctxs.get(device)
    if c is None:
        c = _ctxs[device] = _native.Context(device)
    return c


def _gate_opts(sr, kw: dict) -> _native.GateOpts:
    """noisereduce's keywords as the engine's record, checked without a device: the keywords the engine does not honour
    raise ``NotImplementedError`` by name, what noisereduce refuses raises ``ValueError``."""
    if kw.pop("use_torch", False):
        raise NotImplementedError("use_torch=True is not supported")
    if kw.pop("use_tqdm", False):
        raise NotImplementedError("use_tqdm=True is not supported")
    if kw.pop("n_jobs", 1) != 1:
        raise NotImplementedError("n_jobs != 1 is not supported: a batch is one device pass (reduce_noise_batch)")
    if kw.pop("tmp_folder", None) is not None:
        raise NotImplementedError("tmp_folder is not supported: nothing is spilled to disk")
    kw.pop("device", None)                                            # noisereduce's torch device
    unknown = sorted(set(kw) - set(_GATE_KEYS))
    if unknown:
        raise TypeError(f"reduce_noise: unexpected keyword {unknown[0]!r}")
    if int(sr) != sr or sr < 1:
        raise ValueError("sr must be a positive integer")
    n_fft = kw.get("n_fft", 1024)
    win = kw.get("win_length") or n_fft
    hop = kw.get("hop_length") or win // 4
    if win != n_fft:
        raise NotImplementedError(f"win_length={win!r} != n_fft={n_fft!r} is not supported")
    if (n_fft, hop) not in ((1024, 256), (2048, 512)):
        raise NotImplementedError(f"n_fft={n_fft!r}, hop_length={hop!r} is not supported (only 1024 / 256 and 2048 / 512)")
    opts = _native.gate_opts(int(sr), **kw)
    _native.gate_params(opts)                                         # ValueError / NotImplementedError before any device work
    return opts


def _gate_signals(clips, opts, who: str) -> List[np.ndarray]:
    """The clips as mono float32; refuses an empty one and one longer than chunk_size, before any device work."""
    sig = _mono_f32(clips)
    for i, y in enumerate(sig):
        if y.size == 0:
            raise ValueError(f"{who}: signal {i} is empty")
        if y.size > opts.chunk_size:
            raise NotImplementedError(f"{who}: signal {i} has {y.size} samples, more than chunk_size={opts.chunk_size}: "
                                      "noisereduce's chunk loop is not supported")
    return sig


def _gate_run(sig: List[np.ndarray], noise, opts, device: int):
    """-> (denoised clips, status)"""
    lengths = np.array([s.size for s in sig], np.int64)
    n_off = n_len = None
    parts = list(sig)
    if noise is not None and opts.stationary:
        n_len = np.array([z.size for z in noise], np.int64)
        parts += list(noise)
    all_off = _native.packed_offsets([p.size for p in parts], 4)
    buf = np.zeros(int(all_off[-1]) + parts[-1].size if parts else 0, np.float32)
    for o, p in zip(all_off, parts):
        buf[o:o + p.size] = p
    offsets = all_off[:len(sig)]
    if n_len is not None:
        n_off = all_off[len(sig):]
    out = _ctx(device).gate_batch(buf, offsets, lengths, opts, noise_offsets=n_off, noise_lengths=n_len)
    return [out["out"][o:o + n].copy() for o, n in zip(out["offsets"], lengths)], out["status"]


def reduce_noise_batch(clips: Sequence[np.ndarray], sr: int, y_noise=None, *, device: int = 0, **kw) -> List[np.ndarray]:
    """``noisereduce.reduce_noise(y=clip, sr=sr, **kw)`` of many mono clips in one device pass.  ``y_noise``: one noise clip
    for all, or one per clip (stationary only, as in noisereduce).  A clip with a NaN / inf sample comes back as zeros.
    ``device`` may be a callable that names the device: it is asked only once the arguments have passed."""
    opts = _gate_opts(sr, dict(kw))
    sig = _gate_signals(clips, opts, "reduce_noise")
    noise = None
    if y_noise is not None:
        if isinstance(y_noise, np.ndarray) and y_noise.ndim == 1:
            y_noise = [y_noise] * len(sig)
        noise = _mono_f32(y_noise)
        if len(noise) != len(sig) or any(z.size == 0 for z in noise):
            raise ValueError("reduce_noise: y_noise must be one non-empty mono clip, or one per signal")
    if not sig:
        return []
    return _gate_run(sig, noise, opts, device() if callable(device) else device)[0]


def reduce_noise(y, sr: int, y_noise=None, *, device: int = 0, **kw) -> np.ndarray:
    """``noisereduce.reduce_noise(y, sr, ...)`` (3.0.3) for mono audio on the GPU: spectral gating, stationary (a per-bin
    threshold from the whole noise clip's dB statistics) or non-stationary (a sigmoid over |X| against its forward-backward
    smoothed self), the mask smoothed over time and frequency; float32 of ``y``'s length.  noisereduce's keywords and
    defaults; 1024 / 256 and 2048 / 512 frames; clips of at most ``chunk_size`` samples (DESIGN.md section 25 lists the
    deviations)."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise NotImplementedError(f"reduce_noise: only mono audio is supported, got shape {y.shape}")
    return reduce_noise_batch([y], sr, y_noise, device=device, **kw)[0]


# ---- time stretching (afx_time_stretch_batch): librosa.effects.time_stretch -------------------------------------------------
def time_stretch_batch(signals: Sequence[np.ndarray], rates, *, n_fft: int = 2048, hop_length: Optional[int] = None,
                       win_length: Optional[int] = None, window="hann", center: bool = True, pad_mode: str = "constant",
                       device: int = 0) -> List[Optional[np.ndarray]]:
    """``librosa.effects.time_stretch(signal, rate=rates[i], ...)`` of many mono signals in one device pass (one rate for all,
    or one per signal): stft, phase vocoder and istft with the spectra never leaving the device.  Per signal float32 of
    round(len / rate) samples, or None where the single call would raise.  ``device`` may be a callable that names the
    device: it is asked only once the arguments have passed."""
    from .core import spectrum as S
    opts = S._opts(n_fft, hop_length, win_length, center, pad_mode)
    table = S._window(window, win_length, opts.n_fft)
    sig = [S._signal(s, i) for i, s in enumerate(signals)]
    rates = [rates] * len(sig) if np.isscalar(rates) else list(rates)
    if len(rates) != len(sig):
        raise ValueError("rates must have one entry per signal")
    rates = [S._rate(r, i) for i, r in enumerate(rates)]
    if not sig:
        return []
    if len({s.dtype for s in sig}) > 1:
        sig = [s if s.dtype == np.float32 else s.astype(np.float32) / np.float32(32768.0) for s in sig]
    size = np.array([s.size for s in sig], np.int64)
    offsets = _native.packed_offsets(size, 4)
    buf = np.zeros(max(int((offsets + size).max()), 1), sig[0].dtype)
    for o, s in zip(offsets, sig):
        buf[o:o + s.size] = s
    r = _ctx(device() if callable(device) else device).time_stretch_batch(buf, offsets, size, rates, opts, table)
    return [r["out"][o:o + n].copy() if st == _native.CLIP_OK else None for o, n, st in zip(r["offsets"], r["samples"], r["status"])]


def time_stretch(y, *, rate, n_fft: int = 2048, hop_length: Optional[int] = None, win_length: Optional[int] = None,
                 window="hann", center: bool = True, pad_mode: str = "constant", device: int = 0) -> np.ndarray:
    """``librosa.effects.time_stretch(y, rate=rate, ...)`` for mono audio on the GPU: ``istft(phase_vocoder(stft(y), rate),
    length=round(len(y) / rate))`` in one device call; float32.  ``rate > 1`` speeds up.  stft's
    limits apply (n_fft 1024 or 2048); ValueError for a rate that is not finite and > 0 and for a clip stft refuses."""
    from .core import spectrum as S
    rate = S._rate(rate)
    out, = time_stretch_batch([y], [rate], n_fft=n_fft, hop_length=hop_length, win_length=win_length, window=window,
                              center=center, pad_mode=pad_mode, device=device)
    if out is None:
        raise ValueError("time_stretch: y is too short for this framing or not finite everywhere")
    return out
