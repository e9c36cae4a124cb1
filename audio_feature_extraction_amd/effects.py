"""``librosa.effects.hpss / harmonic / percussive`` on the GPU: harmonic-percussive separation at librosa 0.11's defaults
(kernel_size 31, power 2, margin 1) on the 2048 / 512 periodic-Hann STFT, the separation the reference's harmonic features
start from (04_feature_extraction_experiment/feature_extractor.py:525-556).

The STFT, both 31-tap median filters, the soft masks and the inverse STFT run in ``libafx.so`` (``afx_hpss_batch``); there
is no CPU fallback.  The time-axis median follows scipy's 'reflect' mirror repeated with period 2T for every clip of T
frames (scipy itself departs from it at T = 2, i.e. 512 .. 1023 samples).

On the same STFT, the reference's STFT-domain noise reducers (00_audio_data_collection_experiment/noise_reduction.py:15-92:
``spectral_subtraction``, ``wiener_filter``) and the signal conditioning in front of its DTW aligner
(05_dtw_alignment_experiment/process_audio.py:9-54: ``preprocess_alignment``), all in ``afx_denoise_batch``.
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
