"""Restatement of the reference's STFT-domain noise reducers (00_audio_data_collection_experiment/noise_reduction.py:15-92:
``spectral_subtraction``, ``wiener_filter``) and of the conditioning in front of its DTW aligner
(05_dtw_alignment_experiment/process_audio.py:13-51: RMS gain, spectral subtraction of the whole profile, energy VAD),
written out with numpy alone on the STFT / ISTFT of tests/hpss_ref.py.

``f32=False``: every step in float64 (the oracle).  ``f32=True``: the reference's dtypes -- the STFT in float64 rounded to
complex64, float32 magnitudes, profile and gains, the gained spectrum as complex64, overlap-add into a float32 signal
(as ``hpss_ref.hpss(f32=True)`` does) -- which bounds what the reference itself would get.

Every reducer returns an array of its input's length: the ISTFT gives L' = 512 (len // 512) samples and the reference pads
the rest with zeros."""
import numpy as np

from tests.hpss_ref import HOP, istft, stft, window  # noqa: F401  (window: re-exported for the tests)

EPS = float(np.finfo(float).eps)             # 2^-52, what wiener_filter adds to its denominator


def kept(n: int) -> int:
    """L': the samples librosa.istft(length=None) returns for a signal of n samples"""
    return HOP * (n // HOP)


def _unit_phase(X, S):
    zero = S == 0
    return np.where(zero, 1, X / np.where(zero, 1, S)).astype(X.dtype)


def _reconstruct(Y, n, f32):
    out = np.zeros(n, np.float32 if f32 else np.float64)
    Lp = kept(n)
    if Lp:
        out[:Lp] = istft(Y, Lp, f32)
    return out


def spectral_subtraction(y, beta=0.01, noise_frames=10, f32=False):
    """Y = max(|X| - beta N, 0) exp(i angle X), N the mean magnitude of the first min(T, noise_frames) frames"""
    y = np.asarray(y)
    if y.size == 0:
        return np.zeros(0, np.float32 if f32 else np.float64)
    X = stft(y, f32)
    S = np.abs(X)                                                   # float32 for complex64
    N = np.mean(S[:, :noise_frames], axis=1, keepdims=True)
    C = np.maximum(S - S.dtype.type(beta) * N, 0)
    return _reconstruct((C * _unit_phase(X, S)).astype(X.dtype), y.size, f32)


def wiener(y, noise_frames=10, f32=False):
    """Y = X P / (P + Np + eps), P = |X|^2, Np the mean power of the first min(T, noise_frames) frames"""
    y = np.asarray(y)
    if y.size == 0:
        return np.zeros(0, np.float32 if f32 else np.float64)
    X = stft(y, f32)
    P = np.abs(X) ** 2
    Np = np.mean(P[:, :noise_frames], axis=1, keepdims=True)
    G = P / (P + Np + P.dtype.type(EPS))
    return _reconstruct((X * G).astype(X.dtype), y.size, f32)


def rms_gain(y, f32=False):
    """(gain, y * gain): gain = 0.1 / (sqrt(mean y^2) + 1e-6)"""
    y = np.asarray(y, np.float32 if f32 else np.float64)
    g = 0.1 / (np.sqrt(np.mean(y ** 2)) + 1e-6)                      # a float32 scalar with f32 (numpy keeps the array's type)
    g = y.dtype.type(g)
    return float(g), y * g


def vad_frames(Lp: int, sr: int):
    """(fl, hop, F) of librosa.feature.rms(frame_length=int(0.025 sr), hop_length=int(0.010 sr), center=True)"""
    fl, hop = int(0.025 * sr), int(0.010 * sr)
    return fl, hop, 1 + (Lp + 2 * (fl // 2) - fl) // hop


def vad(d, sr, f32=False) -> dict:
    """The energy VAD over the denoised signal d: centred (zero-padded) RMS frames, threshold half their mean, and the
    reference's copy loop, whose windows [i hop, i hop + fl) are NOT centred and are skipped when they pass the end."""
    d = np.asarray(d, np.float32 if f32 else np.float64)
    fl, hop, F = vad_frames(d.size, sr)
    p = np.pad(d, fl // 2)
    idx = np.arange(F)[:, None] * hop + np.arange(fl)[None, :]
    e = np.sqrt(np.mean(np.abs(p[idx]) ** 2, axis=1))
    thr = e.dtype.type(0.5) * np.mean(e)
    speech = e > thr
    mask = np.zeros(d.size, bool)
    for i in np.flatnonzero(speech):
        if i * hop + fl <= d.size:
            mask[i * hop:i * hop + fl] = True
    return {"out": np.where(mask, d, 0).astype(d.dtype), "mask": mask, "e": e, "thr": float(thr), "speech": speech,
            "fl": fl, "hop": hop}


def preprocess_alignment(y, sr, f32=False) -> dict:
    """process_audio.py:13-51 for a signal of at least 512 samples: ``out`` (L' samples), ``d`` (the denoised signal the
    VAD masks), ``mask``, ``gain``, ``thr``, ``speech``, ``e``, ``scaled`` (the signal the STFT sees)"""
    g, scaled = rms_gain(y, f32)
    d = spectral_subtraction(scaled, beta=1.0, noise_frames=10, f32=f32)[:kept(len(scaled))]
    v = vad(d, sr, f32)
    v.update(d=d, gain=g, scaled=scaled)
    return v
