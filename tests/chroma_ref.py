"""Restatement of the timbre group of 04_feature_extraction_experiment/feature_extractor.py:558-590 --
librosa.feature.chroma_stft (with librosa.estimate_tuning / piptrack), librosa.feature.melspectrogram and the scalar MFCC
statistics -- at librosa's defaults (n_fft 2048, hop 512, centred, zero padding, periodic Hann, power 2), written out with
numpy alone.  librosa is not installed where this runs, so this file is the spec of afx_chroma_batch; parity with librosa
itself is unpinned, as for tests/hpss_ref.py.

``f32=False``: every step in float64 (the oracle).  ``f32=True``: librosa's dtypes (a float32 power spectrogram and
float32 arithmetic behind it), which bounds what librosa itself would get."""
import numpy as np

from oracle import cpu_ref
from tests.hpss_ref import BINS, N_FFT, stft

N_CHROMA, N_MELS, N_MFCC = 12, 128, 13
EDGES = np.linspace(-0.5, 0.5, 101)          # estimate_tuning(resolution=0.01): 100 bins, EDGES[50] == 0.0
KEYS = ("mel_energy_mean", "mel_energy_std", "chroma_mean", "chroma_std", "mfcc_mean", "mfcc_std")


def power_spectrogram(y, f32=False) -> np.ndarray:
    """|X|^2, [1025, T]; float32 (librosa's spectrogram dtype for float32 audio) or float64"""
    S = np.abs(stft(y)) ** 2
    return S.astype(np.float32) if f32 else S


def piptrack(S, sr):
    """librosa.piptrack(S=S, sr=sr, fmin=150, fmax=4000, threshold=0.1, ref=max over the frame) in S's dtype (S is used as
    given: the power spectrogram is treated as the magnitude) -> (peak mask [1025, T], pitch, mag)"""
    dt = S.dtype.type
    b = np.zeros_like(S)
    a = np.zeros_like(S)
    b[1:-1] = (S[2:] - S[:-2]) / dt(2)
    a[1:-1] = S[2:] + S[:-2] - dt(2) * S[1:-1]
    flat = np.abs(b) >= np.abs(a)
    shift = np.where(flat, dt(0), -b / np.where(flat, dt(1), a)).astype(S.dtype)
    dskew = dt(0.5) * b * shift
    Sm = S * (S > dt(0.1) * S.max(axis=0, keepdims=True))
    k = np.arange(BINS)
    f = k * (float(sr) / N_FFT)
    band = (f >= 150.0) & (f < min(4000.0, sr / 2.0))
    peak = np.zeros(S.shape, bool)
    peak[1:-1] = (Sm[1:-1] > Sm[:-2]) & (Sm[1:-1] >= Sm[2:])
    peak &= band[:, None]
    pitch = ((k[:, None].astype(S.dtype) + shift) * dt(float(sr) / N_FFT)).astype(S.dtype)
    return peak, pitch, (S + dskew).astype(S.dtype)


def tuning_histogram(S, sr):
    """(peaks, kept, counts[100]) of librosa.estimate_tuning(S=S, sr=sr, resolution=0.01, bins_per_octave=12)"""
    peak, pitch, mag = piptrack(S, sr)
    p, m = pitch[peak], mag[peak]
    if p.size == 0:
        return 0, 0, np.zeros(100, np.int64)
    keep = m >= np.median(m)
    r = np.mod(S.dtype.type(12) * np.log2(p[keep] / S.dtype.type(27.5)), S.dtype.type(1))
    r = np.where(r >= 0.5, r - S.dtype.type(1), r)
    counts = np.histogram(r.astype(np.float64), EDGES)[0]
    return int(p.size), int(keep.sum()), counts


def estimate_tuning(S, sr) -> float:
    peaks, _, counts = tuning_histogram(S, sr)
    return 0.0 if peaks == 0 else float(EDGES[int(np.argmax(counts))])


def chroma_filters(sr, tuning=0.0) -> np.ndarray:
    """librosa.filters.chroma(sr=sr, n_fft=2048, tuning=tuning) at its defaults: [12, 1025] float32"""
    fr = np.linspace(0, sr, N_FFT, endpoint=False)[1:]
    q = N_CHROMA * np.log2(fr / (440.0 * 2.0 ** (tuning / N_CHROMA) / 16))
    q = np.concatenate(([q[0] - 1.5 * N_CHROMA], q))
    bw = np.concatenate((np.maximum(q[1:] - q[:-1], 1.0), [1.0]))
    D = np.remainder(q[None, :] - np.arange(N_CHROMA)[:, None] + N_CHROMA // 2 + 10 * N_CHROMA, N_CHROMA) - N_CHROMA // 2
    w = np.exp(-0.5 * (2 * D / bw) ** 2)
    w = w / np.maximum(np.sqrt(np.sum(w ** 2, axis=0)), np.finfo(np.float64).tiny)
    w = w * np.exp(-0.5 * (((q / N_CHROMA - 5.0) / 2.0) ** 2))
    return np.roll(w, -3, axis=0)[:, :BINS].astype(np.float32)


def chroma_from(S, sr, tuning=None) -> np.ndarray:
    if tuning is None:
        tuning = estimate_tuning(S, sr)
    raw = chroma_filters(sr, tuning).astype(S.dtype) @ S
    mx = np.max(np.abs(raw), axis=0, keepdims=True)
    return raw / np.where(mx < np.finfo(np.float32).tiny, S.dtype.type(1), mx)


def chroma_stft(y, sr, tuning=None, f32=False) -> np.ndarray:
    return chroma_from(power_spectrogram(y, f32), sr, tuning)


def mel_from(S, sr) -> np.ndarray:
    return cpu_ref.mel_filterbank(sr, N_FFT, N_MELS).astype(S.dtype) @ S


def melspectrogram(y, sr, f32=False) -> np.ndarray:
    return mel_from(power_spectrogram(y, f32), sr)


def mfcc_from(mel) -> np.ndarray:
    """librosa.feature.mfcc(n_mfcc=13) of a mel power matrix: dct(power_to_db(mel, top_db=80))[:13]"""
    import scipy.fft
    return scipy.fft.dct(cpu_ref.power_to_db(mel), axis=-2, type=2, norm="ortho")[:N_MFCC]


def timbre_features(y, sr, f32=False) -> dict:
    S = power_spectrogram(y, f32)
    mel = mel_from(S, sr)
    chroma = chroma_from(S, sr)
    mf = mfcc_from(mel)
    vals = (np.mean(mel), np.std(mel), np.mean(chroma), np.std(chroma), np.mean(mf), np.std(mf))
    return dict(zip(KEYS, (float(v) for v in vals)))


def tuning_is_robust(y, sr) -> bool:
    """True when the tuning of y may be pinned exactly: ten estimates (float64 S, float32 S, S64 * (1 + 1e-5 randn) with
    eight fixed seeds) agree and in each the top count exceeds the runner-up by at least 8 -- a peak whose magnitude sits at
    the median, or whose residual sits on a bin edge, may fall either way in float32 -- or none of the ten has a peak."""
    S64 = power_spectrogram(y)
    variants = [S64, S64.astype(np.float32)]
    for seed in range(8):
        variants.append(S64 * (1.0 + 1e-5 * np.random.default_rng(1000 + seed).standard_normal(S64.shape)))
    hists = [tuning_histogram(S, sr) for S in variants]
    if all(h[0] == 0 for h in hists):
        return True
    if any(h[0] == 0 for h in hists):
        return False
    tops = set()
    for _, _, counts in hists:
        order = np.sort(counts)
        if order[-1] - order[-2] < 8:
            return False
        tops.add(int(np.argmax(counts)))
    return len(tops) == 1


def tones(sr, n, freqs, noise=0.0, seed=5) -> np.ndarray:
    t = np.arange(n) / float(sr)
    y = sum(np.sin(2 * np.pi * f * t) for f in freqs) * (0.5 / len(freqs))
    if noise:
        y = y + noise * np.random.default_rng(seed).standard_normal(n)
    return y.astype(np.float32)
