"""Restatement of librosa.effects.hpss / harmonic (librosa 0.11 defaults: kernel_size 31, power 2, margin 1) and of the
harmonic features of 04_feature_extraction_experiment/feature_extractor.py:525-556, written out with numpy alone.

``f32=False``: every step in float64 (the oracle).  ``f32=True``: librosa's dtypes (the STFT in float64 rounded to
complex64, float32 magnitudes, medians and masks, float32 irfft, overlap-add into a float32 signal), which bounds what
librosa itself would get.  The median filters write scipy's 'reflect' rule out: the half-sample mirror
``d c b a | a b c d | d c b a``, repeated with period 2n when the window is longer than the row."""
import numpy as np

N_FFT, HOP, HALF, BINS = 2048, 512, 15, 1025


def window() -> np.ndarray:
    n = np.arange(N_FFT)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)


def reflect(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def stft(y, f32=False) -> np.ndarray:
    """centred (zero-padded) periodic-Hann STFT, [1025, T], T = 1 + len(y) // 512"""
    T = 1 + len(y) // HOP
    yp = np.pad(np.asarray(y, np.float64), N_FFT // 2)
    yp = np.pad(yp, (0, max(0, (T - 1) * HOP + N_FFT - yp.size)))
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    X = np.fft.rfft(yp[idx] * window(), axis=1).T
    return X.astype(np.complex64) if f32 else X


def median_time(S: np.ndarray) -> np.ndarray:
    """median_filter(S, size=(1, 31), mode='reflect') with the periodic mirror for every T"""
    T = S.shape[1]
    out = np.empty_like(S)
    for t0 in range(0, T, 256):
        t = np.arange(t0, min(T, t0 + 256))
        idx = reflect(t[:, None] + np.arange(-HALF, HALF + 1)[None, :], T)
        out[:, t] = np.sort(S[:, idx], axis=-1)[..., HALF]
    return out


def median_freq(S: np.ndarray) -> np.ndarray:
    """median_filter(S, size=(31, 1), mode='reflect')"""
    F = S.shape[0]
    idx = reflect(np.arange(F)[:, None] + np.arange(-HALF, HALF + 1)[None, :], F)
    out = np.empty_like(S)
    for t0 in range(0, S.shape[1], 256):
        blk = S[:, t0:t0 + 256]
        out[:, t0:t0 + 256] = np.sort(blk[idx], axis=1)[:, HALF]
    return out


def softmask(X, X_ref):
    """librosa.util.softmask(X, X_ref, power=2, split_zeros=True) in X's dtype"""
    Z = np.maximum(X, X_ref)
    bad = Z < np.finfo(X.dtype).tiny
    Z = np.where(bad, 1, Z).astype(X.dtype)
    m, r = (X / Z) ** 2, (X_ref / Z) ** 2
    out = np.where(bad, X.dtype.type(0.5), m / np.where(bad, 1, m + r))
    return out.astype(X.dtype)


def istft(Y: np.ndarray, length: int, f32=False) -> np.ndarray:
    T = Y.shape[1]
    fr = np.fft.irfft(Y.T, n=N_FFT, axis=1)
    w = window()
    dt = np.float32 if f32 else np.float64
    out = np.zeros(N_FFT + HOP * (T - 1), dt)
    wss = np.zeros_like(out)
    ytmp = fr * w
    for t in range(T):                          # frames in increasing order (librosa's __overlap_add)
        out[t * HOP:t * HOP + N_FFT] += ytmp[t]
        wss[t * HOP:t * HOP + N_FFT] += w ** 2
    out, wss = out[N_FFT // 2:N_FFT // 2 + length], wss[N_FFT // 2:N_FFT // 2 + length]
    nz = wss > np.finfo(dt).tiny
    out[nz] /= wss[nz]
    return out


def hpss(y, f32=False):
    """(h, p, S, Hm, Pm)"""
    X = stft(y, f32)
    S = np.abs(X)
    Hm, Pm = median_time(S), median_freq(S)
    mh, mp = softmask(Hm, Pm), softmask(Pm, Hm)
    zero = S == 0
    phase = np.where(zero, 1, X / np.where(zero, 1, S)).astype(X.dtype)
    h = istft((S * mh) * phase, len(y), f32)
    p = istft((S * mp) * phase, len(y), f32)
    return h, p, S, Hm, Pm


def centroid(y, sr) -> np.ndarray:
    """librosa.feature.spectral_centroid(y=y, sr=sr)[0] at its defaults, float64"""
    S = np.abs(stft(y))
    f = np.arange(BINS) * (sr / N_FFT)
    tot = S.sum(axis=0)
    return (f[:, None] * S).sum(axis=0) / np.where(tot < np.finfo(np.float32).tiny, 1.0, tot)


def harmonic_features(y, sr, h=None) -> dict:
    if h is None:
        h = hpss(y)[0]
    y = np.asarray(y, np.float64)
    eh = float(np.sum(np.asarray(h, np.float64) ** 2))
    c = centroid(h, sr)
    return {"harmonic_energy": eh, "harmonic_ratio": eh / (float(np.sum(y ** 2)) + 1e-8),
            "harmonic_freq_mean": float(np.mean(c)), "harmonic_freq_std": float(np.std(c))}


def click_train(n: int, every: int = 5000) -> np.ndarray:
    y = np.zeros(n, np.float32)
    y[::every] = 1.0
    return y
