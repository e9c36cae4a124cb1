"""Restatement of the rhythm group of 04_feature_extraction_experiment/feature_extractor.py:592-622 --
librosa.onset.onset_strength, the tempo of librosa.beat.beat_track (librosa.feature.tempo on librosa.feature.tempogram
with ac_size 8 s) and three scalars of the onset envelope -- at librosa 0.11's defaults, written out with numpy and
scipy.fft alone.  librosa is not installed where this runs, so this file is the spec of afx_rhythm_batch; parity with
librosa itself is unpinned, as for tests/chroma_ref.py.  The beat positions, which the reference discards, are not restated.

dtype "f64": every step in float64 (the oracle).  "f32": librosa's dtypes behind a float64 FFT (a float32 power
spectrogram, float32 dB, a float32 envelope, a float32 FFT autocorrelation).  "fft32": the same with the STFT itself taken
by a float32 FFT, which is what a float32 device computes -- the yardstick of the GPU tolerances."""
import numpy as np
import scipy.fft

from tests import chroma_ref as C
from tests.hpss_ref import HOP, N_FFT, window

KEYS = ("tempo", "rhythm_regularity", "onset_strength_mean", "onset_strength_std")
ONSET_LAG = 1 + N_FFT // (2 * HOP)            # zeros in front of the envelope: lag 1, and the centring of the frames
TINY32 = float(np.finfo(np.float32).tiny)


def power_spectrogram(y, dtype="f64") -> np.ndarray:
    """|X|^2, [1025, T]: chroma_ref's for "f64" / "f32"; "fft32": float32 frames, window, FFT and square"""
    if dtype != "fft32":
        return C.power_spectrogram(y, dtype == "f32")
    T = 1 + len(y) // HOP
    yp = np.pad(np.asarray(y, np.float32), N_FFT // 2)
    yp = np.pad(yp, (0, max(0, (T - 1) * HOP + N_FFT - yp.size)))
    idx = np.arange(T)[:, None] * HOP + np.arange(N_FFT)[None, :]
    X = scipy.fft.rfft(yp[idx] * window().astype(np.float32), axis=1).T
    assert X.dtype == np.complex64
    return (X.real * X.real + X.imag * X.imag).astype(np.float32)


def onset_from_mel(mel) -> np.ndarray:
    """onset_strength(S=power_to_db(mel)) in mel's dtype: dB with ref 1, amin 1e-10, top_db 80 over the clip; the rectified
    difference at lag 1; the mean over the bands; ONSET_LAG zeros in front; cut to T"""
    dt = mel.dtype.type
    T = mel.shape[1]
    db = dt(10.0) * np.log10(np.maximum(dt(1e-10), mel))
    db = np.maximum(db, db.max() - dt(80.0))
    e = np.mean(np.maximum(dt(0.0), db[:, 1:] - db[:, :-1]), axis=0, dtype=mel.dtype)
    return np.concatenate([np.zeros(ONSET_LAG, mel.dtype), e])[:T].astype(mel.dtype)


def onset_strength(y, sr, dtype="f64") -> np.ndarray:
    """librosa.onset.onset_strength(y=y, sr=sr): (T,), T = 1 + len(y) // 512; env[:3] == 0"""
    return onset_from_mel(C.mel_from(power_spectrogram(y, dtype), sr))


def max_abs_db(y, sr) -> float:
    """the largest |dB| of the float64 mel power of y (what a float32 dB value of the clip is rounded at)"""
    mel = C.mel_from(power_spectrogram(y), sr)
    db = 10.0 * np.log10(np.maximum(1e-10, mel))
    return float(np.max(np.abs(np.maximum(db, db.max() - 80.0))))


def tempo_table(sr):
    """(win, kmin, bpm[win], logprior[win]) of librosa.feature.tempo(sr=sr, hop_length=512, start_bpm=120, std_bpm=1,
    ac_size=8, max_tempo=320): win = int(8 sr) // 512 (what beat_track gives tempogram, not its default 384), bpm[0] = inf,
    logprior = -inf below kmin, the first lag slower than 320 bpm"""
    win = int(8.0 * sr) // HOP
    bpm = np.zeros(win, np.float64)
    bpm[0] = np.inf
    bpm[1:] = 60.0 * sr / (HOP * np.arange(1.0, win))
    with np.errstate(invalid="ignore"):
        logprior = -0.5 * ((np.log2(bpm) - np.log2(120.0)) / 1.0) ** 2
    kmin = int(np.argmax(bpm < 320.0))
    logprior[:kmin] = -np.inf
    return win, kmin, bpm, logprior


def tempogram(env, sr, f32=False) -> np.ndarray:
    """librosa.feature.tempogram(onset_envelope=env, sr=sr, win_length=int(8 sr) // 512): [win, T] in float64, or with
    librosa's float32 dtypes (a float32 FFT autocorrelation).  The direct sum over i < win - k of x[i] x[i + k] is what the
    FFT of the frame zero-padded past 2 win - 1 computes."""
    win = int(8.0 * sr) // HOP
    dt = np.float32 if f32 else np.float64
    env = np.asarray(env, dt)
    T = env.shape[0]
    p = np.pad(env, win // 2, mode="linear_ramp", end_values=0)
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)).astype(dt)
    x = p[np.arange(win)[:, None] + np.arange(T)[None, :]] * w[:, None]
    n_pad = scipy.fft.next_fast_len(2 * win - 1, real=True)
    X = scipy.fft.rfft(x, n=n_pad, axis=0)
    ac = scipy.fft.irfft(X.real * X.real + X.imag * X.imag, n=n_pad, axis=0)[:win]
    assert ac.dtype == dt
    mx = np.max(np.abs(ac), axis=0, keepdims=True)
    return ac / np.where(mx < TINY32, dt(1), mx)


def tempogram_direct(env, sr) -> np.ndarray:
    """the same in float64 by the sum itself (small inputs: the cross-check of the FFT route)"""
    win = int(8.0 * sr) // HOP
    env = np.asarray(env, np.float64)
    p = np.pad(env, win // 2, mode="linear_ramp", end_values=0)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    out = np.zeros((win, env.shape[0]))
    for t in range(env.shape[0]):
        x = p[t:t + win] * w
        ac = np.array([np.dot(x[:win - k], x[k:]) for k in range(win)])
        mx = np.max(np.abs(ac))
        out[:, t] = ac / (1.0 if mx < TINY32 else mx)
    return out


def decide(acmean, sr):
    """(lag, tempo, scores) of the mean tempogram: the first maximum of log1p(1e6 acmean) + logprior"""
    _, _, bpm, logprior = tempo_table(sr)
    score = np.log1p(1e6 * np.asarray(acmean, np.float64)) + logprior
    lag = int(np.argmax(score))
    return lag, float(bpm[lag]), score


def tempo_from(env, sr, f32=False):
    """(tempo, lag, acmean, scores) of beat_track's tempo for an onset envelope; 0.0 (lag 0) when it has no non-zero value"""
    tg = tempogram(env, sr, f32)
    acmean = np.mean(tg, axis=1)
    lag, bpm, score = decide(acmean, sr)
    if not np.any(env):
        return 0.0, 0, acmean, score
    return bpm, lag, acmean, score


def tempo(y, sr, dtype="f64") -> float:
    return tempo_from(onset_strength(y, sr, dtype), sr, dtype != "f64")[0]


def rhythm_features(y, sr, dtype="f64") -> dict:
    env = onset_strength(y, sr, dtype)
    mean, std = float(np.mean(env, dtype=np.float64)), float(np.std(env, dtype=np.float64))
    return dict(zip(KEYS, (tempo_from(env, sr, dtype != "f64")[0], std / (mean + 1e-8), mean, std)))


def tempo_lead(y, sr):
    """(lags, lead): the lag each of ten envelopes chooses -- float64, librosa's dtypes, the float64 one times (1 + 1e-5
    randn) with eight fixed seeds -- and the smallest lead of a best score over its runner-up.  ((0,) * 10, inf) when
    every envelope is all zero."""
    e64 = onset_strength(y, sr)
    envs = [(e64, False), (onset_strength(y, sr, "f32"), True)]
    for seed in range(8):
        envs.append((e64 * (1.0 + 1e-5 * np.random.default_rng(2000 + seed).standard_normal(e64.shape)), False))
    lags, lead = [], np.inf
    for env, f32 in envs:
        _, lag, _, score = tempo_from(env, sr, f32)
        lags.append(lag)
        if np.any(env):
            top = np.sort(score[np.isfinite(score)])
            lead = min(lead, float(top[-1] - top[-2]))
    return tuple(lags), lead


def tempo_is_robust(y, sr) -> bool:
    """True when the tempo of y may be pinned exactly: the ten envelopes of tempo_lead choose one lag and every best score
    leads its runner-up by at least 1e-2.  The lead is a condition, not a measurement: scores are O(10) and a float32 path
    moves them by about 1e-6."""
    lags, lead = tempo_lead(y, sr)
    return len(set(lags)) == 1 and lead >= 1e-2


def clicks(sr, bpm, seconds=8.0, noise=1e-3, seed=7, silent=None) -> np.ndarray:
    """decaying 1 kHz bursts every 60 / bpm s on white noise; silent = (t0, t1): digital silence over that stretch"""
    n = int(seconds * sr)
    t = np.arange(n) / float(sr)
    y = noise * np.random.default_rng(seed).standard_normal(n)
    period = 60.0 / bpm
    k = 0
    while k * period < seconds:
        d = t - k * period
        on = (d >= 0) & (d < 0.1)
        y[on] += 0.5 * np.sin(2 * np.pi * 1000.0 * d[on]) * np.exp(-d[on] / 0.02)
        k += 1
    if silent is not None:
        y[int(silent[0] * sr):int(silent[1] * sr)] = 0.0
    return y.astype(np.float32)
