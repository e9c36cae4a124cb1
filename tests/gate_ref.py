"""Float64 oracle of spectral-gating noise reduction: noisereduce 3.0.3's ``reduce_noise`` for one mono clip no longer than
``chunk_size``, restated with numpy + scipy (DESIGN.md section 25 is the definition; the library is not installed, so
parity with it is unpinned).  Two forms:

* ``f32=False``: float64 throughout, the truth;
* ``f32=True``: rounds to float32 wherever a float32 implementation must -- the windowed frame, the FFT, the mask product, the
  inverse FFT, the overlap-add and its normalisation.  Statistics, thresholds and the smoothing stay float64.  Its distance
  from the float64 form is the yardstick the device's tolerances are multiples of.

Deviations from the library, fixed by the definition: float64 on both grids, S = 0 gives mask 0, a NaN / inf sample gives a
zero output, and a clip longer than ``chunk_size`` is refused.
"""
import numpy as np
import scipy.fft
import scipy.signal

EPS = np.finfo(np.float64).eps          # 2^-52
TOP_DB = 80.0

DEFAULTS = dict(stationary=False, prop_decrease=1.0, time_constant_s=2.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50,
                thresh_n_mult_nonstationary=2, sigmoid_slope_nonstationary=10, n_std_thresh_stationary=1.5,
                chunk_size=600000, padding=30000, n_fft=1024, clip_noise_stationary=True)


def hann(n):
    """scipy.signal.get_window('hann', n): periodic."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def n_frames(length, hop, padding=30000):
    """Frames of the signal grid of a clip of ``length`` samples."""
    return 1 + (length + 2 * padding) // hop


def stft(x, n_fft, hop, f32=False):
    """scipy.signal.stft(x, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop, padded=False) at scipy's other defaults:
    [bins, T] with T = 1 + len(x) // hop.  f32: the windowed frame and the spectrum are rounded to float32 / complex64."""
    x = np.asarray(x, np.float64)
    w = hann(n_fft)
    xp = np.concatenate([np.zeros(n_fft // 2), x, np.zeros(n_fft // 2)])
    T = 1 + x.size // hop
    fr = np.lib.stride_tricks.sliding_window_view(xp, n_fft)[::hop][:T]
    if f32:
        fr = (fr.astype(np.float32) * w.astype(np.float32)).astype(np.float64)
        X = (scipy.fft.rfft(fr, axis=-1) / w.sum()).astype(np.complex64).astype(np.complex128)
    else:
        X = scipy.fft.rfft(fr * w, axis=-1) / w.sum()
    return np.ascontiguousarray(X.T)


def istft(Y, n_fft, hop, f32=False):
    """The matching scipy.signal.istft: (T - 1) hop samples.  f32: the inverse FFT, the windowed segment, the overlap-add
    (increasing frame order) and the normalisation are float32."""
    T = Y.shape[1]
    w = hann(n_fft)
    seg = scipy.fft.irfft(Y.T, n=n_fft, axis=-1)
    dt = np.float32 if f32 else np.float64
    if f32:
        seg = seg.astype(np.float32) * (w.astype(np.float32) * np.float32(w.sum()))
        w2 = w.astype(np.float32) ** 2
    else:
        seg = seg * (w * w.sum())
        w2 = w * w
    x = np.zeros((T - 1) * hop + n_fft, dt)
    norm = np.zeros_like(x)
    for t in range(T):
        x[t * hop:t * hop + n_fft] += seg[t]
        norm[t * hop:t * hop + n_fft] += w2
    x = np.where(norm > 1e-10, x / np.where(norm > 1e-10, norm, 1), x)
    return x[n_fft // 2:n_fft // 2 + (T - 1) * hop].astype(np.float64)


def db(a):
    """20 log10(a + 2^-52), floored per frequency row at the row's maximum over time minus 80."""
    d = 20.0 * np.log10(a + EPS)
    return np.maximum(d, d.max(axis=1, keepdims=True) - TOP_DB)


def smooth_sizes(sr, n_fft, hop, freq_mask_smooth_hz=500, time_mask_smooth_ms=50):
    """(n_f, n_t); ValueError where noisereduce raises."""
    n_f = int(freq_mask_smooth_hz / (sr / (n_fft / 2)))
    n_t = int(time_mask_smooth_ms / (hop / sr * 1000))
    if n_f < 1:
        raise ValueError("freq_mask_smooth_hz needs to be at least %g Hz" % (sr / (n_fft / 2)))
    if n_t < 1:
        raise ValueError("time_mask_smooth_ms needs to be at least %g ms" % (hop / sr * 1000))
    return n_f, n_t


def taps(n):
    """The 2 n + 1 taps of one axis of the smoothing filter, not normalised."""
    return np.concatenate([np.linspace(0, 1, n + 1, endpoint=False), np.linspace(1, 0, n + 2)])[1:-1]


def smoothing_filter(n_f, n_t):
    F = np.outer(taps(n_f), taps(n_t))
    return F / F.sum()


def beta(sr, hop, time_constant_s=2.0):
    t = time_constant_s * sr / float(hop)
    return (np.sqrt(1 + 4 * t ** 2) - 1) / (2 * t ** 2)


def reduce_noise(y, sr, y_noise=None, f32=False, hard_mask=None, thresh=None, parts=None, **kw):
    """The denoised clip as float32[len(y)].  ``hard_mask`` ([bins, T] bool) or ``thresh`` ([bins], dB) override the
    stationary decision, so that a device's own decisions can be followed; ``parts`` (a dict) receives X, thr, hard, mask."""
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p) - {"win_length", "hop_length"}
    if unknown:
        raise TypeError("unknown arguments %s" % sorted(unknown))
    p.update({k: v for k, v in kw.items() if k in p})
    n_fft = int(p["n_fft"])
    win = kw.get("win_length") or n_fft
    hop = kw.get("hop_length") or win // 4
    if win != n_fft:
        raise NotImplementedError("win_length != n_fft")
    y = np.asarray(y)
    if y.ndim != 1 or y.size == 0:
        raise ValueError("a mono clip of at least one sample")
    if y.size > p["chunk_size"]:
        raise NotImplementedError("clips longer than chunk_size")
    n_f, n_t = smooth_sizes(sr, n_fft, hop, p["freq_mask_smooth_hz"], p["time_mask_smooth_ms"])
    do_smooth = not (n_f == 1 and n_t == 1)
    noise = y if y_noise is None else np.asarray(y_noise)
    if not (np.all(np.isfinite(y)) and np.all(np.isfinite(noise))):
        return np.zeros(y.size, np.float32)
    pad, pd = int(p["padding"]), float(p["prop_decrease"])
    chunk = np.concatenate([np.zeros(pad), y.astype(np.float64), np.zeros(pad)])
    X = stft(chunk, n_fft, hop, f32)
    A = np.abs(X)
    F = smoothing_filter(n_f, n_t)
    out = {}
    if p["stationary"]:
        if hard_mask is None:
            if thresh is None:
                if p["clip_noise_stationary"]:
                    noise = noise[:p["chunk_size"]]
                N = db(np.abs(stft(noise.astype(np.float64), n_fft, hop, f32)))
                thresh = N.mean(axis=1) + p["n_std_thresh_stationary"] * N.std(axis=1)
            hard_mask = db(A) > np.asarray(thresh, np.float64)[:, None]
        out["thr"], out["hard"] = thresh, np.asarray(hard_mask, bool)
        mask = out["hard"] * pd + (1.0 - pd)
        if do_smooth:
            mask = scipy.signal.fftconvolve(mask, F, mode="same")
    else:
        b = beta(sr, hop, p["time_constant_s"])
        S = scipy.signal.filtfilt([b], [1, b - 1], A, axis=-1, padtype=None)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            mask = 1.0 / (1.0 + np.exp(-((A - S) / S - p["thresh_n_mult_nonstationary"]) * p["sigmoid_slope_nonstationary"]))
        mask = np.where(S == 0, 0.0, mask)
        if do_smooth:
            mask = scipy.signal.fftconvolve(mask, F, mode="same")
        mask = mask * pd + (1.0 - pd)
    if f32:
        m32 = mask.astype(np.float32).astype(np.float64)
        Y = (X * m32).astype(np.complex64).astype(np.complex128)
    else:
        Y = X * mask
    x = istft(Y, n_fft, hop, f32)
    full = np.zeros(chunk.size)
    full[:x.size] = x[:chunk.size]
    if parts is not None:
        out["X"], out["mask"] = X, mask
        parts.update(out)
    return full[pad:pad + y.size].astype(np.float32)


def make_clip(sr, seconds=2.0, seed=0, silence=False, length=None):
    """The issue's clip: a gated two-tone (vibrato 220 Hz + 0.5 x 1330 Hz) plus white noise, float32."""
    n = int(round(sr * seconds)) if length is None else int(length)
    t = np.arange(n) / sr
    rng = np.random.default_rng(seed)
    tone = np.sin(2 * np.pi * 220 * t + 3.0 * np.sin(2 * np.pi * 5 * t)) + 0.5 * np.sin(2 * np.pi * 1330 * t)
    y = 0.3 * (np.sin(2 * np.pi * 1.5 * t) > 0.2) * tone + 0.02 * rng.standard_normal(n)
    if silence:
        y[:n // 8] = 0.0
    return y.astype(np.float32)


def noise_clip(sr, seconds=1.0, seed=100):
    rng = np.random.default_rng(seed)
    return (0.02 * rng.standard_normal(int(round(sr * seconds)))).astype(np.float32)
