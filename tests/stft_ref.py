"""Oracle of librosa-style ``stft`` / ``istft`` (librosa 0.11), restated with numpy + scipy (DESIGN.md section 26 is the
definition; librosa is not installed, so parity with it is unpinned).  Two forms:

* ``f32=False``: float64 throughout, the truth;
* ``f32=True``: the float32-faithful form -- float32 window and frames, ``scipy.fft.rfft`` / ``irfft`` in single precision,
  float32 accumulations in increasing frame order.  Its distance from the float64 form is the yardstick the device's
  tolerances are multiples of.
"""
import numpy as np
import scipy.fft
import scipy.signal

TINY = np.finfo(np.float32).tiny


def pad_center(w, size):
    """librosa.util.pad_center for a 1-D array: zeros on both sides, the odd one on the right."""
    w = np.asarray(w)
    lpad = (size - w.size) // 2
    if lpad < 0:
        raise ValueError("window longer than n_fft")
    return np.pad(w, (lpad, size - w.size - lpad))


def get_window(window, win_length, n_fft):
    """The float64 window of n_fft values: scipy's periodic window of win_length (or the caller's array), padded centred."""
    if isinstance(window, (str, tuple, float)):
        w = scipy.signal.get_window(window, win_length, fftbins=True)
    else:
        w = np.asarray(window, np.float64)
        if w.shape != (win_length,):
            raise ValueError("window must hold win_length values")
    return pad_center(w, n_fft)


def _framing(n_fft, hop_length, win_length):
    win_length = n_fft if win_length is None else int(win_length)
    hop = win_length // 4 if hop_length is None else int(hop_length)
    return win_length, hop


def n_frames(length, n_fft, hop, center=True, pad_mode="constant"):
    """Frames of a clip, or None where the definition refuses it (too short)."""
    if length == 0 or (not center and length < n_fft) or (center and pad_mode == "reflect" and length <= n_fft // 2):
        return None
    return 1 + (length + (n_fft if center else 0) - n_fft) // hop


def stft(y, n_fft=2048, hop_length=None, win_length=None, window="hann", center=True, pad_mode="constant", f32=False):
    """[1 + n_fft / 2, T] in Fortran order: complex128, or complex64 with f32.  ValueError for a clip that is too short or
    not finite, and for a pad_mode other than constant / reflect."""
    win_length, hop = _framing(n_fft, hop_length, win_length)
    if pad_mode not in ("constant", "reflect"):
        raise ValueError("pad_mode")
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError("mono")
    if not np.all(np.isfinite(y)):
        raise ValueError("audio buffer is not finite everywhere")
    T = n_frames(y.size, n_fft, hop, center, pad_mode)
    if T is None:
        raise ValueError("clip too short")
    dt = np.float32 if f32 else np.float64
    w = get_window(window, win_length, n_fft).astype(dt)
    yp = y.astype(dt)
    if center:
        yp = np.pad(yp, n_fft // 2, mode=pad_mode)
    fr = np.lib.stride_tricks.sliding_window_view(yp, n_fft)[::hop][:T]
    assert fr.shape[0] == T
    D = scipy.fft.rfft(fr * w, axis=-1)
    assert D.dtype == (np.complex64 if f32 else np.complex128)
    return np.asfortranarray(D.T)


def istft(D, hop_length=None, win_length=None, n_fft=None, window="hann", center=True, length=None, f32=False):
    """float64 samples (float32 values with f32).  ValueError for no frames."""
    D = np.asarray(D)
    n_fft = 2 * (D.shape[0] - 1) if n_fft is None else int(n_fft)
    win_length, hop = _framing(n_fft, hop_length, win_length)
    T = D.shape[1]
    if T == 0:
        raise ValueError("no frames")
    s = n_fft // 2 if center else 0
    nf = T if length is None else min(T, -(-(length + 2 * s) // hop))
    dt = np.float32 if f32 else np.float64
    w = get_window(window, win_length, n_fft).astype(dt)
    w2 = w * w
    Dk = np.array(D[:, :nf].T, np.complex64 if f32 else np.complex128)
    Dk[:, 0] = Dk[:, 0].real                                               # numpy's irfft ignores these imaginary parts
    Dk[:, -1] = Dk[:, -1].real
    seg = scipy.fft.irfft(Dk, n=n_fft, axis=-1) if nf else np.zeros((0, n_fft), dt)
    assert seg.dtype == dt
    seg = w * seg
    full = n_fft + hop * (nf - 1) if nf else 0
    acc, wss = np.zeros(full, dt), np.zeros(full, dt)
    for t in range(nf):
        acc[t * hop:t * hop + n_fft] += seg[t]
        wss[t * hop:t * hop + n_fft] += w2
    big = wss > TINY
    x = np.where(big, acc / np.where(big, wss, 1), acc)
    L = max(full - 2 * s, 0) if length is None else int(length)
    out = np.zeros(L, dt)
    k = max(min(L, full - s), 0)
    out[:k] = x[s:s + k]
    return out.astype(np.float64)


def make_clip(length, seed=0, sr=22050):
    """A vibrato tone, a second partial, a click and white noise: float32, peak below 1."""
    t = np.arange(length) / sr
    rng = np.random.default_rng(seed)
    y = 0.4 * np.sin(2 * np.pi * 220 * t + 3.0 * np.sin(2 * np.pi * 5 * t)) + 0.2 * np.sin(2 * np.pi * 1330 * t)
    y = y + 0.05 * rng.standard_normal(length)
    if length > 10:
        y[length // 3] += 0.3
    return y.astype(np.float32)
