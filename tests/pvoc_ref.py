"""Oracle of librosa-style ``phase_vocoder`` / ``effects.time_stretch`` (librosa 0.11), restated with numpy (DESIGN.md
section 27 is the definition; librosa is not installed, so parity with it is unpinned).  The transforms come from
tests/stft_ref.py.  Two forms of the vocoder, both walking time column by column as librosa's loop does:

* ``f32=False``: float64 magnitudes and phases on the complex64 input, the truth;
* ``f32=True``: the device-faithful form -- float32 magnitudes (|c| = sqrt(re re + im im), the weights float32(1 - a) and
  float32(a), two products and a sum, each rounded once), float64 phases.  Its distance from the float64 form is the
  yardstick the device's tolerance is a multiple of.

``angles32=True`` is the form the definition rejects (float32 angles and accumulator), kept to show why.
"""
import numpy as np

from tests import stft_ref as R

TWO_PI = 2.0 * np.pi


def steps(T, rate):
    """(T_out, j, a): T_out = ceil(T / rate) in float64, s_t = float64(t) * rate, j = floor(s_t), a = s_t - j."""
    T_out = int(np.ceil(np.float64(T) / np.float64(rate)))
    s = np.arange(T_out, dtype=np.float64) * np.float64(rate)
    j = np.floor(s)
    return T_out, j.astype(np.int64), s - j


def check_rate(rate):
    rate = float(rate)
    if not (np.isfinite(rate) and rate > 0):
        raise ValueError("rate must be finite and > 0")
    return rate


def _framing(bins, hop_length, n_fft):
    n_fft = 2 * (bins - 1) if n_fft is None else int(n_fft)
    return n_fft, n_fft // 4 if hop_length is None else int(hop_length)


def _vocode(D, rate, hop, n_fft, f32=False, angles32=False):
    """The column loop on a complex64 or complex128 spectrum -> complex128 [bins, T_out], not yet rounded."""
    bins, T = D.shape
    T_out, J, A = steps(T, rate)
    Dp = np.concatenate([D, np.zeros((bins, 2), D.dtype)], axis=1)             # columns T and T + 1 are +0 + 0i
    re, im = Dp.real, Dp.imag
    if f32:
        assert re.dtype == np.float32
        mag = np.sqrt(re * re + im * im)                                      # float32, each operation rounded once
        assert mag.dtype == np.float32
    else:
        mag = np.hypot(re.astype(np.float64), im.astype(np.float64))
    adt = np.float32 if angles32 else np.float64
    ang = np.arctan2(im.astype(np.float64), re.astype(np.float64)).astype(adt)
    phi = (TWO_PI * hop * np.arange(bins, dtype=np.float64) / n_fft).astype(adt)
    two_pi = adt(TWO_PI)
    acc = ang[:, 0].copy()
    out = np.zeros((bins, T_out), np.complex128, order="F")
    for t in range(T_out):
        j, a = int(J[t]), A[t]
        if f32:
            m = np.float32(1.0 - a) * mag[:, j] + np.float32(a) * mag[:, j + 1]
            assert m.dtype == np.float32
        else:
            m = (1.0 - a) * mag[:, j] + a * mag[:, j + 1]
        ph, m = acc.astype(np.float64), m.astype(np.float64)
        out[:, t] = m * np.cos(ph) + 1j * (m * np.sin(ph))
        d = ang[:, j + 1] - ang[:, j] - phi
        acc = acc + phi + (d - two_pi * np.rint(d / two_pi))
        assert acc.dtype == adt
    return out


def phase_vocoder(D, *, rate, hop_length=None, n_fft=None, f32=False, angles32=False, exact=False):
    """[bins, T_out] complex64 in Fortran order (``exact``: complex128, the result before that last rounding, which is what
    the yardsticks are measured against).  ValueError for a bad rate, no frames, or a NaN / inf bin (the stated deviation:
    librosa lets it poison its row)."""
    rate = check_rate(rate)
    D = np.asarray(D, np.complex64)
    n_fft, hop = _framing(D.shape[0], hop_length, n_fft)
    if D.shape[1] == 0:
        raise ValueError("no frames")
    if not (np.all(np.isfinite(D.real)) and np.all(np.isfinite(D.imag))):
        raise ValueError("not finite everywhere")
    P = _vocode(D, rate, hop, n_fft, f32, angles32)
    return P if exact else np.asfortranarray(P.astype(np.complex64))


def stretch_length(length, rate):
    """int(rint(length / rate)) in float64, halves to even: Python's round, as librosa uses it."""
    return int(round(length / check_rate(rate)))


def time_stretch(y, *, rate, n_fft=2048, hop_length=None, win_length=None, window="hann", center=True, pad_mode="constant",
                 f32=False):
    """float64 samples: istft(phase_vocoder(stft(y)), length=round(len / rate)).  With f32 every stage is its float32-
    faithful form (complex64 between them); without, everything is float64 and complex128."""
    rate = check_rate(rate)
    y = np.asarray(y)
    D = R.stft(y, n_fft, hop_length, win_length, window, center, pad_mode, f32=f32)
    hop = (n_fft if win_length is None else win_length) // 4 if hop_length is None else hop_length
    P = _vocode(D, rate, hop, n_fft, f32=f32)
    if f32:
        P = P.astype(np.complex64)
    return R.istft(P, hop_length, win_length, n_fft, window, center, length=stretch_length(y.size, rate), f32=f32)
