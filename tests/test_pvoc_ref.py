"""The oracle of phase_vocoder / time_stretch (tests/pvoc_ref.py) on its own: closed forms it must reproduce before anything
is compared against it.  CPU only."""
import numpy as np
import pytest

from tests import pvoc_ref as P
from tests import stft_ref as R

RATES = (1.0, 0.5, 2.0, 0.8, 1.25, 3.7, 1.0 / 3.0, 0.1, 7.0)


def _random_spectrum(bins, T, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((bins, T)) + 1j * rng.standard_normal((bins, T))).astype(np.complex64)


def test_steps_equal_aranges():
    for rate in RATES:
        for T in range(1, 200):
            want = np.arange(0, T, rate, dtype=np.float64)
            T_out, j, a = P.steps(T, rate)
            assert T_out == want.size, (T, rate)
            np.testing.assert_array_equal(j, np.floor(want).astype(np.int64))
            np.testing.assert_array_equal(a, want - np.floor(want))     # arange's start + t * step is t * rate for start 0
            assert j.max() <= T - 1 and a.min() >= 0 and a.max() < 1


@pytest.mark.parametrize("f32", [False, True])
def test_rate_one_returns_the_input_to_rounding(f32):
    for n_fft, hop, T in ((16, 4, 40), (1024, 256, 9), (2048, 441, 5)):
        D = _random_spectrum(n_fft // 2 + 1, T, seed=n_fft)
        out = P.phase_vocoder(D, rate=1.0, hop_length=hop, n_fft=n_fft, f32=f32)
        assert out.shape == D.shape and out.dtype == np.complex64 and out.flags.f_contiguous
        # |D| is kept to a float32 rounding or two; the phase is angle(D) plus a telescoping sum that wrap() keeps within
        # pi of it, so it is exact modulo 2 pi up to the float64 roundings of a few thousand radians
        top = np.abs(D).max(axis=0, keepdims=True)
        assert float((np.abs(out - D) / top).max()) < 4e-7


def test_a_stationary_bin_centred_tone_keeps_its_magnitude_and_advances_phi():
    n_fft, hop, k0, T = 16, 4, 3, 50
    phi = 2 * np.pi * hop * k0 / n_fft
    D = np.zeros((n_fft // 2 + 1, T), np.complex64)
    D[k0] = (0.5 * np.exp(1j * (phi * np.arange(T) + 0.3))).astype(np.complex64)
    for rate in RATES:
        for f32 in (False, True):
            out = P.phase_vocoder(D, rate=rate, hop_length=hop, n_fft=n_fft, f32=f32)
            T_out, j, _ = P.steps(T, rate)
            assert out.shape == (9, T_out)
            inside = j + 1 < T                                          # both columns lie in the clip
            assert not np.delete(out, k0, axis=0).any()
            np.testing.assert_allclose(np.abs(out[k0, inside]), 0.5, rtol=0, atol=1e-6)
            want = phi * np.arange(T_out) + 0.3
            err = np.angle(out[k0, inside] * np.exp(-1j * want[inside]))
            assert np.abs(err).max() < 1e-5, (rate, f32)


def test_a_zero_column_gives_a_zero_column_and_the_tail_fades():
    D = _random_spectrum(9, 12, seed=5)
    D[:, 4] = 0
    D[:, 5] = 0
    for f32 in (False, True):
        out = P.phase_vocoder(D, rate=0.5, hop_length=4, n_fft=16, f32=f32)
        assert out.shape[1] == 24
        assert not out[:, 8:11].any() and out[:, 7].all() and out[:, 11].all()   # steps 8, 9, 10 mix columns 4 and 5 only
        # the last column is mixed with column T, which is zero: step 23 is half of |D[:, 11]|
        np.testing.assert_allclose(np.abs(out[:, 23]), 0.5 * np.abs(D[:, 11]), rtol=1e-6)
    assert not P.phase_vocoder(np.zeros((9, 5), np.complex64), rate=0.8, hop_length=4, n_fft=16).any()


def test_float32_angles_would_not_hold_the_bound():
    """why the phases are float64: at a thousand steps of pi hop per step a float32 accumulator has an ulp of 0.125"""
    y = R.make_clip(40000, seed=1)
    D = R.stft(y, 2048, 512, f32=True)
    P64 = P.phase_vocoder(D, rate=0.8, hop_length=512, exact=True)
    top = np.abs(P64).max(axis=0, keepdims=True)
    dev = float((np.abs(P.phase_vocoder(D, rate=0.8, hop_length=512, f32=True) - P64) / top).max())
    a32 = float((np.abs(P.phase_vocoder(D, rate=0.8, hop_length=512, angles32=True) - P64) / top).max())
    assert dev < 2.5e-7 and a32 > 4 * dev, (dev, a32)


def test_errors_and_lengths():
    D = _random_spectrum(9, 4)
    for rate in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            P.phase_vocoder(D, rate=rate)
    with pytest.raises(ValueError):
        P.phase_vocoder(D[:, :0], rate=1.0)
    bad = D.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        P.phase_vocoder(bad, rate=1.0)
    assert [P.stretch_length(L, 2.0) for L in (1, 3, 5, 7)] == [0, 2, 2, 4]  # halves to even
    y = R.make_clip(9000)
    for rate in (0.8, 1.25, 2.0):
        x = P.time_stretch(y, rate=rate)
        assert x.size == round(9000 / rate) and np.all(np.isfinite(x))
    # rate 1 is the round trip of stft / istft, to the vocoder's rounding
    assert np.abs(P.time_stretch(y, rate=1.0) - y).max() < 1e-9
