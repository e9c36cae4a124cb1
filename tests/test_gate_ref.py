"""The float64 oracle of spectral gating (tests/gate_ref.py) against scipy and against answers known in advance.  CPU only."""
import numpy as np
import pytest
import scipy.signal

from tests import gate_ref as G


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_stft_and_istft_are_scipys(n_fft):
    hop = n_fft // 4
    x = np.concatenate([np.zeros(30000), G.make_clip(16000, length=7001).astype(np.float64), np.zeros(30000)])
    _, _, Z = scipy.signal.stft(x, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop, padded=False)
    X = G.stft(x, n_fft, hop)
    assert X.shape == Z.shape == (n_fft // 2 + 1, 1 + x.size // hop)
    assert np.abs(X - Z).max() <= 1e-15
    _, xi = scipy.signal.istft(Z, nfft=n_fft, nperseg=n_fft, noverlap=n_fft - hop)
    xo = G.istft(X, n_fft, hop)
    assert xo.shape == xi.shape == ((X.shape[1] - 1) * hop,)
    assert np.abs(xo - xi).max() <= 1e-14
    assert np.abs(xo - x[:xo.size]).max() <= 1e-14


def test_filter_sizes_taps_and_sum():
    assert G.smooth_sizes(16000, 1024, 256) == (16, 3)
    assert G.smooth_sizes(16000, 2048, 512) == (32, 1)
    assert G.smooth_sizes(22050, 1024, 256) == (11, 4)
    with pytest.raises(ValueError):
        G.smooth_sizes(8000, 2048, 512)
    for n_f, n_t in ((16, 3), (32, 1), (11, 4), (1, 1)):
        F = G.smoothing_filter(n_f, n_t)
        assert F.shape == (2 * n_f + 1, 2 * n_t + 1)
        assert abs(F.sum() - 1.0) <= 1e-15
        assert np.all(F > 0) and F[n_f, n_t] == F.max()
        assert np.abs(F - F[::-1, ::-1]).max() <= 1e-16               # symmetric to the rounding of linspace's two ramps


def test_prop_decrease_zero_returns_the_clip():
    """The non-stationary mask is smoothed before p enters, so p = 0 gives mask 1 exactly.  The stationary mask is hard p +
    (1 - p) = 1 *before* the smoothing, whose zero padding at the array's edges then pulls the lowest and highest n_f bins
    below 1: y comes back only with the smoothing off (n_f = n_t = 1)."""
    sr = 16000
    y = G.make_clip(sr)
    assert np.abs(G.reduce_noise(y, sr, prop_decrease=0.0) - y).max() <= 2.0 ** -24 * np.abs(y).max()
    off = dict(freq_mask_smooth_hz=sr / 512.0, time_mask_smooth_ms=16.0)
    assert G.smooth_sizes(sr, 1024, 256, 31.25, 16.0) == (1, 1)
    assert np.abs(G.reduce_noise(y, sr, stationary=True, prop_decrease=0.0, **off) - y).max() <= 2.0 ** -24 * np.abs(y).max()
    assert np.abs(G.reduce_noise(y, sr, stationary=True, prop_decrease=0.0) - y).max() > 1e-3


@pytest.mark.parametrize("stationary", [True, False])
def test_zeros_give_zeros(stationary):
    for f32 in (False, True):
        out = G.reduce_noise(np.zeros(3000, np.float32), 16000, stationary=stationary, f32=f32)
        assert out.dtype == np.float32 and out.shape == (3000,) and not out.any()


def test_digital_silence_and_nonfinite():
    y = G.make_clip(16000, silence=True, seed=1)
    for stationary in (True, False):
        assert np.all(np.isfinite(G.reduce_noise(y, 16000, stationary=stationary)))
    y[5] = np.inf
    assert not G.reduce_noise(y, 16000).any()
    with pytest.raises(NotImplementedError):
        G.reduce_noise(np.zeros(600001, np.float32), 16000)
    with pytest.raises(ValueError):
        G.reduce_noise(np.zeros(0, np.float32), 16000)


def test_stationary_white_noise_is_attenuated_by_about_one_minus_p():
    """Every bin's mask is at least 1 - p.  |X| of white noise is Rayleigh; in dB its mean lies 2.5 dB below and its std is
    5.57 dB, so thr sits 5.85 dB above the RMS level and a fraction exp(-10^0.585) = 0.021 of the bins passes: the smoothed
    mask averages (1 - p) + 0.021 p, 1.5 dB above 20 log10(1 - p) at p = 0.9.  Taken with 1.5 dB to either side, and never
    below the floor."""
    sr, p = 16000, 0.9
    y = (0.05 * np.random.default_rng(7).standard_normal(2 * sr)).astype(np.float32)
    out = G.reduce_noise(y, sr, stationary=True, prop_decrease=p).astype(np.float64)
    mid = slice(sr // 4, -sr // 4)
    att = 20 * np.log10(np.sqrt(np.mean(out[mid] ** 2)) / np.sqrt(np.mean(y[mid].astype(np.float64) ** 2)))
    floor = 20 * np.log10(1 - p)
    assert floor <= att <= floor + 3.0, att


@pytest.mark.parametrize("sr,n_fft", [(16000, 1024), (16000, 2048), (22050, 1024), (22050, 2048)])
def test_float32_form_against_float64_form(sr, n_fft):
    """The float32-faithful form rounds at seven places, each to half an ulp of a value of the clip's scale: it stays within
    a few 2^-24 of max|y|, and decides no bin of the test clips differently."""
    y = G.make_clip(sr)
    for stationary in (True, False):
        p64, p32 = {}, {}
        a = G.reduce_noise(y, sr, stationary=stationary, n_fft=n_fft, parts=p64)
        b = G.reduce_noise(y, sr, stationary=stationary, n_fft=n_fft, f32=True, parts=p32)
        err = np.abs(a.astype(np.float64) - b).max() / np.abs(y).max()
        assert 0 < err <= 16 * 2.0 ** -24, err
        if stationary:
            assert np.array_equal(p64["hard"], p32["hard"])
            assert np.abs(p64["thr"] - p32["thr"]).max() <= 1e-3


def test_overrides_follow_a_given_decision():
    sr = 16000
    y = G.make_clip(sr, length=3000)
    parts = {}
    a = G.reduce_noise(y, sr, stationary=True, parts=parts)
    assert np.array_equal(a, G.reduce_noise(y, sr, stationary=True, thresh=parts["thr"]))
    assert np.array_equal(a, G.reduce_noise(y, sr, stationary=True, hard_mask=parts["hard"]))
    assert not np.array_equal(a, G.reduce_noise(y, sr, stationary=True, hard_mask=~parts["hard"]))
    assert parts["hard"].shape == (513, G.n_frames(3000, 256))
