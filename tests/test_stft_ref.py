"""The oracle of stft / istft (tests/stft_ref.py) against closed forms and scipy's own STFT, and the pure-numpy helpers of
audio_feature_extraction_amd.core.spectrum.  CPU only."""
import numpy as np
import pytest
import scipy.signal

from audio_feature_extraction_amd.core import spectrum as S      # the front end whose contract the oracle restates
from tests import stft_ref as R


@pytest.fixture(autouse=True)
def _one_window_rule():
    """the oracle and the front end build the same table: what a test below says of one holds for what the device is given"""
    for n in (1024, 2048):
        assert np.array_equal(S._window("hann", None, n), R.get_window("hann", n, n).astype(np.float32))


@pytest.mark.parametrize("n", [1024, 2048])
def test_unit_impulse(n):
    y = np.zeros(n)
    y[5] = 1.0
    D = R.stft(y, n, n, window="boxcar", center=False)
    assert D.shape == (n // 2 + 1, 1) and D.dtype == np.complex128 and D.flags.f_contiguous
    want = np.exp(-2j * np.pi * np.arange(n // 2 + 1) * 5 / n)
    assert np.abs(D[:, 0] - want).max() <= 1e-13
    D32 = R.stft(y.astype(np.float32), n, n, window="boxcar", center=False, f32=True)
    assert D32.dtype == np.complex64 and np.abs(D32[:, 0] - want).max() <= 1e-6


@pytest.mark.parametrize("n", [1024, 2048])
def test_bin_centred_sinusoid(n):
    k0 = 37
    y = np.cos(2 * np.pi * k0 * np.arange(3 * n) / n)
    D = R.stft(y, n, n, center=False)                               # hann: n / 4 at k0, -n / 8 beside it, nothing else
    assert D.shape == (n // 2 + 1, 3)
    want = np.zeros(n // 2 + 1)
    want[k0], want[k0 - 1], want[k0 + 1] = n / 4, -n / 8, -n / 8
    assert np.abs(D - want[:, None]).max() <= 1e-9


@pytest.mark.parametrize("n,hop", [(1024, 256), (2048, 512), (1024, 160), (2048, 1024)])
def test_agrees_with_scipy_on_the_grid_both_define(n, hop):
    y = R.make_clip(9000, seed=1).astype(np.float64)
    _, _, Z = scipy.signal.stft(y, nperseg=n, noverlap=n - hop, window="hann", boundary="zeros", padded=False)
    D = R.stft(y, n, hop)                                           # center, constant: scipy's zero boundary
    w = scipy.signal.get_window("hann", n)
    assert D.shape == Z.shape == (n // 2 + 1, 1 + 9000 // hop)
    assert np.abs(D - Z * w.sum()).max() <= 1e-10 * np.abs(D).max()


@pytest.mark.parametrize("n", [1024, 2048])
@pytest.mark.parametrize("window,div", [("hann", 4), ("hann", 2), ("hamming", 4)])
def test_round_trip_in_float64(n, window, div):
    y = R.make_clip(3 * n + 123, seed=2).astype(np.float64)
    for pad_mode in ("constant", "reflect"):
        D = R.stft(y, n, n // div, window=window, pad_mode=pad_mode)
        x = R.istft(D, n // div, window=window, length=y.size)
        assert np.abs(x - y).max() <= 1e-12
    x = R.istft(R.stft(y, n, n // div, window=window), n // div, window=window)
    assert x.size == (y.size // (n // div)) * (n // div) and np.abs(x - y[:x.size]).max() <= 1e-12


def test_the_length_rule():
    n, hop = 1024, 256
    y = R.make_clip(5000, seed=3).astype(np.float64)
    D = R.stft(y, n, hop)
    T = D.shape[1]
    full = n + hop * (T - 1)
    nat = R.istft(D, hop)
    assert nat.size == full - n
    short = R.istft(D, hop, length=2000)                            # the frames dropped cover none of the samples kept
    assert short.size == 2000 and np.array_equal(short, nat[:2000])
    assert -(-(2000 + n) // hop) < T
    long_ = R.istft(D, hop, length=full + 300)
    assert long_.size == full + 300 and np.array_equal(long_[:nat.size], nat)
    assert not long_[full - n // 2:].any() and long_[nat.size:full - n // 2].any()
    x = R.istft(R.stft(y, n, hop, center=False), hop, center=False)
    assert x.size == n + hop * ((5000 - n) // hop)
    one = R.istft(D[:, :1], hop, center=False)                      # T = 1
    assert one.size == n
    with pytest.raises(ValueError):
        R.istft(D[:, :0], hop)


@pytest.mark.parametrize("f32", [False, True])
def test_the_tiny_rule_leaves_the_joints_undivided(f32):
    n = 1024
    y = R.make_clip(4 * n, seed=4)
    D = R.stft(y, n, n, f32=f32)                                    # hann at hop = n_fft: wss = 0 where the frames join
    x = R.istft(D, n, f32=f32, length=y.size)
    assert np.all(np.isfinite(x))
    joints = np.arange(n // 2, y.size, n)                           # sample 0 of every frame but the first
    assert not x[joints].any()
    w2 = np.tile(np.roll(scipy.signal.get_window("hann", n) ** 2, n // 2), 4)
    ok = w2 > 1e-4
    assert np.abs(x[ok] - y[ok]).max() <= (1e-3 if f32 else 1e-9)


def test_pad_center_and_window_tables():
    w = R.get_window("hann", 400, 1024)
    assert w.shape == (1024,) and not w[:312].any() and not w[712:].any()
    assert np.array_equal(w[312:712], scipy.signal.get_window("hann", 400, fftbins=True))
    assert np.array_equal(R.pad_center(np.ones(3), 8), [0, 0, 1, 1, 1, 0, 0, 0])
    arr = np.linspace(0.1, 1.0, 1024)
    assert np.array_equal(R.get_window(arr, 1024, 1024), arr)
    with pytest.raises(ValueError):
        R.get_window(arr, 400, 1024)
    assert np.array_equal(S._window("hann", 400, 1024), w.astype(np.float32))
    assert np.array_equal(S._window(arr, None, 1024), arr.astype(np.float32))


def test_refusals_and_frame_counts():
    y = R.make_clip(1024)
    for kw in (dict(center=False, n_fft=2048), dict(pad_mode="reflect", n_fft=2048), dict(pad_mode="wrap")):
        with pytest.raises(ValueError):
            R.stft(y, **kw)
    with pytest.raises(ValueError):
        R.stft(np.zeros(0))
    bad = y.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError):
        R.stft(bad)
    assert R.stft(y, 2048).shape == (1025, 3) and R.stft(y[:1], 2048).shape == (1025, 1)
    assert R.stft(y, 1024, 1, center=False).shape == (513, 1) and R.stft(y[:513], 1024, pad_mode="reflect").shape == (513, 3)
    ref = np.pad(y[:600].astype(np.float64), 512, mode="reflect")
    D = R.stft(y[:600], 1024, 100, window="boxcar", pad_mode="reflect")
    assert np.abs(D[:, 2] - np.fft.rfft(ref[200:1224])).max() <= 1e-10


def test_the_float32_form_loses_what_float32_loses():
    y = R.make_clip(6000, seed=5)
    for n in (1024, 2048):
        D64, D32 = R.stft(y, n), R.stft(y, n, f32=True)
        e = np.abs(D32 - D64).max() / np.abs(D64).max()
        assert 1e-9 < e < 1e-6
        Dc = D64.astype(np.complex64)
        x64, x32 = R.istft(Dc, length=y.size), R.istft(Dc, length=y.size, f32=True)
        assert 1e-9 < np.abs(x32 - x64).max() / np.abs(y).max() < 1e-6


def test_numpy_helpers_follow_librosa():
    from audio_feature_extraction_amd import amplitude_to_db, magphase, power_to_db
    rng = np.random.default_rng(0)
    D = (rng.standard_normal((5, 7)) + 1j * rng.standard_normal((5, 7))).astype(np.complex64)
    D[0, 0] = 0
    mag, ph = magphase(D)
    assert ph.dtype == np.complex64 and ph[0, 0] == 1 and np.abs(mag * ph - D).max() <= 1e-6
    assert np.allclose(magphase(D, power=2)[0], np.abs(D) ** 2)
    S = np.abs(D) ** 2
    db = power_to_db(S)
    want = 10 * np.log10(np.maximum(1e-10, S))
    assert np.allclose(db, np.maximum(want, want.max() - 80))
    assert power_to_db(S, ref=np.max).max() == 0.0 and power_to_db(S, ref=np.max).min() >= -80.0
    assert np.allclose(power_to_db(S, ref=2.0, top_db=None), want - 10 * np.log10(2.0))
    # amin is applied before top_db: a zero floors at amin, then at the maximum - top_db
    z = np.array([1.0, 0.0])
    assert np.array_equal(power_to_db(z, top_db=None), [0.0, -100.0]) and np.array_equal(power_to_db(z), [0.0, -80.0])
    a = amplitude_to_db(np.abs(D), ref=np.max)
    assert np.allclose(a, power_to_db(S, ref=S.max(), amin=1e-10)) and a.max() == 0.0
    assert np.array_equal(amplitude_to_db(z, top_db=None), [0.0, -100.0])
    for bad in (dict(amin=0.0), dict(top_db=-1.0)):
        with pytest.raises(ValueError):
            power_to_db(S, **bad)
