"""The oracle of the noise reducers and the aligner's preprocess (tests/denoise_ref.py) against properties that follow from
the reference's formulae alone.  CPU only."""
import numpy as np
import pytest

from tests import denoise_ref as D
from tests import hpss_ref as R


def _noise(n, sigma=0.1, seed=0):
    return sigma * np.random.default_rng(seed).standard_normal(n)


@pytest.mark.parametrize("n", [4096, 9000, 12345])
def test_beta_zero_is_the_istft_round_trip(n):
    y = _noise(n, seed=n)
    Lp = D.kept(n)
    out = D.spectral_subtraction(y, beta=0.0)
    assert out.shape == (n,) and Lp == 512 * (n // 512)
    np.testing.assert_allclose(out[:Lp], R.istft(R.stft(y), Lp), rtol=0, atol=1e-12)
    np.testing.assert_allclose(out[:Lp], y[:Lp], rtol=0, atol=1e-12)      # the window sum-square undoes the windows
    assert not out[Lp:].any()


def test_a_silent_lead_leaves_the_clip_unchanged():
    # frames 0 .. 9 end at padded sample 9 * 512 + 2048, i.e. before sample 5632 of the signal
    y = np.concatenate([np.zeros(5632), _noise(9000, 0.2, 3)])
    Lp = D.kept(y.size)
    assert not np.abs(R.stft(y))[:, :10].any()
    for f32 in (False, True):
        s = D.spectral_subtraction(y, beta=1.0, f32=f32)
        w = D.wiener(y, f32=f32)
        assert np.isfinite(s).all() and np.isfinite(w).all()
        tol = 2e-6 if f32 else 1e-12
        np.testing.assert_allclose(s[:Lp], y[:Lp], rtol=0, atol=tol)
        # P / (P + eps): a bin loses |X| eps / (|X|^2 + eps) <= sqrt(eps) / 2 = 7.5e-9
        np.testing.assert_allclose(w[:Lp], y[:Lp], rtol=0, atol=tol + 1e-7)
        assert not s[Lp:].any() and not w[Lp:].any()
        assert not s[:4096].any() and not w[:4096].any()                 # 0 / (0 + 0 + eps) = 0, never NaN


def test_heavy_subtraction_of_stationary_noise_is_silence():
    y = _noise(20000, 0.1, 5)
    for f32 in (False, True):
        out = D.spectral_subtraction(y, beta=50.0, f32=f32)
        assert out.shape == y.shape and not out.any()


def test_noise_frames_beyond_the_clip_use_every_frame():
    y = _noise(1500, seed=8)                                              # T = 3
    np.testing.assert_array_equal(D.spectral_subtraction(y, 1.0, 3), D.spectral_subtraction(y, 1.0, 10))
    np.testing.assert_array_equal(D.wiener(y, 3), D.wiener(y, 64))


@pytest.mark.parametrize("n", [0, 1, 511])
def test_clips_below_one_hop_are_silence(n):
    y = np.full(n, 0.25)
    for f32 in (False, True):
        for out in (D.spectral_subtraction(y, f32=f32), D.wiener(y, f32=f32)):
            assert out.shape == (n,) and not out.any()
            assert out.dtype == (np.float32 if f32 else np.float64)


def _rule(d, speech, fl, hop):
    """the issue's statement of the copy loop, sample by sample"""
    keep = np.zeros(d.size, bool)
    for j in range(d.size):
        for i in range(speech.size):
            if speech[i] and i * hop <= j < i * hop + fl and i * hop + fl <= d.size:
                keep[j] = True
    return keep


def test_vad_windows_are_uncentred_and_stop_at_the_end():
    sr, Lp = 22050, 512 * 20
    fl, hop, F = D.vad_frames(Lp, sr)
    assert (fl, hop) == (551, 220) and F == 1 + (Lp + 550 - 551) // 220 == 47     # odd fl: 2 (fl // 2) = fl - 1
    d = np.zeros(Lp)
    d[3000:5000] = 1.0
    d[9900:] = 1.0
    v = D.vad(d, sr)
    assert v["e"].shape == (F,) and v["speech"].shape == (F,)
    # frame i is centred on i hop: e[i]^2 is the share of ones in [i hop - 275, i hop + 276)
    np.testing.assert_allclose(v["e"][16], 1.0, atol=1e-12)             # 3245 .. 3796, inside the burst
    np.testing.assert_allclose(v["e"][13] ** 2, (2860 + 276 - 3000) / 551.0, atol=1e-12)
    assert v["thr"] == pytest.approx(0.5 * v["e"].mean(), rel=1e-12)
    i0 = int(np.flatnonzero(v["speech"])[0])
    assert v["e"][i0] > v["thr"] >= v["e"][i0 - 1]
    # the copy window of frame i0 starts at i0 hop, not at the frame's own start i0 hop - 275
    assert v["mask"][i0 * hop] and not v["mask"][:i0 * hop].any()
    assert i0 * hop - 275 < 3000                                          # the frame itself reaches further back
    # the last frames are speech, but a window that would pass L' copies nothing: 44 * 220 + 551 = 10231 is the last to fit
    assert v["speech"][45] and v["speech"][46] and v["speech"][44]
    assert v["mask"][10230] and not v["mask"][10231:].any()
    np.testing.assert_array_equal(v["mask"], _rule(d, v["speech"], fl, hop))
    np.testing.assert_array_equal(v["out"], np.where(v["mask"], d, 0.0))


def test_preprocess_alignment_chain():
    from audio_feature_extraction_amd.synth import make_clip
    sr = 16000
    y = make_clip(4, sr, 1.0, speechy=True)
    p = D.preprocess_alignment(y, sr)
    assert p["out"].shape == (D.kept(y.size),)
    assert p["gain"] == pytest.approx(0.1 / (np.sqrt(np.mean(y.astype(np.float64) ** 2)) + 1e-6), rel=1e-12)
    np.testing.assert_array_equal(p["d"], D.spectral_subtraction(p["scaled"], 1.0, 10)[:D.kept(y.size)])
    fl, hop, F = D.vad_frames(D.kept(y.size), sr)
    assert (fl, hop) == (400, 160) and p["e"].size == F == 1 + D.kept(y.size) // 160
    q = D.preprocess_alignment(y, sr, f32=True)
    assert q["out"].dtype == np.float32 and abs(q["gain"] - p["gain"]) <= 1e-6 * p["gain"]
