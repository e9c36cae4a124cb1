"""CPU known answers of tests/beat_ref.py, the restatement afx_beat_batch and afx_beat_track_host are held to."""
import functools

import numpy as np
import pytest

from tests import beat_ref as B
from tests import rhythm_ref as R
from tests.test_rhythm_ref import pinned_inputs

RATES = (16000, 22050, 44100)


@functools.lru_cache(maxsize=None)
def pinned_envelopes():
    """(name, sr, float64 envelope, tempo) of every signal tests/test_gpu_beat.py pins the beats of end to end: the click
    tracks of test_rhythm_ref.pinned_inputs (the silence clip has no tempo and no beats)"""
    out = []
    for name, sr, y in pinned_inputs():
        env = R.onset_strength(y, sr)
        out.append((name, sr, env, R.tempo_from(env, sr)[0]))
    return tuple(out)


@pytest.mark.parametrize("sr", RATES)
def test_frames_per_beat_of_a_table_tempo_is_its_lag(sr):
    win, kmin, bpm, _ = R.tempo_table(sr)
    fps = sr / 512.0
    for lag in range(1, win):
        assert B.frames_per_beat(fps, bpm[lag]) == lag
    assert 1 <= kmin < win <= B.MAX_FPB


def test_round_is_half_to_even():
    assert [B.round_half_even(v) for v in (0.5, 1.5, 2.5, 3.5, 10.5, 11.5)] == [0, 2, 2, 4, 10, 12]
    assert B.frames_per_beat(43.0, 60 * 43.0 / 2.5) == 2          # lo of fpb 5 = round(2.5) = 2 by the same rule


@pytest.mark.parametrize("p", (2, 3, 22, 43))
def test_impulse_train_gives_beats_on_the_impulses(p):
    """impulses at 0, p, 2 p, ...; 2 p > T, == T and < T.  (Without the trim a last frame that tops its left neighbour can
    end the chain -- that is the tracker, not an error -- so the known answer is stated with the default trim.)"""
    fps = 22050 / 512.0
    for T in (2 * p - 1, 2 * p, 2 * p + 1, 5 * p + 3, 12 * p + 1):
        e = B.impulse_train(T, p, 0)
        for dtype in ("f64", "f32"):
            r = B.beat_track(e, fps, 60.0 * fps / p, dtype=dtype)
            assert r["fpb"] == p
            assert np.array_equal(r["beats"], np.flatnonzero(e)), (p, T, dtype)
        assert B.beats_are_robust(e, fps, 60.0 * fps / p)


def test_constant_envelope_terminates_without_dividing_by_zero():
    for dtype in ("f64", "f32"):
        for T in (2, 5, 64, 200):
            with np.errstate(divide="raise"):                        # the normalisation divides by std + tiny
                r = B.beat_track(np.ones(T, np.float32), 43.0, 120.0, dtype=dtype)
            assert r["fpb"] == 22 and r["beats"].size <= T
            assert np.all(np.diff(r["beats"]) > 0)


@pytest.mark.parametrize("T", (0, 1, 2, 3))
def test_no_beats(T):
    for dtype in ("f64", "f32"):
        assert B.beat_track(np.zeros(T), 43.0, 120.0, dtype=dtype)["beats"].size == 0
        assert B.beat_track(np.ones(T), 43.0, 0.0, dtype=dtype)["beats"].size == 0
    r = B.beat_track(np.arange(1.0, T + 1.0), 43.0, 120.0)
    if T < 2:
        assert r["beats"].size == 0 and r["cumscore"] is None     # one frame: librosa is undefined, ours is no beats
    else:
        assert r["cumscore"].shape == (T,)
    # a cumulative score without a local maximum (strictly falling) has no last beat
    assert B.last_beat(np.array([3.0, 2.0, 1.0])) == -1
    assert B.last_beat(np.array([1.0, 2.0, 3.0])) == 2            # frame T - 1 tops its left neighbour
    assert B.last_beat(np.array([5.0, 1.0, 1.0])) == -1           # frame 0 is never a maximum


def test_refusals():
    for bpm in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            B.beat_track(np.ones(8), 43.0, bpm)
    with pytest.raises(ValueError):
        B.beat_track(np.ones(8), 43.0, 60 * 43.0 / 769)           # fpb 769
    with pytest.raises(ValueError):
        B.beat_track(np.ones(8), 43.0, 60 * 43.0 / 0.4)           # fpb 0
    assert B.beat_track(np.ones(8), 43.0, 60 * 43.0 / 768)["fpb"] == 768


def test_frames_per_beat_one():
    e = np.random.default_rng(5).random(40).astype(np.float32)
    r = B.beat_track(e, 43.0, 60 * 43.0, trim=False)
    assert r["fpb"] == 1 and B.round_half_even(0.5) == 0
    # lo = 0: frame i is its own first candidate; cumscore[i] is still 0 then, so the first strict maximum is decided
    # among i (score -inf: log 0), i - 1 and i - 2
    assert np.all(r["backlink"] < np.arange(40))
    d = np.diff(r["beats"])
    assert np.all((d >= 1) & (d <= 2))


def test_local_score_is_numpy_convolve_same():
    rng = np.random.default_rng(11)
    for T, fpb in ((1, 1), (2, 3), (7, 3), (50, 22), (44, 22), (43, 22), (100, 43), (30, 43)):
        x = rng.standard_normal(T)
        w = B.beat_window(fpb)
        assert w.shape == (2 * fpb + 1,) and w[fpb] == 1.0
        full = np.convolve(x, w, "full")[fpb:fpb + T]             # "same" centred on the longer operand, stated for any T
        if T >= w.size:
            assert np.array_equal(full, np.convolve(x, w, "same"))
        np.testing.assert_allclose(B.local_score(x, fpb), full, rtol=0, atol=64 * 2.0 ** -53 * np.abs(x).sum())


@pytest.mark.parametrize("n", (1, 2, 4, 5, 9))
def test_trim_rule(n):
    rng = np.random.default_rng(n)
    s = rng.random(n) + 0.1
    sm = B.trim_smooth(s)
    if n >= 5:
        np.testing.assert_allclose(sm, np.convolve(s, B.HANN5, "same"), rtol=0, atol=4 * 2.0 ** -53 * 2 * s.max())
    want = np.array([0.5 * (s[j - 1] if j else 0.0) + s[j] + 0.5 * (s[j + 1] if j + 1 < n else 0.0) for j in range(n)])
    assert np.array_equal(sm, want)
    ls = np.zeros(100)
    beats = np.arange(n) * 10 + 3
    ls[beats] = s
    keep = np.flatnonzero(sm > 0.5 * np.sqrt(np.mean(sm ** 2)))
    assert keep.size and np.array_equal(B.trim_beats(beats, ls), beats[keep[0]:keep[-1] + 1])
    # weak first and last beats are cut; their strong neighbours' halves keep the next ones in
    if n == 5:
        ls[beats] = (0.01, 0.01, 1.0, 0.01, 0.01)
        assert np.array_equal(B.trim_beats(beats, ls), beats[1:4])
    ls[beats] = 0.0
    assert B.trim_beats(beats, ls).size == 0                      # nothing above the threshold: nothing kept


def test_beat_stats():
    assert B.beat_stats([], 43.0)[0] == 0 and np.isnan(B.beat_stats([5], 43.0)[1])
    n, m, s = B.beat_stats([10, 20, 40], 10.0)
    assert (n, m) == (3, 1.5) and s == 0.5


def test_pinned_inputs_are_robust_and_known():
    names = set()
    for name, sr, env, bpm in pinned_envelopes():
        fps = sr / 512.0
        if bpm == 0.0:
            assert B.beat_track(env, fps, bpm)["beats"].size == 0
            continue
        assert B.beats_are_robust(env, fps, bpm), name
        names.add(name)
        r = B.beat_track(env, fps, bpm)
        gaps = np.diff(r["beats"])
        assert r["beats"].size >= 5 and np.all(np.abs(gaps - r["fpb"]) <= 2), name
        if name == "clicks120_22050":
            assert r["fpb"] == 22 and list(r["beats"][:5]) == [22, 44, 66, 87, 109]
    for sr in RATES:
        assert any(n.endswith(str(sr)) for n in names)
    for bpm in (90, 120, 150):                                    # ten-second click tracks
        y = R.clicks(22050, bpm, seconds=10.0)
        env = R.onset_strength(y, 22050)
        assert B.beats_are_robust(env, 22050 / 512.0, R.tempo_from(env, 22050)[0]), bpm
