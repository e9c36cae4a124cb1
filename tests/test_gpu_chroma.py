"""GPU checks of afx_chroma_batch / audio_feature_extraction_amd.feature / AudioFeatureExtractor.extract_timbre_features
against the restatement tests/chroma_ref.py.

Tolerances, with eps32 = 2^-23 and err32 = the float32 restatement's own largest error against the float64 one for the clip:
  chroma (values in [0, 1])   max|c - c64| <= 4 err32 + 32 eps32.  The second term covers the float32 FFT, which the
                              restatement rounds only once: about log2(2048) = 11 eps on a dominant bin, doubled by squaring,
                              with slack.  A wrong tuning step or a rolled row is an error of 1e-2 or more.
  mel                         the same bound in units of the clip's max(mel64): 4 err32 + 32 eps32 max(mel64), err32 absolute
  statistics                  |x - ref| <= 1e-5 (|ref_mean| + ref_std): float64 sums of values that each carry a few eps
The estimated tuning is pinned only on inputs tests/test_chroma_ref.py shows to be robust (tuning_is_robust)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chroma_ref as R
from tests.test_chroma_ref import pinned_inputs, unpinned_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -23
SMALL = (300, 700, 1500, 7500, 8000, 8500, 40001)      # T = 1, 2, 3, 15, 16, 17 (either side of the 16-frame tile), 79


@pytest.fixture(scope="module")
def N():
    from audio_feature_extraction_amd import _native
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return _native


@pytest.fixture(scope="module")
def plans(N):
    return {sr: N.Plan(N.Context(0), N.make_params(sr, 2048, 512, 13, 128, "hann")) for sr in (16000, 22050, 44100)}


def _pack(sigs):
    lengths = np.array([s.size for s in sigs], np.int64)
    offsets = np.zeros(len(sigs), np.int64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    return np.concatenate(sigs).astype(np.float32), offsets, lengths


@functools.lru_cache(maxsize=None)
def _cases():
    """(name, sr, signal, pinned)"""
    rng = np.random.default_rng(2)
    out = [(f"noise{n}", 22050, (0.5 * rng.standard_normal(n)).astype(np.float32), False) for n in SMALL]
    out += [(name, sr, y, True) for name, sr, y in pinned_inputs()]
    out += [(name, sr, y, False) for name, sr, y in unpinned_inputs()]
    t = np.arange(2 * 16000) / 16000.0
    out.append(("chirp16000", 16000, (0.4 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 900.0 * t * t))).astype(np.float32), False))
    return tuple(out)


def _by_rate():
    return {sr: [c for c in _cases() if c[1] == sr] for sr in (16000, 22050, 44100)}


@functools.lru_cache(maxsize=None)
def _spec(name):
    """the float64 and float32 power spectrograms of a case (computed once, shared, never modified)"""
    y = next(c[2] for c in _cases() if c[0] == name)
    S = R.power_spectrogram(y)
    S.setflags(write=False)
    S32 = S.astype(np.float32)
    S32.setflags(write=False)
    return S, S32


def _check_matrices(name, sr, tuning, chroma, mel, stats):
    S, S32 = _spec(name)
    c64, m64 = R.chroma_from(S, sr, tuning), R.mel_from(S, sr)
    ce = float(np.max(np.abs(R.chroma_from(S32, sr, tuning) - c64)))
    me = float(np.max(np.abs(R.mel_from(S32, sr) - m64)))
    assert chroma.shape == c64.shape and chroma.dtype == np.float32 and mel.shape == m64.shape and mel.dtype == np.float32
    cb, mb = 4 * ce + 32 * EPS32, 4 * me + 32 * EPS32 * float(np.max(m64))
    cr, mr = float(np.max(np.abs(chroma - c64))) / cb, float(np.max(np.abs(mel - m64))) / max(mb, 1e-300)
    ref = (np.mean(m64), np.std(m64), np.mean(c64), np.std(c64))
    sr_ = [abs(stats[k] - ref[k]) / max(1e-5 * (abs(ref[k - k % 2]) + ref[k - k % 2 + 1]), 1e-300) for k in range(4)]
    print(f"{name} tuning {tuning}: chroma {cr:.3f} mel {mr:.3f} stats {max(sr_):.3f} of the bound")
    assert cr <= 1.0, (name, tuning, "chroma", cr)
    assert mr <= 1.0, (name, tuning, "mel", mr)
    assert max(sr_) <= 1.0, (name, tuning, "stats", sr_)
    return cr, mr, max(sr_)


@pytest.mark.parametrize("tuning", [0.0, 0.46])
def test_given_tuning_matches_the_oracle(plans, tuning):
    worst = np.zeros(3)
    for sr, cases in _by_rate().items():
        out = plans[sr].chroma_batch(*_pack([c[2] for c in cases]), tuning=tuning, want_mel=True)
        assert (out["status"] == 0).all() and (out["tuning"] == tuning).all()
        for i, (name, _, _, _) in enumerate(cases):
            worst = np.maximum(worst, _check_matrices(name, sr, tuning, out["chroma"][i], out["mel"][i], out["stats"][i]))
    print("largest ratios to the bounds (chroma, mel, statistics):", worst)


def test_estimated_tuning_is_exact_on_robust_inputs(plans):
    for sr, cases in _by_rate().items():
        out = plans[sr].chroma_batch(*_pack([c[2] for c in cases]), store_hist=True)
        for i, (name, _, _, pinned) in enumerate(cases):
            if pinned:
                assert out["tuning"][i] == R.estimate_tuning(_spec(name)[0], sr), (name, out["tuning"][i], out["hist"][i][:2])
            if name == "nopeak22050":
                assert out["tuning"][i] == 0.0 and out["hist"][i][0] == 0


def test_estimate_is_consistent_on_every_input(plans):
    for sr, cases in _by_rate().items():
        packed = _pack([c[2] for c in cases])
        a = plans[sr].chroma_batch(*packed, store_hist=True)
        b = plans[sr].chroma_batch(*packed, tuning=a["tuning"])
        assert (a["status"] == 0).all()
        for i, (name, _, _, _) in enumerate(cases):
            np.testing.assert_array_equal(a["chroma"][i], b["chroma"][i], err_msg=name)
            peaks, kept, counts = a["hist"][i][0], a["hist"][i][1], a["hist"][i][2:]
            assert counts.sum() == kept and kept <= peaks, name
            k = int(np.argmax(counts)) if peaks else 50
            assert a["tuning"][i] == R.EDGES[k], (name, a["tuning"][i], k)
            if peaks:
                assert kept >= (peaks + 1) // 2, name          # at least the upper half sits at or above the median
            mx = a["chroma"][i].max(axis=0)
            assert np.all((mx == 1.0) | (np.abs(a["chroma"][i]).max(axis=0) == 0.0)), name


def _batch50():
    from audio_feature_extraction_amd.synth import make_clip
    sigs = [make_clip(i, 22050, 0.3 + 0.05 * (i % 7), speechy=bool(i % 2)) for i in range(50)]
    sigs[20] = sigs[20].copy()
    sigs[20][777] = np.nan
    sigs[30] = np.zeros(0, np.float32)
    return sigs


def _same(a, b, keys=("chroma", "mel")):
    for k in keys:
        for u, v in zip(a[k], b[k]):
            np.testing.assert_array_equal(u, v)
    for k in ("stats", "tuning", "hist", "status"):
        np.testing.assert_array_equal(a[k], b[k])


def test_failed_clips_are_isolated_and_runs_are_deterministic(plans, N):
    plan = plans[22050]
    sigs = _batch50()
    y, off, ln = _pack(sigs)
    a = plan.chroma_batch(y, off, ln, want_mel=True, store_hist=True)
    b = plan.chroma_batch(y, off, ln, want_mel=True, store_hist=True)
    assert a["status"][20] == N.CLIP_NONFINITE and a["status"][30] == N.CLIP_TOO_SHORT
    assert (np.delete(a["status"], [20, 30]) == 0).all()
    for i in (20, 30):
        assert np.isnan(a["stats"][i]).all() and not a["chroma"][i].any() and not a["mel"][i].any()
        assert a["chroma"][i].shape == (12, 1 + sigs[i].size // 512)
    assert np.isfinite(np.delete(a["stats"], [20, 30], axis=0)).all()
    _same(a, b)
    for i in (0, 19, 21, 29, 31, 49):
        solo = plan.chroma_batch(sigs[i], np.zeros(1, np.int64), np.array([sigs[i].size], np.int64), want_mel=True, store_hist=True)
        np.testing.assert_array_equal(solo["chroma"][0], a["chroma"][i])
        np.testing.assert_array_equal(solo["mel"][0], a["mel"][i])
        np.testing.assert_array_equal(solo["stats"][0], a["stats"][i])
        np.testing.assert_array_equal(solo["hist"][0], a["hist"][i])
        assert solo["tuning"][0] == a["tuning"][i]


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_chroma import _batch50, _pack
from audio_feature_extraction_amd import _native as N
plan = N.Plan(N.Context(0), N.make_params(22050, 2048, 512, 13, 128, "hann"))
y, off, ln = _pack(_batch50())
o = plan.chroma_batch(y, off, ln, want_mel=True, store_hist=True)
np.savez(sys.argv[2], chroma=np.concatenate([c.ravel() for c in o["chroma"]]), mel=np.concatenate([m.ravel() for m in o["mel"]]),
         stats=o["stats"], status=o["status"], tuning=o["tuning"], hist=o["hist"])
"""


def test_chunked_batch_equals_one_chunk(plans, tmp_path):
    y, off, ln = _pack(_batch50())
    ref = plans[22050].chroma_batch(y, off, ln, want_mel=True, store_hist=True)
    env = dict(os.environ, AFX_TEST_CHROMA_BUDGET="400000")      # a few clips per chunk
    dst = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=300)
    z = np.load(dst)
    np.testing.assert_array_equal(z["status"], ref["status"])
    np.testing.assert_array_equal(z["chroma"], np.concatenate([c.ravel() for c in ref["chroma"]]))
    np.testing.assert_array_equal(z["mel"], np.concatenate([m.ravel() for m in ref["mel"]]))
    np.testing.assert_array_equal(z["stats"], ref["stats"])
    np.testing.assert_array_equal(z["tuning"], ref["tuning"])
    np.testing.assert_array_equal(z["hist"], ref["hist"])


def test_s16_and_device_inputs_match_host_f32(plans, N):
    plan = plans[22050]
    rng = np.random.default_rng(4)
    q = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (5000, 12345, 700)]
    f = [x.astype(np.float32) / 32768.0 for x in q]
    y, off, ln = _pack(f)
    ref = plan.chroma_batch(y, off, ln, want_mel=True, store_hist=True)
    s16 = plan.chroma_batch(np.concatenate(q), off, ln, fmt=N.FMT_S16, want_mel=True, store_hist=True)
    dev = plan.device_buffer(y.nbytes)
    dev.upload(y)
    d = plan.chroma_batch(dev.ptr, off, ln, mem=N.MEM_DEVICE, want_mel=True, store_hist=True)
    dev.free()
    _same(s16, ref)
    _same(d, ref)


def test_preemphasis_flag_equals_preemphasised_input(plans, N):
    plan = plans[22050]
    y = (0.3 * np.random.default_rng(9).standard_normal(9000)).astype(np.float32)
    one = np.zeros(1, np.int64), np.array([y.size], np.int64)
    a = plan.chroma_batch(y, *one, flags=N.FLAG_PREEMPH, want_mel=True, store_hist=True)
    yp = np.ascontiguousarray(plan.preprocess(y)[0], np.float32)      # the plan's pre-emphasis (trim off: full span)
    b = plan.chroma_batch(yp, *one, want_mel=True, store_hist=True)
    _same(a, b)


def test_other_plan_shapes_and_flags_are_refused(plans, N):
    other = N.Plan(N.Context(0), N.make_params(22050, 1024, 256, 13, 128, "hann"))
    y = np.zeros(4096, np.float32)
    one = np.zeros(1, np.int64), np.array([y.size], np.int64)
    with pytest.raises(NotImplementedError):
        other.chroma_batch(y, *one)
    with pytest.raises(NotImplementedError):
        plans[22050].chroma_batch(y, *one, flags=N.FLAG_TRIM)


def test_feature_api(N):
    from audio_feature_extraction_amd import feature
    name, sr, y, _ = next(c for c in _cases() if c[0] == "octave22050")
    S = _spec(name)[0]
    c = feature.chroma_stft(y, sr)
    m = feature.melspectrogram(y, sr)
    T = 1 + y.size // 512
    assert c.shape == (12, T) and c.dtype == np.float32 and m.shape == (128, T) and m.dtype == np.float32
    t = feature.estimate_tuning(y, sr)
    assert type(t) is float and t == R.estimate_tuning(S, sr)
    c64, m64 = R.chroma_from(S, sr), R.mel_from(S, sr)
    S32 = _spec(name)[1]
    assert np.max(np.abs(c - c64)) <= 4 * np.max(np.abs(R.chroma_from(S32, sr) - c64)) + 32 * EPS32
    assert np.max(np.abs(m - m64)) <= 4 * np.max(np.abs(R.mel_from(S32, sr) - m64)) + 32 * EPS32 * np.max(m64)
    short = y[:700]
    cb = feature.chroma_stft_batch([y, short], sr)
    mb = feature.melspectrogram_batch([y, short], sr)
    np.testing.assert_array_equal(cb[0], c)
    np.testing.assert_array_equal(mb[0], m)
    assert cb[1].shape == (12, 2) and mb[1].shape == (128, 2)
    np.testing.assert_array_equal(feature.chroma_stft(y, sr, tuning=t), c)
    assert feature.chroma_stft(y[:1], sr).shape == (12, 1)            # one sample is enough


def test_timbre_features_match_the_oracle(N):
    from audio_feature_extraction_amd import AudioFeatureExtractor
    for sr, cases in _by_rate().items():
        mine = [c for c in cases if c[3]]
        fx = AudioFeatureExtractor(sr=sr)
        res = fx.extract_timbre_features_batch([c[2] for c in mine])
        for (name, _, y, _), d in zip(mine, res):
            assert list(d) == list(R.KEYS)
            assert all(type(v) is float for v in d.values())
            json.dumps(d)
            ref = R.timbre_features(y, sr)
            for mk, sk, tol in (("mel_energy_mean", "mel_energy_std", 1e-5), ("chroma_mean", "chroma_std", 1e-5), ("mfcc_mean", "mfcc_std", 1e-4)):
                bound = tol * (abs(ref[mk]) + ref[sk])
                print(f"{name}: {mk} {abs(d[mk] - ref[mk]) / bound:.3f} {sk} {abs(d[sk] - ref[sk]) / bound:.3f} of the bound")
                assert abs(d[mk] - ref[mk]) <= bound, (name, mk, d[mk], ref[mk])
                assert abs(d[sk] - ref[sk]) <= bound, (name, sk, d[sk], ref[sk])
        assert fx.extract_timbre_features(mine[0][2]) == res[0]
        with pytest.raises(ValueError):
            fx.extract_timbre_features(mine[0][2][:3000])
