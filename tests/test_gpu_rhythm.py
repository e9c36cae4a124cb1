"""GPU checks of afx_rhythm_batch / audio_feature_extraction_amd.onset / feature.tempogram / feature.tempo /
AudioFeatureExtractor.extract_rhythm_features against the restatement tests/rhythm_ref.py.

Tolerances, with eps32 = 2^-23; every err32 is the error of a float32 restatement against the float64 one on the same input,
and the factor 4 in front of it is tests/parity.py's rule:
  envelope      max|env - env64| <= 4 err32 + 4 ulp32(max|dB64|).  err32: the restatement whose STFT is a float32 FFT and
                whose dtypes behind it are librosa's.  The second term is the rounding of a float32 dB value of the clip's size.
  tempogram     against the float64 restatement applied to the envelope the GPU returned (the stage alone):
                max|tg - tg64| <= 4 err32 + 16 eps32 on values in [-1, 1]; err32: the restatement with a float32 FFT
                autocorrelation on that envelope.  Lag 0 of every non-zero frame is exactly 1.
  acmean        the same bound, with err32 the float32 restatement's error of the mean tempogram
  statistics    |x - ref64| <= 4 (the float32 restatement's error of that statistic) + 1e-6 (|mean| + std)
  decision      out_lag is the first maximum of log1p(1e6 acmean) + logprior recomputed in float64 from the GPU's own acmean,
                and out_tempo == bpm[lag]: exactly, on every input.  The tempo equals the restatement's on every input of
                tests/test_rhythm_ref.pinned_inputs (shown robust there); it is left open only on unpinned_inputs and on the
                noise clips of the shape cases, whose arg-max a float32 path may move (tempo_is_robust's margin)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rhythm_ref as R
from tests.test_rhythm_ref import pinned_inputs, unpinned_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -23
# frames of the shape cases at 22050 Hz: the degenerate ones, either side of the 16-frame tile and of four tiles, either
# side of win / 2 = 172 (where the right ramp of the padding starts to reach frame 0), and win + 1
SHAPES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 171, 172, 173, 345)


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
    out = [(f"noise_T{T}", 22050, (0.5 * rng.standard_normal((T - 1) * 512 + 100)).astype(np.float32), False) for T in SHAPES]
    out += [(name, sr, y, True) for name, sr, y in pinned_inputs()]
    out += [(name, sr, y, False) for name, sr, y in unpinned_inputs()]
    t = np.arange(2 * 16000) / 16000.0
    out.append(("chirp16000", 16000, (0.4 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 900.0 * t * t))).astype(np.float32), False))
    out.append(("noise44100", 44100, (0.3 * rng.standard_normal(44100)).astype(np.float32), False))
    t = np.arange(44100) / 44100.0
    gate = (np.floor(t / 0.21) % 2 == 0).astype(np.float64)
    out.append(("gated44100", 44100, (0.4 * gate * np.sin(2 * np.pi * 660.0 * t)).astype(np.float32), False))
    return tuple(out)


def _by_rate():
    return {sr: [c for c in _cases() if c[1] == sr] for sr in (16000, 22050, 44100)}


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the float64 envelope of a case, the float32-FFT restatement's, and the clip's largest |dB| (computed once, shared,
    never modified)"""
    _, sr, y, _ = next(c for c in _cases() if c[0] == name)
    e64, e32 = R.onset_strength(y, sr), R.onset_strength(y, sr, "fft32")
    e64.setflags(write=False)
    e32.setflags(write=False)
    return e64, e32, R.max_abs_db(y, sr)


@pytest.fixture(scope="module")
def runs(plans):
    """every case through afx_rhythm_batch once, one batch per rate, everything stored"""
    out = {}
    for sr, cases in _by_rate().items():
        out[sr] = plans[sr].rhythm_batch(*_pack([c[2] for c in cases]), want_tempogram=True, want_acmean=True)
        assert (out[sr]["status"] == 0).all()
    return out


def test_rates_have_three_clips_and_a_click_track():
    by = _by_rate()
    assert len(by[16000]) == 3 and len(by[44100]) == 3
    assert any(c[0].startswith("clicks") for c in by[16000]) and any(c[0].startswith("clicks") for c in by[44100])
    assert [1 + c[2].size // 512 for c in by[22050][:len(SHAPES)]] == list(SHAPES)


def test_envelope_and_statistics_match_the_oracle(runs):
    worst = np.zeros(2)
    for sr, cases in _by_rate().items():
        out = runs[sr]
        for i, (name, _, y, _) in enumerate(cases):
            e64, e32, maxdb = _ref(name)
            env = out["env"][i]
            assert env.shape == e64.shape and env.dtype == np.float32 and not env[:3].any()
            bound = 4 * float(np.max(np.abs(e32 - e64))) + 4 * float(np.spacing(np.float32(maxdb)))
            er = float(np.max(np.abs(env - e64))) / bound
            ref = (np.mean(e64), np.std(e64))
            s32 = (np.mean(e32, dtype=np.float64), np.std(e32, dtype=np.float64))
            sr_ = [abs(out["stats"][i][k] - ref[k]) / max(4 * abs(s32[k] - ref[k]) + 1e-6 * (abs(ref[0]) + ref[1]), 1e-300) for k in range(2)]
            print(f"{name}: envelope {er:.3f} statistics {max(sr_):.3f} of the bound (max env {e64.max():.3f}, max |dB| {maxdb:.1f})")
            if not e64.any():
                assert not env.any() and out["stats"][i][0] == 0.0 and out["stats"][i][1] == 0.0, name
                continue
            assert er <= 1.0, (name, "envelope", er)
            assert max(sr_) <= 1.0, (name, "statistics", sr_)
            worst = np.maximum(worst, (er, max(sr_)))
    print("largest ratios to the bounds (envelope, statistics):", worst)


def test_tempogram_and_acmean_match_the_oracle_on_the_returned_envelope(runs):
    worst = np.zeros(2)
    for sr, cases in _by_rate().items():
        out = runs[sr]
        win = R.tempo_table(sr)[0]
        for i, (name, _, y, _) in enumerate(cases):
            env, tg, am = out["env"][i], out["tempogram"][i], out["acmean"][i]
            assert tg.shape == (win, env.size) and tg.dtype == np.float32 and am.shape == (win,) and am.dtype == np.float64
            tg64, tg32 = R.tempogram(env, sr), R.tempogram(env, sr, f32=True)
            tb = 4 * float(np.max(np.abs(tg32 - tg64))) + 16 * EPS32
            ab = 4 * float(np.max(np.abs(np.mean(tg32, axis=1, dtype=np.float64) - np.mean(tg64, axis=1)))) + 16 * EPS32
            tr, ar = float(np.max(np.abs(tg - tg64))) / tb, float(np.max(np.abs(am - np.mean(tg64, axis=1)))) / ab
            print(f"{name}: tempogram {tr:.3f} acmean {ar:.3f} of the bound")
            assert tr <= 1.0, (name, "tempogram", tr)
            assert ar <= 1.0, (name, "acmean", ar)
            live = np.abs(tg).max(axis=0) > 0
            assert np.all(tg[0, live] == 1.0) and np.abs(tg).max() <= 1.0, name
            assert np.array_equal(live, np.abs(tg64).max(axis=0) > 0), name
            worst = np.maximum(worst, (tr, ar))
    print("largest ratios to the bounds (tempogram, acmean):", worst)


def test_decision_is_exact_on_every_input(runs):
    for sr, cases in _by_rate().items():
        out = runs[sr]
        _, _, bpm, logprior = R.tempo_table(sr)
        for i, (name, _, _, _) in enumerate(cases):
            if not out["env"][i].any():
                assert out["lag"][i] == 0 and out["tempo"][i] == 0.0, name
                continue
            lag = int(np.argmax(np.log1p(1e6 * out["acmean"][i]) + logprior))
            assert out["lag"][i] == lag and out["tempo"][i] == bpm[lag], (name, out["lag"][i], lag)


def test_tempo_equals_the_oracle_on_every_pinned_input(runs):
    checked = set()
    for sr, cases in _by_rate().items():
        for i, (name, _, y, pinned) in enumerate(cases):
            if pinned:
                assert runs[sr]["tempo"][i] == R.tempo(y, sr), (name, runs[sr]["tempo"][i], runs[sr]["lag"][i])
                checked.add(name)
    assert checked == {c[0] for c in pinned_inputs()}
    left = {c[0] for c in _cases()} - checked                       # unpinned_inputs, the noise of the shape cases, the extra clips
    assert left == {c[0] for c in _cases() if not c[3]} and {c[0] for c in unpinned_inputs()} <= left
    for name in ("noise_T1", "noise_T2", "noise_T3"):              # three frames or fewer: nothing to decide
        i = [c[0] for c in _by_rate()[22050]].index(name)
        assert runs[22050]["tempo"][i] == 0.0 and runs[22050]["lag"][i] == 0


def _batch():
    """short synthetic clips with an all-zero, a NaN and an empty clip inside, and clip 0 again at the end"""
    from audio_feature_extraction_amd.synth import make_clip
    sigs = [pinned_inputs()[0][2]] + [make_clip(i, 22050, 0.3 + 0.05 * (i % 7), speechy=bool(i % 2)) for i in range(1, 14)]
    sigs[4] = np.zeros(9000, np.float32)
    sigs[7] = sigs[7].copy()
    sigs[7][777] = np.nan
    sigs[10] = np.zeros(0, np.float32)
    return sigs + [sigs[0]]


def _flat(o):
    return {"env": np.concatenate(o["env"]), "tempogram": np.concatenate([t.ravel() for t in o["tempogram"]]),
            "acmean": o["acmean"], "tempo": o["tempo"], "lag": o["lag"], "stats": o["stats"], "status": o["status"]}


def test_failed_clips_are_isolated_and_runs_are_deterministic(plans, N):
    plan = plans[22050]
    sigs = _batch()
    a = plan.rhythm_batch(*_pack(sigs), want_tempogram=True, want_acmean=True)
    b = plan.rhythm_batch(*_pack(sigs), want_tempogram=True, want_acmean=True)
    for k, v in _flat(a).items():
        np.testing.assert_array_equal(v, _flat(b)[k], err_msg=k)
    assert a["status"][7] == N.CLIP_NONFINITE and a["status"][10] == N.CLIP_TOO_SHORT
    assert (np.delete(a["status"], [7, 10]) == 0).all()
    assert a["tempo"][4] == 0.0 and a["lag"][4] == 0 and not a["stats"][4].any() and not a["env"][4].any()      # digital silence
    for i in (7, 10):
        assert np.isnan(a["tempo"][i]) and np.isnan(a["stats"][i]).all() and a["lag"][i] == 0
        assert not a["env"][i].any() and not a["tempogram"][i].any() and not a["acmean"][i].any()
        assert a["env"][i].shape == (1 + sigs[i].size // 512,) and a["tempogram"][i].shape == (344, 1 + sigs[i].size // 512)
    assert np.isfinite(np.delete(a["tempo"], [7, 10])).all() and np.isfinite(np.delete(a["stats"], [7, 10], axis=0)).all()
    last = len(sigs) - 1
    for k in ("env", "tempogram", "acmean", "tempo", "lag", "stats"):                  # the repeated clip
        np.testing.assert_array_equal(a[k][0], a[k][last], err_msg=k)
    for i in range(len(sigs) - 1):
        if i in (7, 10):
            continue
        solo = plan.rhythm_batch(sigs[i], np.zeros(1, np.int64), np.array([sigs[i].size], np.int64), want_tempogram=True, want_acmean=True)
        for k in ("env", "tempogram", "acmean", "tempo", "lag", "stats"):
            np.testing.assert_array_equal(solo[k][0], a[k][i], err_msg=f"{k} of clip {i}")


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_rhythm import _batch, _flat, _pack
from audio_feature_extraction_amd import _native as N
plan = N.Plan(N.Context(0), N.make_params(22050, 2048, 512, 13, 128, "hann"))
np.savez(sys.argv[2], **_flat(plan.rhythm_batch(*_pack(_batch()), want_tempogram=True, want_acmean=True)))
"""


def test_chunked_batch_equals_one_chunk(plans, tmp_path):
    """a budget of 400 kB holds three of the short clips (about 100 kB of workspace each, tempogram included) and neither
    click track (2 MB), so the fifteen clips take at least five chunks"""
    ref = _flat(plans[22050].rhythm_batch(*_pack(_batch()), want_tempogram=True, want_acmean=True))
    env = dict(os.environ, AFX_TEST_RHYTHM_BUDGET="400000")
    dst = str(tmp_path / "chunked.npz")
    subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=150)
    z = np.load(dst)
    for k, v in ref.items():
        np.testing.assert_array_equal(z[k], v, err_msg=k)


def test_s16_device_input_and_preemphasis(plans, N):
    plan = plans[22050]
    rng = np.random.default_rng(4)
    q = [rng.integers(-20000, 20000, n).astype(np.int16) for n in (5000, 12345, 700)]
    f = [x.astype(np.float32) / 32768.0 for x in q]
    y, off, ln = _pack(f)
    ref = _flat(plan.rhythm_batch(y, off, ln, want_tempogram=True, want_acmean=True))
    s16 = _flat(plan.rhythm_batch(np.concatenate(q), off, ln, fmt=N.FMT_S16, want_tempogram=True, want_acmean=True))
    dev = plan.device_buffer(y.nbytes)
    dev.upload(y)
    d = _flat(plan.rhythm_batch(dev.ptr, off, ln, mem=N.MEM_DEVICE, want_tempogram=True, want_acmean=True))
    dev.free()
    one = np.zeros(1, np.int64), np.array([f[1].size], np.int64)
    pre = _flat(plan.rhythm_batch(f[1], *one, flags=N.FLAG_PREEMPH, want_tempogram=True, want_acmean=True))
    yp = np.ascontiguousarray(plan.preprocess(f[1])[0], np.float32)
    given = _flat(plan.rhythm_batch(yp, *one, want_tempogram=True, want_acmean=True))
    for k, v in ref.items():
        np.testing.assert_array_equal(s16[k], v, err_msg=k)
        np.testing.assert_array_equal(d[k], v, err_msg=k)
        np.testing.assert_array_equal(pre[k], given[k], err_msg=k)


def test_other_plan_shapes_and_flags_are_refused(plans, N):
    y = np.zeros(4096, np.float32)
    one = np.zeros(1, np.int64), np.array([y.size], np.int64)
    for params in (N.make_params(22050, 1024, 256, 13, 128, "hann"), N.make_params(22050, 2048, 512, 13, 128, "hamming"),
                   N.make_params(50000, 2048, 512, 13, 128, "hann")):
        with pytest.raises(NotImplementedError):
            N.Plan(N.Context(0), params).rhythm_batch(y, *one)
    with pytest.raises(NotImplementedError):
        plans[22050].rhythm_batch(y, *one, flags=N.FLAG_TRIM)


def test_python_api(N, runs):
    from audio_feature_extraction_amd import AudioFeatureExtractor, feature, onset
    cases = _by_rate()[22050]
    i = [c[0] for c in cases].index("clicks90_22050")
    name, sr, y, _ = cases[i]
    T = 1 + y.size // 512
    e = onset.onset_strength(y, sr)
    assert e.shape == (T,) and e.dtype == np.float32
    np.testing.assert_array_equal(e, runs[sr]["env"][i])
    t = feature.tempo(y, sr)
    assert t.shape == (1,) and t.dtype == np.float64 and t[0] == R.tempo(y, sr) == runs[sr]["tempo"][i]
    tg = feature.tempogram(y, sr)
    assert tg.shape == (344, T) and tg.dtype == np.float32
    np.testing.assert_array_equal(tg, runs[sr]["tempogram"][i])
    short = y[:700]
    eb, tb, gb = onset.onset_strength_batch([y, short], sr), feature.tempo_batch([y, short], sr), feature.tempogram_batch([y, short], sr)
    np.testing.assert_array_equal(eb[0], e)
    np.testing.assert_array_equal(gb[0], tg)
    assert eb[1].shape == (2,) and gb[1].shape == (344, 2) and tb.shape == (2,) and tb[0] == t[0] and tb[1] == 0.0
    assert onset.onset_strength(y[:1], sr).shape == (1,) and feature.tempo(y[:1], sr)[0] == 0.0       # one sample is enough
    fx = AudioFeatureExtractor(sr=sr)
    mine = [c for c in cases if c[3]] + [cases[3], cases[0]]
    res = fx.extract_rhythm_features_batch([c[2] for c in mine])
    for (nm, _, yy, pinned), d in zip(mine, res):
        assert list(d) == list(R.KEYS) and all(type(v) is float for v in d.values()), nm
        assert d == fx.extract_rhythm_features(yy), nm
        assert d["rhythm_regularity"] == d["onset_strength_std"] / (d["onset_strength_mean"] + 1e-8), nm
        if pinned:
            assert d["tempo"] == R.tempo(yy, sr), nm
    assert res[-1]["tempo"] == 0.0 and res[-1]["onset_strength_mean"] == 0.0                          # one frame
    bad = y.copy()
    bad[5] = np.inf
    with pytest.raises(ValueError):
        fx.extract_rhythm_features(bad)
    with pytest.raises(ValueError):
        fx.extract_rhythm_features(np.zeros(0, np.float32))
