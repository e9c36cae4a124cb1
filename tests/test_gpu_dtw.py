"""GPU checks of afx_dtw_batch / sequence.dtw / AudioFeatureExtractor.align_* against the float64 oracle (tests/dtw_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dtw_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 300, 1000]
DIMS = [1, 7, 13, 39, 64, 65, 120, 128, 20]
BANDS = [None, 0.1, 0.25, 0.5]


@pytest.fixture(scope="module")
def seq():
    from audio_feature_extraction_amd import _native, sequence
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return sequence


def _int_case(rng, n, m, dim, zero=False):
    if zero:
        return np.zeros((dim, n), np.float32), np.zeros((dim, m), np.float32)
    return (rng.integers(-4, 5, size=(dim, n)).astype(np.float32), rng.integers(-4, 5, size=(dim, m)).astype(np.float32))


def _cases():
    rng = np.random.default_rng(2024)
    out = []
    for c in range(60):
        n, m = int(rng.choice(SIZES)), int(rng.choice(SIZES))
        out.append((c, n, m, DIMS[c % 8], BANDS[(c // 8) % len(BANDS)], c % 10 == 9))   # the first eight dims: ids as before
    out += [(60, 64, 64, 13, None, True), (61, 129, 65, 39, 0.25, True), (62, 1, 1, 1, None, False)]
    # dim 20 (librosa's n_mfcc default): the 24-wide instance, on both sides of a strip edge, with every band
    out += [(63, 65, 129, 20, None, False), (64, 129, 65, 20, 0.1, False), (65, 64, 300, 20, 0.25, False),
            (66, 300, 127, 20, 0.5, False), (67, 128, 128, 20, None, True), (68, 2, 63, 20, 0.25, False)]
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: "c%d-%dx%d-d%d-b%s%s" % (c[0], c[1], c[2], c[3], c[4], "-zero" if c[5] else ""))
def test_bit_exact_small_integers(seq, case):
    c, n, m, dim, band, zero = case
    X, Y = _int_case(np.random.default_rng(c), n, m, dim, zero)
    gc = band is not None
    D, steps, cost, wp, st = R.dtw(X, Y, "sqeuclidean", gc, band or 0.25)
    if st == R.NO_PATH:
        with pytest.raises(ValueError):
            seq.dtw(X, Y, metric="sqeuclidean", global_constraints=gc, band_rad=band or 0.25)
        return
    Dg, wpg = seq.dtw(X, Y, metric="sqeuclidean", global_constraints=gc, band_rad=band or 0.25, return_cost_matrix=True)
    np.testing.assert_array_equal(Dg, D)
    np.testing.assert_array_equal(wpg, wp)
    costg, wpg2 = seq.dtw(X, Y, metric="sqeuclidean", global_constraints=gc, band_rad=band or 0.25)
    assert costg == cost
    np.testing.assert_array_equal(wpg2, wp)


def _mfcc_stacks(k, seconds_list, seed0=0):
    from audio_feature_extraction_amd import _native as N
    from audio_feature_extraction_amd.synth import make_clip
    ctx = N.Context(0)
    plan = N.Plan(ctx, N.make_params(22050, 1024, 256, 13))
    ys = [make_clip(seed0 + i, 22050, s, speechy=True) for i, s in enumerate(seconds_list)]
    lengths = np.array([y.size for y in ys], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    out = plan.extract_batch(np.concatenate(ys), offsets, lengths, want_frames=True)
    assert (out["status"] == 0).all()
    res = [np.vstack([f["mfcc"], f["mfcc_delta"], f["mfcc_delta2"]]) for f in out["frames"]]
    plan.close()
    ctx.close()
    return res


@pytest.fixture(scope="module")
def real_feats(seq):
    rng = np.random.default_rng(7)
    return _mfcc_stacks(13, rng.uniform(1.0, 6.0, size=10).tolist())


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("band", [None, 0.25])
def test_real_mfcc_features(seq, real_feats, metric, band):
    gc = band is not None
    for a in range(0, 10, 2):
        X, Y = real_feats[a], real_feats[a + 1]
        r = R.band_radius(X.shape[1], Y.shape[1], 0.25) if gc else None
        C = R.local_cost(X, Y, metric, r)
        _, _, ref, _, st = R.dtw_vec(C)
        assert st == R.OK
        cost, wp = seq.dtw(X, Y, metric=metric, global_constraints=gc)
        tol = 1e-6 * ref + (1e-6 * len(wp) if metric == "cosine" else 0.0)
        assert abs(cost - ref) <= tol, (a, cost, ref)
        R.check_path(wp, X.shape[1], Y.shape[1], R.band_mask(X.shape[1], Y.shape[1], r))
        assert abs(R.path_cost(C, wp) - ref) <= tol


def _ragged_pairs(n_pairs=200):
    rng = np.random.default_rng(11)
    pairs = []
    for p in range(n_pairs):
        n, m = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        pairs.append((rng.integers(-4, 5, size=(13, n)).astype(np.float32), rng.integers(-4, 5, size=(13, m)).astype(np.float32)))
    bad = pairs[17][0].copy()
    bad[3, bad.shape[1] // 2] = np.nan
    pairs[17] = (bad, pairs[17][1])
    pairs[18] = (np.zeros((13, 2), np.float32), np.zeros((13, 2), np.float32))   # r = round(0.25 * 2) = 0: no path
    return pairs


def test_batch_equals_single_calls_and_isolates_failures(seq):
    pairs = _ragged_pairs()
    res = seq.dtw_batch(pairs, metric="sqeuclidean", global_constraints=True, band_rad=0.25)
    # r = round(0.25 * min(N, M)) = 0 (min <= 2) admits no path: rule 2 puts (0, 0) outside the band
    failed = {17} | {p for p, (X, Y) in enumerate(pairs) if R.band_radius(X.shape[1], Y.shape[1], 0.25) == 0}
    assert 18 in failed and len(failed) < 20
    assert {p for p, r in enumerate(res) if r is None} == failed
    from audio_feature_extraction_amd import _native as N
    # statuses straight from the binding
    ctx = seq._context(0)
    feats = np.concatenate([pairs[p][k].T for p in (16, 17, 18, 19) for k in (0, 1)])
    lens = [pairs[p][k].shape[1] for p in (16, 17, 18, 19) for k in (0, 1)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    xo, yo = offs[0::2], offs[1::2]
    xl, yl = np.array(lens[0::2]), np.array(lens[1::2])
    band = np.array([R.band_radius(a, b, 0.25) for a, b in zip(xl, yl)], np.int32)
    out = ctx.dtw_batch(feats, xo, xl, yo, yl, band, "sqeuclidean")
    assert out["status"].tolist() == [N.DTW_OK, N.DTW_NONFINITE, N.DTW_NO_PATH, N.DTW_OK]
    for p in list(range(0, 200, 3)) + [16, 19]:
        if p in failed:
            continue
        X, Y = pairs[p]
        single = seq.dtw(X, Y, metric="sqeuclidean", global_constraints=True, band_rad=0.25)
        assert res[p][0] == single[0]
        np.testing.assert_array_equal(res[p][1], single[1])


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_dtw import _ragged_pairs
from audio_feature_extraction_amd import sequence
res = sequence.dtw_batch(_ragged_pairs(), metric="sqeuclidean", global_constraints=True, band_rad=0.25)
cost = np.array([np.nan if r is None else r[0] for r in res])
paths = np.concatenate([np.zeros((0, 2), np.int64)] + [r[1] for r in res if r is not None])
np.savez(sys.argv[2], cost=cost, paths=paths)
"""


def test_chunked_batch_equals_one_chunk(seq, tmp_path):
    res = seq.dtw_batch(_ragged_pairs(), metric="sqeuclidean", global_constraints=True, band_rad=0.25)
    env = dict(os.environ, AFX_TEST_DTW_BUDGET="300000")     # a few pairs per chunk
    dst = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=300)
    z = np.load(dst)
    cost = np.array([np.nan if r is None else r[0] for r in res])
    np.testing.assert_array_equal(z["cost"], cost)
    np.testing.assert_array_equal(z["paths"], np.concatenate([r[1] for r in res if r is not None]))


def test_backtrack_off_gives_the_same_cost(seq, real_feats):
    for metric in ("euclidean", "sqeuclidean", "cosine"):
        X, Y = real_feats[2], real_feats[5]
        c1, _ = seq.dtw(X, Y, metric=metric)
        c0 = seq.dtw(X, Y, metric=metric, backtrack=False)
        assert c0 == c1


def test_large_pair_crosses_many_strips(seq):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((39, 4000)).astype(np.float32)
    Y = rng.standard_normal((39, 3500)).astype(np.float32)
    C = R.local_cost(X, Y)
    _, _, ref, wpr, st = R.dtw_vec(C)
    cost, wp = seq.dtw(X, Y)
    assert abs(cost - ref) <= 1e-6 * ref
    R.check_path(wp, 4000, 3500)
    assert abs(R.path_cost(C, wp) - ref) <= 1e-6 * ref


def _tones(durations, sr=22050, seed=0):
    freqs = [220.0, 330.0, 495.0, 660.0, 392.0, 294.0, 523.0, 247.0]
    out = []
    for k, d in enumerate(durations):
        t = np.arange(int(d * sr)) / sr
        out.append(0.4 * np.sin(2 * np.pi * freqs[k % len(freqs)] * t) + 0.1 * np.sin(2 * np.pi * 3.1 * freqs[k % len(freqs)] * t))
    return np.concatenate(out).astype(np.float32)


def test_align_files_end_to_end(seq, tmp_path):
    from audio_feature_extraction_amd import wavio
    from audio_feature_extraction_amd.core.feature_extractor import AudioFeatureExtractor
    durs = [0.35, 0.5, 0.25, 0.45, 0.3, 0.4, 0.3, 0.35]
    teacher, student = str(tmp_path / "teacher.wav"), str(tmp_path / "student.wav")
    wavio.write_wav_pcm16(teacher, _tones(durs), 22050)
    wavio.write_wav_pcm16(student, _tones([1.3 * d for d in durs]), 22050)
    fx = AudioFeatureExtractor(device=0)
    r = fx.align_files(teacher, student)
    assert set(r) == {"teacher_path", "student_path", "dtw_distance", "normalized_distance", "path"}
    wp = r["path"]
    assert r["normalized_distance"] == pytest.approx(r["dtw_distance"] / len(wp))
    dev = np.abs(wp[:, 1] - 1.3 * wp[:, 0]).mean()
    assert dev <= 3.0, dev
    # the same frames from .npz files written by save_frame_features
    tz, sz = str(tmp_path / "teacher.npz"), str(tmp_path / "student.npz")
    fx.save_frame_features(fx.extract_frame_features(teacher), tz)
    fx.save_frame_features(fx.extract_frame_features(student), sz)
    rz = fx.align_files(tz, sz)
    assert rz["dtw_distance"] == r["dtw_distance"]
    np.testing.assert_array_equal(rz["path"], wp)
    b = fx.align_batch([(teacher, student), (tz, sz), (student, teacher)])
    assert b[0]["dtw_distance"] == r["dtw_distance"]
    np.testing.assert_array_equal(b[0]["path"], wp)
    assert b[1]["dtw_distance"] == rz["dtw_distance"]
    rs = fx.align_files(student, teacher)
    assert b[2]["dtw_distance"] == rs["dtw_distance"]
    np.testing.assert_array_equal(b[2]["path"], rs["path"])
