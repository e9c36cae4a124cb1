"""GPU checks of afx_dtw_steps_batch / sequence.dtw's step_sizes_sigma, weights_add, weights_mul and subseq against the
float64 oracle (tests/dtw_steps_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dtw_ref as R
from tests import dtw_steps_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# strip boundaries (lanes 0 and 1 read both boundary rows at 64 / 65 / 66 and 128 / 129 / 130), tile edges (multiples of 8
# and their neighbours) and ring edges (the 72-column ring wraps at 72)
SIZES = [1, 2, 3, 7, 8, 9, 63, 64, 65, 66, 71, 72, 73, 127, 128, 129, 130, 200]
DIMS = [1, 13, 39, 64, 128, 20]
W_MUL = [1.0, 1.5, 2.0, 3.0]
W_ADD = [0.0, 0.5, 1.0]
SLOPE = [[1, 1], [1, 2], [2, 1]]
FIVE = [[1, 1], [2, 1], [1, 2], [2, 2], [0, 1]]        # five steps, (0, 1) as a custom step
DIAG = [[1, 1]]
LISTS = {"defw": None, "slope": SLOPE, "five": FIVE, "diag": DIAG}
PER_GROUP = 10


@pytest.fixture(scope="module")
def seq():
    from audio_feature_extraction_amd import _native, sequence
    if _native.device_count() < 1:
        pytest.fail("no GPU visible")
    return sequence


def _shape(rng, name, subseq, c):
    n, m = int(rng.choice(SIZES)), int(rng.choice(SIZES))
    if name == "slope" and not subseq:
        m = int(rng.integers(n // 2 + 1, max(n // 2 + 2, 2 * n)))      # M in [N // 2 + 1, 2 N - 1]: a path exists
    elif name == "five" and not subseq and n > 2 * m - 1:
        n, m = m, n                                # at most two rows per column: N <= 2 M - 1 or there is no path
    elif name == "diag":
        if subseq:
            n, m = min(n, m), max(n, m)            # [(1,1)] needs N <= M
        elif c == PER_GROUP - 1:
            n, m = 64, 73                          # N < M without subseq: no path, the GPU must raise
        else:
            m = n                                  # the diagonal alone reaches (N-1, M-1) only when N == M
    return n, m


def _cases():
    rng = np.random.default_rng(4242)
    out = []
    for name in LISTS:
        for subseq in (False, True):
            for c in range(PER_GROUP):
                n, m = _shape(rng, name, subseq, c)
                k = 3 if LISTS[name] is None else len(LISTS[name])
                weighted = name == "defw" or c % 2 == 1
                wa = rng.choice(W_ADD, size=k).tolist() if weighted else None
                wm = rng.choice(W_MUL, size=k).tolist() if weighted else None
                out.append((name, subseq, c, n, m, DIMS[(c + len(out)) % 5], wa, wm, None))   # the first five dims: ids as before
    for c in range(PER_GROUP):                     # default steps + weights + band, with subseq
        n, m = int(rng.choice(SIZES[1:])), int(rng.choice(SIZES[1:]))
        out.append(("defw-band", True, c, n, m, DIMS[c % 5], rng.choice(W_ADD, size=3).tolist(),
                    rng.choice(W_MUL, size=3).tolist(), [0.25, 0.5][c % 2]))
    # dim 20 (librosa's n_mfcc default): the 24-wide instance, one weighted case per list, with and without subseq, drawn
    # after every case above so that those keep their shapes
    for name in LISTS:
        for subseq in (False, True):
            n, m = _shape(rng, name, subseq, PER_GROUP)
            k = 3 if LISTS[name] is None else len(LISTS[name])
            out.append((name, subseq, PER_GROUP, n, m, 20, rng.choice(W_ADD, size=k).tolist(),
                        rng.choice(W_MUL, size=k).tolist(), None))
    out.append(("defw-band", True, PER_GROUP, 129, 72, 20, [0.0, 0.5, 1.0], [1.0, 1.5, 2.0], 0.25))
    return out


def _id(case):
    name, subseq, c, n, m, dim = case[:6]
    return "%s%s-%d-%dx%d-d%d" % (name, "-sub" if subseq else "", c, n, m, dim)


def _int_pair(seed, n, m, dim):
    rng = np.random.default_rng(seed)
    return (rng.integers(-4, 5, size=(dim, n)).astype(np.float32), rng.integers(-4, 5, size=(dim, m)).astype(np.float32))


def _kwargs(case):
    name, subseq, c, n, m, dim, wa, wm, band = case
    kw = dict(metric="sqeuclidean", step_sizes_sigma=LISTS[name.split("-")[0]], weights_add=wa, weights_mul=wm,
              subseq=subseq)
    if band is not None:
        kw.update(global_constraints=True, band_rad=band)
    return kw


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_bit_exact_small_integers(seq, case):
    """Integer features in [-4, 4] and weights that are multiples of 0.5: every sum is exact in float32 / float64, so D,
    the cost and the path must equal the oracle's bit for bit."""
    name, subseq, c, n, m, dim = case[:6]
    X, Y = _int_pair(1000 * len(name) + 10 * c + subseq, n, m, dim)
    kw = _kwargs(case)
    D, wp, cost, end, st = S.dtw(X, Y, **kw)
    if st == S.NO_PATH:
        with pytest.raises(ValueError):
            seq.dtw(X, Y, **kw)
        return
    assert st == S.OK
    Dg, wpg = seq.dtw(X, Y, return_cost_matrix=True, **kw)
    np.testing.assert_array_equal(Dg, D)
    np.testing.assert_array_equal(wpg, wp)
    costg, wpg2 = seq.dtw(X, Y, **kw)
    assert costg == cost
    np.testing.assert_array_equal(wpg2, wp)
    assert seq.dtw(X, Y, backtrack=False, **kw) == cost


@pytest.mark.parametrize("kw", [
    dict(step_sizes_sigma=FIVE, subseq=True),
    dict(step_sizes_sigma=SLOPE, weights_mul=[1.0, 1.0, 1.0]),
    dict(weights_mul=[1.0, 1.0, 1.0], subseq=True),
], ids=["five-sub", "slope", "defw-sub"])
def test_all_zero_features_tie_everywhere(seq, kw):
    X, Y = np.zeros((13, 65), np.float32), np.zeros((13, 129), np.float32)   # M = 2 N - 1: the slope-limited list's limit
    D, wp, cost, end, st = S.dtw(X, Y, metric="sqeuclidean", **kw)
    assert st == S.OK and cost == 0.0
    Dg, wpg = seq.dtw(X, Y, metric="sqeuclidean", return_cost_matrix=True, **kw)
    np.testing.assert_array_equal(Dg, D)
    np.testing.assert_array_equal(wpg, wp)           # the first minimum wins every tie, the first argmin ends the path


def test_nan_feature_raises(seq):
    X, Y = _int_pair(1, 70, 90, 13)
    X[5, 33] = np.nan
    assert S.dtw(X, Y, step_sizes_sigma=SLOPE, subseq=True)[4] == S.NONFINITE
    with pytest.raises(ValueError, match="NaN"):
        seq.dtw(X, Y, step_sizes_sigma=SLOPE, subseq=True)
    with pytest.raises(ValueError, match="NaN"):
        seq.dtw(Y, X, step_sizes_sigma=SLOPE, subseq=True)


def test_zero_norm_frame_under_cosine_raises(seq):
    X, Y = _int_pair(2, 70, 90, 13)
    Y[:, 77] = 0.0
    assert S.dtw(X, Y, "cosine", weights_mul=[1, 2, 2])[4] == S.NONFINITE
    with pytest.raises(ValueError, match="NaN"):
        seq.dtw(X, Y, metric="cosine", weights_mul=[1, 2, 2])


@pytest.fixture(scope="module")
def real_feats(seq):
    from tests.test_gpu_dtw import _mfcc_stacks
    rng = np.random.default_rng(7)
    # lengths within a factor 1.9 of each other: the slope-limited list (slope between 1/2 and 2) admits a path
    return _mfcc_stacks(13, rng.uniform(2.0, 3.8, size=10).tolist())


_REF = {}


def _real_ref(real_feats, a, metric, mode):
    """The oracle's result for pair (a, a + 1) of the real features, computed once per (pair, metric, mode)."""
    key = (a, metric, mode)
    if key not in _REF:
        steps, subseq = MODES[mode]
        X, Y = real_feats[a], real_feats[a + 1]                      # where X is the longer one subseq swaps (rule 2)
        St, wa, wm = S.step_table(steps, None if steps is None else [0.0, 0.5, 0.5], None if steps is None else [1.0, 2.0, 2.0])
        XX, YY = (Y, X) if subseq and X.shape[1] > Y.shape[1] else (X, Y)
        C = R.local_cost(XX, YY, metric)
        _, _, ref, end, _, st = S.dtw_vec(C, St, wa, wm, subseq)
        C.setflags(write=False)
        _REF[key] = (C, St, wa, wm, ref, st, XX is not X)
    return _REF[key]


MODES = {"slope": (SLOPE, False), "slope-sub": (SLOPE, True), "default-sub": (None, True)}


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("mode", list(MODES))
def test_real_mfcc_features(seq, real_feats, metric, mode):
    steps, subseq = MODES[mode]
    for a in range(0, 10, 2):
        X, Y = real_feats[a], real_feats[a + 1]
        C, St, wa, wm, ref, st, swapped = _real_ref(real_feats, a, metric, mode)
        assert st == S.OK
        kw = {} if steps is None else dict(step_sizes_sigma=steps, weights_add=[0.0, 0.5, 0.5], weights_mul=[1.0, 2.0, 2.0])
        cost, wp = seq.dtw(X, Y, metric=metric, subseq=subseq, **kw)
        tol = 1e-6 * ref + (1e-6 * len(wp) if metric == "cosine" else 0.0)
        print(mode, metric, a, X.shape[1], Y.shape[1], cost, ref, abs(cost - ref), tol)
        assert abs(cost - ref) <= tol, (a, cost, ref)
        wpd = wp[:, ::-1] if swapped else wp                         # the orientation the DP ran in
        S.check_path(wpd, C.shape[0], C.shape[1], St, wm, subseq, end=int(wpd[0, 1]))
        assert abs(S.path_cost(C, wpd, St, wa, wm) - ref) <= tol


def _ragged_pairs(n_pairs=60, big=False):
    rng = np.random.default_rng(11)
    pairs = []
    for p in range(n_pairs):
        n, m = int(rng.integers(1, 150)), int(rng.integers(1, 150))
        pairs.append((rng.integers(-4, 5, size=(13, n)).astype(np.float32), rng.integers(-4, 5, size=(13, m)).astype(np.float32)))
    bad = pairs[17][0].copy()
    bad[3, bad.shape[1] // 2] = np.nan
    pairs[17] = (bad, pairs[17][1])
    if big:                                            # one pair whose workspace alone exceeds the child's budget
        pairs[30] = (rng.integers(-4, 5, size=(13, 900)).astype(np.float32), rng.integers(-4, 5, size=(13, 800)).astype(np.float32))
    return pairs


_BATCH_KW = dict(metric="sqeuclidean", step_sizes_sigma=SLOPE, weights_add=[0.0, 0.5, 1.0], weights_mul=[1.0, 1.5, 2.0])


def test_batch_equals_single_calls_and_isolates_failures(seq):
    from audio_feature_extraction_amd import _native as N
    pairs = _ragged_pairs()
    res = seq.dtw_batch(pairs, **_BATCH_KW)
    oracle = [S.dtw(X, Y, **_BATCH_KW) for X, Y in pairs]
    failed = {p for p, o in enumerate(oracle) if o[4] != S.OK}
    assert 17 in failed and oracle[17][4] == S.NONFINITE
    assert any(oracle[p][4] == S.NO_PATH for p in failed) and len(failed) < len(pairs) - 10
    assert {p for p, r in enumerate(res) if r is None} == failed
    for p, r in enumerate(res):
        if r is None:
            continue
        assert r[0] == oracle[p][2]
        np.testing.assert_array_equal(r[1], oracle[p][1])
        if p % 4 == 0:
            single = seq.dtw(*pairs[p], **_BATCH_KW)
            assert single[0] == r[0]
            np.testing.assert_array_equal(single[1], r[1])
    # statuses and end columns straight from the binding, with subseq
    sel = (16, 17, 18, 19)
    feats = np.concatenate([pairs[p][k].T for p in sel for k in (0, 1)])
    lens = [pairs[p][k].shape[1] for p in sel for k in (0, 1)]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    xo, yo, xl, yl = offs[0::2], offs[1::2], np.array(lens[0::2]), np.array(lens[1::2])
    swap = xl > yl                                     # the binding aligns X inside Y as given: the swap is the caller's
    out = seq._context(0).dtw_steps_batch(feats, np.where(swap, yo, xo), np.where(swap, yl, xl), np.where(swap, xo, yo),
                                          np.where(swap, xl, yl), None, "sqeuclidean", True, False,
                                          np.array(SLOPE, np.int32), _BATCH_KW["weights_add"], _BATCH_KW["weights_mul"], True)
    assert out["status"].tolist() == [N.DTW_OK, N.DTW_NONFINITE, N.DTW_OK, N.DTW_OK]
    for q, p in enumerate(sel):
        if q == 1:
            assert out["paths"][q] is None and out["end"][q] == -1
            continue
        D, wp, cost, end, st = S.dtw(*pairs[p], subseq=True, **_BATCH_KW)
        assert out["cost"][q] == cost and out["end"][q] == end
        np.testing.assert_array_equal(out["paths"][q][:, ::-1] if swap[q] else out["paths"][q], wp)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_gpu_dtw_steps import _ragged_pairs, _BATCH_KW
from audio_feature_extraction_amd import sequence
res = sequence.dtw_batch(_ragged_pairs(big=True), subseq=True, **_BATCH_KW)
cost = np.array([np.nan if r is None else r[0] for r in res])
paths = np.concatenate([np.zeros((0, 2), np.int64)] + [r[1] for r in res if r is not None])
np.savez(sys.argv[2], cost=cost, paths=paths)
"""


def test_chunked_batch_equals_one_chunk(seq, tmp_path):
    pairs = _ragged_pairs(big=True)
    res = seq.dtw_batch(pairs, subseq=True, **_BATCH_KW)
    assert [p for p, r in enumerate(res) if r is None] == [17]
    D, wp, cost, end, st = S.dtw(*pairs[30], subseq=True, **_BATCH_KW)
    assert res[30][0] == cost
    np.testing.assert_array_equal(res[30][1], wp)
    # 4-bit codes: the 900 x 800 pair needs 15 strips x 108 words x 64 lanes x 4 bytes = 414,720 bytes, more than the budget;
    # the other pairs need up to 3 x 27 x 64 x 4 = 20,736 bytes of codes each, so the batch takes several chunks
    env = dict(os.environ, AFX_TEST_DTW_BUDGET="300000")
    dst = str(tmp_path / "chunked.npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, dst], env=env, check=True, timeout=300)
    z = np.load(dst)
    np.testing.assert_array_equal(z["cost"], np.array([np.nan if r is None else r[0] for r in res]))
    np.testing.assert_array_equal(z["paths"], np.concatenate([r[1] for r in res if r is not None]))


def test_align_files_finds_the_teacher_inside_the_student(seq, tmp_path):
    """Teacher clip A against a student recording of lead-in + A + tail.  The lead-in and tail are quiet room noise 15 dB
    under A -- above the trim threshold (30 dB), so the trim that precedes the MFCC leaves them in.  With subseq the path's
    student span must be the A part; without it the path is forced across the whole recording."""
    from audio_feature_extraction_amd import wavio
    from audio_feature_extraction_amd.core.feature_extractor import AudioFeatureExtractor
    from tests.test_gpu_dtw import _tones
    sr, hop = 22050, 256
    a = _tones([0.35, 0.5, 0.25, 0.45, 0.3, 0.4])
    rng = np.random.default_rng(0)
    lead, tail = int(0.8 * sr), int(0.6 * sr)
    student = np.concatenate([0.05 * rng.standard_normal(lead), a, 0.05 * rng.standard_normal(tail)]).astype(np.float32)
    tp, sp = str(tmp_path / "teacher.wav"), str(tmp_path / "student.wav")
    wavio.write_wav_pcm16(tp, a, sr)
    wavio.write_wav_pcm16(sp, student, sr)
    fx = AudioFeatureExtractor(device=0)
    r = fx.align_files(tp, sp, subseq=True)
    wp = r["path"]
    assert r["normalized_distance"] == pytest.approx(r["dtw_distance"] / len(wp))
    assert wp[0, 0] == wp[:, 0].max() and wp[-1, 0] == 0
    lo, hi = lead / hop, (lead + a.size) / hop
    # delta and delta2 look 4 + 4 frames to each side and a frame spans 4 hops: the span may miss the A part by that much
    assert lo - 12 <= wp[-1, 1] <= lo + 12 and hi - 12 <= wp[0, 1] <= hi + 12, (wp[-1], wp[0], lo, hi)
    full = fx.align_files(tp, sp)
    assert full["path"][-1, 1] == 0 and full["dtw_distance"] > 2 * r["dtw_distance"]
    b = fx.align_batch([(tp, sp), (sp, tp)], subseq=True)
    assert b[0]["dtw_distance"] == r["dtw_distance"]
    np.testing.assert_array_equal(b[0]["path"], wp)
    np.testing.assert_array_equal(b[1]["path"], wp[:, ::-1])         # the longer file first: swapped and flipped back


def test_default_arguments_take_the_default_path(seq):
    """A call that leaves the four step arguments at their defaults returns what afx_dtw_batch returns for the same inputs
    (it is the same call), and the general kernel agrees with it on the default list with unit weights."""
    X, Y = _int_pair(5, 129, 200, 39)
    ctx = seq._context(0)
    feats = np.concatenate([X.T, Y.T])
    direct = ctx.dtw_batch(feats, [0], [129], [129], [200], None, "sqeuclidean", True, True)
    D, wp = seq.dtw(X, Y, metric="sqeuclidean", return_cost_matrix=True)
    np.testing.assert_array_equal(D, direct["D"][0])
    np.testing.assert_array_equal(wp, direct["paths"][0])
    assert seq.dtw(X, Y, metric="sqeuclidean")[0] == direct["cost"][0]
    Dg, wpg = seq.dtw(X, Y, metric="sqeuclidean", return_cost_matrix=True, weights_mul=[1.0, 1.0, 1.0])
    np.testing.assert_array_equal(Dg, D)
    np.testing.assert_array_equal(wpg, wp)
    rng = np.random.default_rng(3)
    Xr, Yr = rng.standard_normal((39, 300)).astype(np.float32), rng.standard_normal((39, 260)).astype(np.float32)
    direct = ctx.dtw_batch(np.concatenate([Xr.T, Yr.T]), [0], [300], [300], [260], None, "euclidean", True, False)
    cost, wp = seq.dtw(Xr, Yr)
    assert cost == direct["cost"][0]
    np.testing.assert_array_equal(wp, direct["paths"][0])
    cg, wpg = seq.dtw(Xr, Yr, weights_add=[0.0, 0.0, 0.0])           # the other kernel, the same local cost: bit-equal
    assert cg == cost
    np.testing.assert_array_equal(wpg, wp)


_BOTH_SHAPES = [(65, 130), (130, 66), (1, 72), (64, 64), (129, 73)]


@pytest.mark.parametrize("dim", [13, 39, 128])
@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "cosine"])
def test_both_kernels_agree_bit_for_bit_on_the_default_steps(seq, metric, dim):
    """k_dtw (dtw_batch) and k_dtw_steps on the default list with no weights (dtw_steps_batch) form the same float64 sums
    from the same float32 local cost (1.0 * c + 0.0 == c), so status, cost, every D and every path are equal, not close:
    seeded standard-normal features, strip / tile / ring edges, with and without a band of 0.25 min(N, M)."""
    rng = np.random.default_rng(1000 * dim + len(metric))
    lens = [k for nm in _BOTH_SHAPES for k in nm]
    feats = rng.standard_normal((sum(lens), dim)).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    xo, yo, xl, yl = offs[0::2], offs[1::2], np.array(lens[0::2]), np.array(lens[1::2])
    ctx = seq._context(0)
    for band in (None, [int(round(0.25 * min(n, m))) for n, m in _BOTH_SHAPES]):
        a = ctx.dtw_batch(feats, xo, xl, yo, yl, band, metric, True, True)
        b = ctx.dtw_steps_batch(feats, xo, xl, yo, yl, band, metric, True, True, steps=None, weights_add=None, weights_mul=None)
        np.testing.assert_array_equal(a["status"], b["status"])
        np.testing.assert_array_equal(a["cost"], b["cost"])
        assert band is not None or (a["status"] == 0).all()
        for p in range(len(_BOTH_SHAPES)):
            np.testing.assert_array_equal(a["D"][p], b["D"][p])
            assert (a["paths"][p] is None) == (b["paths"][p] is None)
            if a["paths"][p] is not None:
                np.testing.assert_array_equal(a["paths"][p], b["paths"][p])
