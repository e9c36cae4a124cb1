"""CPU checks of the DTW oracle (tests/dtw_ref.py) and of sequence.dtw's argument validation (no device is opened)."""
import numpy as np
import pytest

from tests import dtw_ref as R


@pytest.mark.parametrize("seed", range(40))
def test_loop_and_vectorised_forms_agree_on_ties(seed):
    rng = np.random.default_rng(seed)
    n, m, dim = rng.integers(1, 12, size=2).tolist() + [int(rng.integers(1, 4))]
    X = rng.integers(-1, 2, size=(dim, n)).astype(np.float64)     # few distinct values: ties everywhere
    Y = rng.integers(-1, 2, size=(dim, m)).astype(np.float64)
    gc = bool(seed % 2)
    a = R.dtw(X, Y, "sqeuclidean", gc, 0.5, vectorised=False)
    b = R.dtw(X, Y, "sqeuclidean", gc, 0.5, vectorised=True)
    assert a[4] == b[4]
    if a[4] == R.OK:
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[3], b[3])


def test_hand_worked_3x4():
    # X = [0, 1, 2], Y = [0, 0, 1, 2], |x - y|
    X, Y = np.array([0.0, 1.0, 2.0]), np.array([0.0, 0.0, 1.0, 2.0])
    D, steps, cost, wp, st = R.dtw(X, Y, "euclidean", vectorised=False)
    C = np.array([[0, 0, 1, 2], [1, 1, 0, 1], [2, 2, 1, 0]], float)
    np.testing.assert_array_equal(R.local_cost(X, Y), C)
    np.testing.assert_array_equal(D, [[0, 0, 1, 3], [1, 1, 0, 1], [3, 3, 1, 0]])
    assert st == R.OK and cost == 0.0
    np.testing.assert_array_equal(wp, [[2, 3], [1, 2], [0, 1], [0, 0]])


def test_identical_sequences_give_zero_and_the_diagonal():
    X = np.random.default_rng(3).standard_normal((5, 17))
    for vec in (False, True):
        D, _, cost, wp, st = R.dtw(X, X, vectorised=vec)
        assert st == R.OK and cost == 0.0
        np.testing.assert_array_equal(wp, np.stack([np.arange(16, -1, -1)] * 2, 1))


@pytest.mark.parametrize("n,m", [(1, 1), (1, 7), (6, 1)])
def test_single_frame_sides(n, m):
    rng = np.random.default_rng(n * 10 + m)
    X, Y = rng.standard_normal((3, n)), rng.standard_normal((3, m))
    C = R.local_cost(X, Y)
    for vec in (False, True):
        D, _, cost, wp, st = R.dtw(X, Y, vectorised=vec)
        assert st == R.OK
        assert cost == pytest.approx(C.sum())
        assert len(wp) == n + m - 1
        R.check_path(wp, n, m)


@pytest.mark.parametrize("n,m", [(7, 12), (10, 10), (12, 7)])
def test_band_mask_rule(n, m):
    r = R.band_radius(n, m, 0.25)
    mask = R.band_mask(n, m, r)
    off = abs(n - m)
    for i in range(n):
        for j in range(m):
            if n < m:
                want = -r < j - i < r + off
            else:
                want = -r - off < j - i < r
            assert mask[i, j] == want, (i, j)
    assert R.band_radius(10, 10, 0.25) == 2 and R.band_radius(10, 6, 0.25) == 2   # 2.5 and 1.5 round half to even
    C = R.local_cost(np.zeros((1, n)), np.zeros((1, m)), r=r)
    assert np.isinf(C[~mask]).all() and (C[mask] == 0).all()


def test_no_path_when_radius_is_zero():
    *_, st = R.dtw(np.zeros((1, 4)), np.zeros((1, 4)), global_constraints=True, band_rad=0.0)
    assert st == R.NO_PATH


@pytest.mark.parametrize("X,Y", [
    (np.zeros((3, 5)), np.zeros((4, 5))),        # dim mismatch
    (np.zeros((3, 0)), np.zeros((3, 5))),        # empty
    (np.zeros((2, 3, 4)), np.zeros((2, 3, 4))),  # 3-D
])
def test_sequence_dtw_validates_before_the_device(X, Y, monkeypatch):
    from audio_feature_extraction_amd import _native, sequence

    def no_device(*a, **k):
        raise AssertionError("a device was opened")
    monkeypatch.setattr(_native, "Context", no_device)
    with pytest.raises(ValueError):
        sequence.dtw(X, Y)
    with pytest.raises(ValueError):
        sequence.dtw(np.zeros((3, 5)), np.zeros((3, 5)), metric="manhattan")
    assert sequence.dtw_batch([(X, Y)]) == [None]
