"""CPU checks of the step-list DTW oracle (tests/dtw_steps_ref.py)."""
import numpy as np
import pytest

from tests import dtw_ref as R
from tests import dtw_steps_ref as S

SLOPE = [[1, 1], [1, 2], [2, 1]]
FIVE = [[1, 1], [2, 1], [1, 2], [2, 2], [0, 1]]


def _ragged(rng, lo=1, hi=40, dim_hi=4, span=4):
    n, m, dim = int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), int(rng.integers(1, dim_hi))
    X = rng.integers(-span, span + 1, size=(dim, n)).astype(np.float64)
    Y = rng.integers(-span, span + 1, size=(dim, m)).astype(np.float64)
    return X, Y


@pytest.mark.parametrize("seed", range(30))
def test_default_arguments_equal_the_default_oracle(seed):
    rng = np.random.default_rng(seed)
    X, Y = _ragged(rng)
    gc = bool(seed % 2)
    D0, _, cost0, wp0, st0 = R.dtw(X, Y, "sqeuclidean", gc, 0.25)
    for vec in (False, True):
        D, wp, cost, end, st = S.dtw(X, Y, "sqeuclidean", global_constraints=gc, band_rad=0.25, vectorised=vec)
        assert st == st0
        if st == R.NO_PATH:
            continue
        np.testing.assert_array_equal(D, D0)
        assert cost == cost0 and end == Y.shape[1] - 1
        np.testing.assert_array_equal(wp, wp0)


def _configs():
    return [
        dict(weights_add=[0.0, 0.5, 1.0], weights_mul=[1.0, 1.5, 2.0]),
        dict(step_sizes_sigma=SLOPE),
        dict(step_sizes_sigma=SLOPE, weights_add=[0.0, 1.0, 0.5], weights_mul=[2.0, 1.0, 3.0]),
        dict(step_sizes_sigma=FIVE, weights_add=[0, 0.5, 0.5, 1, 1], weights_mul=[1, 1.5, 1.5, 2, 3]),
        dict(step_sizes_sigma=[[0, 2], [2, 0], [1, 1]], weights_mul=[0.0, 1.0, 1.0]),     # a zero weight: inf * 0
    ]


@pytest.mark.parametrize("seed", range(40))
def test_loop_and_vectorised_forms_agree(seed):
    rng = np.random.default_rng(100 + seed)
    X, Y = _ragged(rng, hi=14, span=1)                 # few distinct values: ties everywhere
    cfg = _configs()[seed % 5]
    subseq, gc = bool((seed // 5) % 2), bool((seed // 10) % 2)
    a = S.dtw(X, Y, "sqeuclidean", subseq=subseq, global_constraints=gc, band_rad=0.5, vectorised=False, **cfg)
    b = S.dtw(X, Y, "sqeuclidean", subseq=subseq, global_constraints=gc, band_rad=0.5, vectorised=True, **cfg)
    assert a[4] == b[4]
    if a[4] != S.NONFINITE:
        np.testing.assert_array_equal(a[0], b[0])
        assert a[3] == b[3]
    if a[4] == S.OK:
        assert a[2] == b[2]
        np.testing.assert_array_equal(a[1], b[1])
        n, m = X.shape[1], Y.shape[1]
        swap = subseq and n > m
        St, wa, wm = S.step_table(cfg.get("step_sizes_sigma"), cfg.get("weights_add"), cfg.get("weights_mul"))
        wp = a[1][:, ::-1] if swap else a[1]
        nn, mm = (m, n) if swap else (n, m)
        S.check_path(wp, nn, mm, St, wm, subseq, end=a[3])
        XX, YY = (Y, X) if swap else (X, Y)
        C = R.local_cost(XX, YY, "sqeuclidean", R.band_radius(nn, mm, 0.5) if gc else None)
        if (wm[St[:, 0] == 0] >= 1.0).all():               # else a row-0 cell may undercut its seed (path_cost's docstring)
            assert S.path_cost(C, wp, St, wa, wm) == a[2]  # integer and half-integer sums: exact


def test_hand_worked_subsequence():
    # X = [1, 2] inside Y = [5, 1, 2, 7]: |x - y|, default steps
    X, Y = np.array([1.0, 2.0]), np.array([5.0, 1.0, 2.0, 7.0])
    D, wp, cost, end, st = S.dtw(X, Y, subseq=True, vectorised=False)
    np.testing.assert_array_equal(D, [[4, 0, 1, 6], [7, 1, 0, 5]])
    assert st == S.OK and cost == 0.0 and end == 2
    np.testing.assert_array_equal(wp, [[1, 2], [0, 1]])


@pytest.mark.parametrize("steps", [None, SLOPE, [[1, 1]]])
def test_embedded_sequence_is_found_in_both_argument_orders(steps):
    rng = np.random.default_rng(9)
    Y = rng.integers(-4, 5, size=(3, 50)).astype(np.float64)
    Y[:, :12] += 20.0                                   # nothing outside the copy comes near it
    Y[:, 29:] -= 20.0
    X = Y[:, 12:29].copy()
    for vec in (False, True):
        D, wp, cost, end, st = S.dtw(X, Y, "sqeuclidean", step_sizes_sigma=steps, subseq=True, vectorised=vec)
        assert st == S.OK and cost == 0.0 and end == 28
        np.testing.assert_array_equal(wp, np.stack([np.arange(16, -1, -1), np.arange(28, 11, -1)], 1))
        assert D.shape == (17, 50)
        # the longer sequence first: rule 2 swaps, and the path and D come back in the caller's orientation
        D2, wp2, cost2, end2, st2 = S.dtw(Y, X, "sqeuclidean", step_sizes_sigma=steps, subseq=True, vectorised=vec)
        assert st2 == S.OK and cost2 == 0.0 and end2 == 28
        np.testing.assert_array_equal(wp2, wp[:, ::-1])
        np.testing.assert_array_equal(D2, D.T)


def test_diagonal_only_needs_n_le_m():
    X, Y = np.zeros((2, 6)), np.zeros((2, 5))
    with pytest.raises(ValueError):
        S.dtw(X, Y, step_sizes_sigma=[[1, 1]])
    assert S.dtw(Y, X, step_sizes_sigma=[[1, 1]], subseq=True)[4] == S.OK
    assert S.dtw(X, Y, step_sizes_sigma=[[1, 1]], subseq=True)[4] == S.OK      # swapped by rule 2 first
    assert S.dtw(Y, X, step_sizes_sigma=[[1, 1]])[4] == S.NO_PATH              # 5 rows cannot reach column 5 of 6
    assert S.dtw(X, X, step_sizes_sigma=[[1, 1]])[2] == 0.0


def test_default_steps_never_win_behind_a_custom_list():
    X, Y = np.arange(6.0), np.arange(9.0)
    D, wp, cost, end, st = S.dtw(X, Y, step_sizes_sigma=[[0, 1], [1, 0], [1, 1]])
    D0, _, cost0, wp0, _ = R.dtw(X, Y)
    assert st == S.OK and cost == cost0            # the same three steps in another order: the same costs
    np.testing.assert_array_equal(D, D0)
    St, wa, wm = S.step_table([[0, 1], [1, 0], [1, 1]])
    assert np.isinf(wa[:3]).all() and np.isinf(wm[:3]).all() and St.shape == (6, 2)


def test_nonfinite_and_no_path_status():
    X = np.ones((2, 5))
    Xn = X.copy()
    Xn[0, 2] = np.nan
    assert S.dtw(Xn, X, step_sizes_sigma=SLOPE)[4] == S.NONFINITE
    assert S.dtw(np.zeros((2, 5)), X, "cosine", subseq=True)[4] == S.NONFINITE
    assert S.dtw(np.ones((1, 3)), np.ones((1, 9)), step_sizes_sigma=SLOPE)[4] == S.NO_PATH     # slope above 2
    assert S.dtw(np.ones((1, 3)), np.ones((1, 9)), step_sizes_sigma=SLOPE, subseq=True)[4] == S.OK


def test_slope_limited_pairs_have_a_path():
    # the GPU file draws M from [N // 2 + 1, 2 N - 1] for the slope-limited list without subseq
    rng = np.random.default_rng(3)
    for _ in range(60):
        n = int(rng.integers(1, 60))
        m = int(rng.integers(n // 2 + 1, max(n // 2 + 2, 2 * n)))
        X, Y = rng.integers(-4, 5, size=(2, n)).astype(float), rng.integers(-4, 5, size=(2, m)).astype(float)
        assert S.dtw(X, Y, "sqeuclidean", step_sizes_sigma=SLOPE)[4] == S.OK, (n, m)
