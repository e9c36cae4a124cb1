"""The DTW certificate (tests/dtw_cert.py) tested on the CPU in both directions: it accepts the float64 oracle's result and
the result of the oracle DP over the float32 restatement of the kernel's local cost, and it rejects each single mutation
of an accepted result that a wrong kernel could produce.  Also: how much of the derived tolerance T plain float32 rounding
uses on the inputs the GPU grid runs."""
import numpy as np
import pytest

from tests import dtw_cert as K
from tests import dtw_ref as R
from tests import dtw_steps_ref as S

SLOPE = [[1, 1], [1, 2], [2, 1]]
FIVE = [[1, 1], [2, 1], [1, 2], [2, 2], [0, 1]]
MODES = {
    "default": dict(),
    "band": dict(band_rad=0.25),
    "weighted": dict(steps=SLOPE, wa=[0.0, 0.5, 1.0], wm=[1.0, 1.5, 2.0]),
    "weighted-sub": dict(steps=SLOPE, wa=[0.0, 0.5, 1.0], wm=[1.0, 1.5, 2.0], subseq=True),
    "five-sub": dict(steps=FIVE, subseq=True),
}


def _result(X, Y, metric, restated, steps=None, wa=None, wm=None, subseq=False, band_rad=None, radius=None):
    """What a correct device would return: the oracle DP over C (float64) or over the float32 restatement of the kernel's
    local cost.  A dict of certify's arguments plus the oracle's step matrix."""
    n, m = X.shape[1], Y.shape[1]
    St, wa, wm = S.step_table(steps, wa, wm)
    if radius is None and band_rad is not None:
        radius = R.band_radius(n, m, band_rad)
    C = K.kernel_local_cost(X, Y, metric).astype(np.float64) if restated else R.local_cost(X, Y, metric)
    C = np.where(R.band_mask(n, m, radius), C, np.inf)
    D, codes, cost, end, wp, st = S.dtw_vec(C, St, wa, wm, subseq)
    assert st == S.OK
    return dict(D=D, wp=wp, cost=cost, cost_no_backtrack=cost, X=X, Y=Y, metric=metric, St=St, wa=wa, wm=wm, radius=radius,
                subseq=subseq), codes


@pytest.mark.parametrize("metric", K.METRICS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("restated", [False, True], ids=["float64", "float32-cost"])
def test_accepts_a_correct_result(metric, mode, restated):
    worst = 0.0
    for kind, (n, m), dim in (("normal", (65, 71), 20), ("mfcc", (129, 72), 39), ("normal", (64, 64), 128), ("mfcc", (1, 1), 1)):
        if "sub" in mode and n > m:
            n, m = m, n                                           # the orientation the DP runs in
        if mode == "band" and min(n, m) < 2:
            continue                                              # radius round(0.25 * 1) = 0 admits no path
        X, Y = K.make_pair(kind, n, m, dim, 7 * dim + n)
        args, _ = _result(X, Y, metric, restated, **MODES[mode])
        worst = max(worst, K.certify(label="%s %dx%d d%d" % (kind, n, m, dim), **args)["ratio"])
    print("accept", metric, mode, "restated" if restated else "float64", "max |D - (min pred + C)| / T = %.3f" % worst)
    assert worst < 1.0
    if not restated:
        assert worst < 1e-6                                       # float64 against itself: only the sums' last bits


def _pair_with_ties(metric="euclidean"):
    """70 x 80 frames of dim 20: Y[5:75] is X, so the diagonal j = i + 5 costs nothing, and X repeats one frame four
    times, so a 4 x 4 block of that diagonal is all zeros and its cells tie."""
    X, _ = K.make_pair("mfcc", 70, 80, 20, 11)
    _, Y = K.make_pair("mfcc", 70, 80, 20, 12)
    X[:, 30:34] = X[:, 30:31]
    Y[:, 5:75] = X
    return X, Y


def test_rejects_a_cell_moved_by_three_tolerances():
    for metric in K.METRICS:
        X, Y = K.make_pair("normal", 65, 71, 20, 3)
        args, _ = _result(X, Y, metric, True)
        K.certify(**args)
        T = K.tolerance(R.local_cost(X, Y, metric), metric, 20)
        assert T[40, 37] > 0
        for sign in (1.0, -1.0):
            D = args["D"].copy()
            D[40, 37] += sign * 3.0 * T[40, 37]
            with pytest.raises(AssertionError, match=r"\(c\) cell \(4[01], 3[78]\)"):
                K.certify(**dict(args, D=D))


@pytest.mark.parametrize("metric", K.METRICS)
def test_rejects_a_strip_boundary_cell_fed_from_the_wrong_column(metric):
    """Row 64 is lane 0 of the second strip: its (i-1, j) predecessor comes from the boundary row.  The mutation gives one
    cell of that row the value it has when that predecessor is read one column to the left."""
    X, Y = K.make_pair("normal", 130, 72, 20, 5)
    args, _ = _result(X, Y, metric, True)
    K.certify(**args)
    D = args["D"]
    c = K.kernel_local_cost(X, Y, metric).astype(np.float64)
    T = K.tolerance(R.local_cost(X, Y, metric), metric, 20)
    j = np.arange(1, 72)
    wrong = np.minimum(np.minimum(D[63, j - 1], D[64, j - 1]), D[63, j - 1]) + c[64, j]
    move = np.abs(wrong - D[64, j]) / T[64, j]
    jj = int(j[np.argmax(move)])
    assert move.max() > 3.0, move.max()                           # the shifted read changes this cell by more than 3 T
    Dm = D.copy()
    Dm[64, jj] = wrong[jj - 1]
    with pytest.raises(AssertionError, match=r"\(c\) cell \(6[45], "):
        K.certify(**dict(args, D=Dm))


def test_rejects_a_path_step_flipped_at_an_exact_tie():
    X, Y = _pair_with_ties()
    n, m = 70, 80
    C = K.kernel_local_cost(X, Y, "euclidean").astype(np.float64)
    D, codes, cost, wp, st = R.dtw_vec(C)
    St, wa, wm = S.step_table()
    args = dict(D=D, wp=wp, cost=cost, cost_no_backtrack=cost, X=X, Y=Y, metric="euclidean", St=St, wa=wa, wm=wm)
    K.certify(**args)
    # a path cell whose diagonal (step 0, taken) and left (step 1) predecessors hold the same double
    ties = [(i, j) for i, j in wp[:-1] if i > 0 and j > 0 and codes[i, j] == 0 and D[i - 1, j - 1] == D[i, j - 1]]
    assert ties, "the input was built to tie on the path"
    i, j = ties[0]
    flipped = codes.copy()
    flipped[i, j] = 1
    wp2 = R.backtrack(flipped)                                     # a complete, valid path through the other predecessor
    assert abs(R.path_cost(C, wp2) - cost) <= 1e-9 * cost and not np.array_equal(wp2, wp)
    with pytest.raises(AssertionError, match=r"\(d\) path step \d+ at \(%d, %d\): step 0 .* is listed before the step taken" % (i, j)):
        K.certify(**dict(args, wp=wp2))


def test_rejects_a_band_one_diagonal_too_wide():
    X, Y = K.make_pair("normal", 65, 71, 20, 3)
    r = R.band_radius(65, 71, 0.25)
    args, _ = _result(X, Y, "euclidean", True, radius=r)
    K.certify(**args)
    wide, _ = _result(X, Y, "euclidean", True, radius=r + 1)
    with pytest.raises(AssertionError, match=r"\(a\) reachability"):
        K.certify(**dict(wide, radius=r))
    with pytest.raises(AssertionError, match=r"\(a\) reachability"):
        K.certify(**dict(args, radius=r + 1))                      # and one too narrow


def test_rejects_a_subsequence_end_at_the_second_minimum():
    X, Y = K.make_pair("normal", 64, 200, 20, 9)
    args, codes = _result(X, Y, "euclidean", True, **MODES["weighted-sub"])
    K.certify(**args)
    D = args["D"]
    second = int(np.argsort(D[-1], kind="stable")[1])
    wp2 = S.backtrack(codes, args["St"], second, True)
    with pytest.raises(AssertionError, match=r"\(d\) the path starts at"):
        K.certify(**dict(args, wp=wp2, cost=D[-1, second], cost_no_backtrack=D[-1, second]))
    # all-zero features: every cell of the last row ties at 0, and the end must be the first of them
    Z = np.ones((3, 5), np.float32), np.ones((3, 9), np.float32)
    zargs, zcodes = _result(Z[0], Z[1], "euclidean", True, subseq=True)
    K.certify(**zargs)
    assert zargs["wp"][0, 1] == 0
    with pytest.raises(AssertionError, match=r"\(d\) the path starts at"):
        K.certify(**dict(zargs, wp=S.backtrack(zcodes, zargs["St"], 6, True)))


def test_rejects_a_cost_off_by_one_bit():
    X, Y = K.make_pair("mfcc", 65, 71, 39, 3)
    args, _ = _result(X, Y, "cosine", True)
    K.certify(**args)
    for field in ("cost", "cost_no_backtrack"):
        for to in (np.inf, -np.inf):
            with pytest.raises(AssertionError, match=r"\(e\) cost"):
                K.certify(**dict(args, **{field: np.nextafter(args[field], to)}))


def test_rejects_a_path_that_leaves_the_step_list():
    X, Y = K.make_pair("normal", 65, 71, 20, 3)
    args, _ = _result(X, Y, "euclidean", True, **MODES["weighted"])
    K.certify(**args)
    wp = args["wp"]
    t = len(wp) // 2
    detour = np.concatenate([wp[:t + 1], [[wp[t, 0], wp[t, 1] - 1]], wp[t + 1:]])      # a (0, 1) step: not in SLOPE
    with pytest.raises(AssertionError, match=r"\(d\) "):
        K.certify(**dict(args, wp=detour))


@pytest.mark.parametrize("metric", K.METRICS)
def test_float32_rounding_stays_inside_the_tolerance(metric):
    """Over the GPU grid's own inputs the restated float32 local cost stays below T -- the bound is derived for the worst
    case, so plain rounding must use well under all of it -- and is exactly 0 where C is 0 (Euclidean metrics)."""
    worst = 0.0
    for dim in K.DIMS:
        top = 0.0
        for X, Y in K.grid_pairs(dim):
            C = R.local_cost(X, Y, metric)
            T = K.tolerance(C, metric, dim)
            c32 = K.kernel_local_cost(X, Y, metric).astype(np.float64)
            assert (c32[T == 0] == 0).all()
            if (T > 0).any():
                top = max(top, float((np.abs(c32 - C)[T > 0] / T[T > 0]).max()))
        print("restated %-11s dim %3d width %3d  max |c32 - C| / T = %.3f" % (metric, dim, K.compiled_width(dim), top))
        worst = max(worst, top)
    print("restated %-11s maximum over the grid = %.3f" % (metric, worst))
    assert worst < 1.0


def test_grid_inputs_hold_repeats_copies_and_no_zero_frame():
    for dim in (1, 20, 128):
        for p, (X, Y) in enumerate(K.grid_pairs(dim)):
            assert X.dtype == Y.dtype == np.float32 and (X.shape[1], Y.shape[1]) == K.SHAPES[p]
            assert np.isfinite(X).all() and np.isfinite(Y).all()
            assert (np.abs(X).max(axis=0) > 0).all() and (np.abs(Y).max(axis=0) > 0).all()      # no zero-norm frame
            if p > 0:
                C = R.local_cost(X, Y, "sqeuclidean")
                assert (C == 0).any()                             # a block of Y is a copy of X
            if X.shape[1] >= 4:
                assert (np.abs(np.diff(X, axis=1)).sum(axis=0) == 0).any()                       # a run of repeated frames
    assert [K.compiled_width(d) for d in K.DIMS] == [8, 8, 16, 16, 24, 24, 24, 40, 40, 64, 64, 128, 128]
